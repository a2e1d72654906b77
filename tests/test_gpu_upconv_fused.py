"""sp3d_upconv2x_fused (ConvTranspose3d(2, stride 2) + shift + ReLU + skip [+ 1x1x1 output conv] in one kernel) through the
two entries that launch it, _lib.upsample2x_ and _lib.upsample2x_head_ with ``w_split``.

Referee: F.conv_transpose3d + shift + ReLU + skip (+ conv3d for the head) in float64 on the GPU.  The bound is not a number
chosen in advance: the same entry WITHOUT ``w_split`` (library fp32 GEMM + scatter kernel) is measured on the same inputs and
the one-kernel form may have at most 1.5x its error - the margin test_winograd_fused_split_kernel_has_fp32_accuracy gives the
same split arithmetic.  Error = max |got - ref| / max |ref|.

Shapes: the smallest that reach every path of the kernel -
  head64  (B=2, 64 -> 32, 6x5x3, J in 1, 9, 15): 180 voxels = one full 128-voxel tile + a ragged one (a full wave, a partly
          filled wave, two empty waves); one workgroup per tile walks all 8 taps;
  plain   (B=1, 128 -> 64, 5x5x2, no head): 50 voxels < one tile, two K stages, two accumulators, the taps split over 8 workgroups;
  tile    (B=1, 64 -> 32, 8x8x2, J=1): exactly one full tile, interior stores only;
  multi   (B=1, 32x24x20, both layers): 120 tiles, the smallest count at which a workgroup walks more than one tap (two) and
          fetches the next tap's skip rows ahead - the instantiation the plan's large grids run.

SP3D_UPCONV_FUSED_RECORD=<file.json>: write the measured errors (profiles/r10_upconv_fused_errors.json)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

CASES = {   # name: (B, Cin, X, Y, Z, O, J | None)
    "head64_J1": (2, 64, 6, 5, 3, 32, 1),
    "head64_J9": (2, 64, 6, 5, 3, 32, 9),
    "head64_J15": (2, 64, 6, 5, 3, 32, 15),
    "plain128": (1, 128, 5, 5, 2, 64, None),
    "tile64_J1": (1, 64, 8, 8, 2, 32, 1),
    "head64_multi": (1, 64, 32, 24, 20, 32, 2),
    "plain128_multi": (1, 128, 32, 24, 20, 64, None),
}
_cache = {}


def make_case(name):
    """inputs of a case (randn; weights 0.1 randn), made once and never written"""
    if name not in _cache:
        from selfpose3d_amd import _lib
        B, Cin, X, Y, Z, O, J = CASES[name]
        g = torch.Generator().manual_seed(11)
        cl = torch.channels_last_3d
        c = dict(x=torch.randn(B, Cin, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 wT=(0.1 * torch.randn(Cin, O, 2, 2, 2, generator=g)).cuda(), shift=torch.randn(O, generator=g).cuda(),
                 skip=torch.randn(B, O, 2 * X, 2 * Y, 2 * Z, generator=g).cuda().contiguous(memory_format=cl), wo=None, bo=None)
        if J is not None:
            c["wo"] = (0.1 * torch.randn(J, O, 1, 1, 1, generator=g)).cuda()
            c["bo"] = torch.randn(J, generator=g).cuda()
        c["wg"] = c["wT"].permute(0, 2, 3, 4, 1).reshape(Cin, 8 * O).contiguous()      # columns (i,j,k,o): _FoldedV2V._build
        c["w3"] = _lib.upconv_weights_split(c["wg"])
        _cache[name] = c
    return _cache[name]


def referee(c, x=None):
    x = c["x"] if x is None else x
    y = F.relu(F.conv_transpose3d(x.double(), c["wT"].double(), None, 2) + c["shift"].double().view(1, -1, 1, 1, 1)) + c["skip"].double()
    return y if c["wo"] is None else F.conv3d(y, c["wo"].double(), c["bo"].double())


def run(c, fused, x=None):
    from selfpose3d_amd import _lib
    x = c["x"] if x is None else x
    w3 = c["w3"] if fused else None
    if c["wo"] is None:
        return _lib.upsample2x_(x, c["wg"], c["shift"], c["skip"], w_split=w3)
    return _lib.upsample2x_head_(x, c["wg"], c["shift"], c["skip"], c["wo"], c["bo"], w_split=w3)


def poison(like):
    """leave NaN in the free blocks the next results of ``like``'s size come from (allocate, fill, free)"""
    ts = [torch.full((like.numel(),), float("nan"), device=like.device) for _ in range(3)]
    torch.cuda.synchronize()
    del ts


@pytest.fixture(autouse=True)
def fused_on(monkeypatch):
    monkeypatch.delenv("SP3D_FUSE_UPCONV", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fused_upconv_against_float64(name):
    """one-kernel form <= 1.5 x the error of the GEMM + scatter form against float64, with no NaN from unwritten tiles"""
    c = make_case(name)
    ref = referee(c)
    scale = float(ref.abs().max())
    old = run(c, False)
    poison(old)
    got = run(c, True)
    assert got.shape == ref.shape and got.stride() == old.stride() and got.dtype == torch.float32
    assert not bool(torch.isnan(got).any()), "a tile the kernel never wrote"
    e_old = float((old.double() - ref).abs().max()) / scale
    e_new = float((got.double() - ref).abs().max()) / scale
    print(f"{name}: gemm+scatter {e_old:.3e}  fused {e_new:.3e}")
    path = os.environ.get("SP3D_UPCONV_FUSED_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = dict(shape=list(CASES[name]), gemm_scatter=e_old, fused=e_new)
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
    assert e_new <= 1.5 * e_old, (e_new, e_old)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["head64_J9", "plain128"])
def test_fused_upconv_nonfinite_inputs(name):
    """one inf and one NaN in x reach the 8 output voxels of their own input voxel and nothing else.  The NaN voxel: all of
    its 8 x O (8 x J) outputs.  The inf voxel: with the head all 8 x J (a dot product over 32 channels of which the positive
    weights' are +inf); without it every output the float64 referee has non-finite - a negative weight makes -inf, which
    ReLU turns into 0, so 'all 8 x O' is not what the layer computes - and no output outside its 8 voxels (the split
    product may turn a -inf into NaN, which ReLU lets through: those stay inside the voxel's outputs too)."""
    c = make_case(name)
    B, Cin, X, Y, Z, O, J = CASES[name]
    x = c["x"].clone()
    v_inf, v_nan = (0, 1, 2, 1), (B - 1, X - 1, Y - 2, 0)
    x[v_inf[0], 5, v_inf[1], v_inf[2], v_inf[3]] = float("inf")
    x[v_nan[0], Cin - 3, v_nan[1], v_nan[2], v_nan[3]] = float("nan")
    got = run(c, True, x)
    bad = ~torch.isfinite(got)
    ref_bad = ~torch.isfinite(referee(c, x))

    def block(v):
        m = torch.zeros_like(bad)
        m[v[0], :, 2 * v[1]:2 * v[1] + 2, 2 * v[2]:2 * v[2] + 2, 2 * v[3]:2 * v[3] + 2] = True
        return m
    m_inf, m_nan = block(v_inf), block(v_nan)
    assert int(m_nan.sum()) == 8 * got.shape[1]
    assert bool((bad & m_nan).sum() == m_nan.sum()), "NaN voxel: every output"
    assert not bool((bad & ~(m_inf | m_nan)).any()), "a neighbour is non-finite"
    assert not bool((ref_bad & ~bad).any()), "a non-finite output of the layer came out finite"
    if J is not None:
        assert bool((bad & m_inf).sum() == m_inf.sum()), "inf voxel under the head: every output"
    # everything else is what it was without the two values
    clean = run(c, True)
    keep = ~(m_inf | m_nan)
    assert torch.equal(got[keep], clean[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("head", [False, True])
def test_uncovered_shape_takes_the_gemm_path(head):
    """CIN = 48 is not a shape of the kernel: with w_split the entries run GEMM + scatter, bit for bit"""
    from selfpose3d_amd import _lib
    g = torch.Generator().manual_seed(5)
    cl = torch.channels_last_3d
    B, Cin, X, Y, Z, O = 1, 48, 3, 4, 2, 32
    x = torch.randn(B, Cin, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl)
    wg = (0.1 * torch.randn(Cin, 8 * O, generator=g)).cuda()
    shift = torch.randn(O, generator=g).cuda()
    skip = torch.randn(B, O, 2 * X, 2 * Y, 2 * Z, generator=g).cuda().contiguous(memory_format=cl)
    w3 = _lib.upconv_weights_split(wg)
    assert not _lib.upconv_fused_covers(Cin, O, head)
    if head:
        wo, bo = torch.randn(1, O, 1, 1, 1, generator=g).cuda(), torch.randn(1, generator=g).cuda()
        a, b = _lib.upsample2x_head_(x, wg, shift, skip, wo, bo), _lib.upsample2x_head_(x, wg, shift, skip, wo, bo, w_split=w3)
    else:
        a, b = _lib.upsample2x_(x, wg, shift, skip), _lib.upsample2x_(x, wg, shift, skip, w_split=w3)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["head64_J9", "plain128"])
def test_switch_forces_the_gemm_path(name, monkeypatch):
    """SP3D_FUSE_UPCONV=0: a covered shape with w_split runs GEMM + scatter, bit for bit; without the switch it does not"""
    from selfpose3d_amd import _lib
    c = make_case(name)
    old = run(c, False)
    B, Cin, X, Y, Z, O, J = CASES[name]
    assert _lib.upconv_fused_covers(Cin, O, J is not None)
    assert not torch.equal(run(c, True), old)          # the fused kernel sums in another order: some bits differ
    monkeypatch.setenv("SP3D_FUSE_UPCONV", "0")
    assert not _lib.upconv_fused_covers(Cin, O, J is not None)
    assert torch.equal(run(c, True), old)
