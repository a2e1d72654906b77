"""The 1x1x1 skip projection of a channel-changing residual block on the accumulators of the block's second 3x3x3 conv:
_lib.conv3_split_ (32 -> 32 with a skip from 16, sp3d_conv3_split_skip) and _lib.wino_fused_conv3d_ with split weights
(64 -> 64 with a skip from 32, sp3d_wino_fused_split64_skip), through the trailing keyword arguments (xs, skip_w).

Referee: relu(F.conv3d(h, w2, padding=1) + F.conv3d(xs, ws) + shift) in float64 on the GPU, once per case.  Error =
max |got - f64| / max(1, max |f64|).  Two bounds: the kernel's own from tests/test_gpu_v2v_plan_f64.py (4.7e-6 conv3_split_,
2.3e-6 wino_fused_conv3d_) and at most 1.5x the error of the path the fold replaces - library GEMM for the projection, then
the same kernel in mode 2 with the product as its residual - on the same inputs (the rule of
test_winograd_fused_split_kernel_has_fp32_accuracy).

Shapes:
  direct_edges  B=2, 20x12x6: per sample one interior 16x8x4 block and edge blocks in x, y, z and their combinations - both
                epilogue paths, clamped skip rows;
  direct_walk   B=3, 80x80x8: 300 interior blocks, more than the device has compute units, so persistent workgroups walk two
                blocks - a skip term dropped or doubled on the second block shows here and nowhere smaller;
  wino_edges    B=2, 12x10x3: one interior 8x8x2 block per sample + edges in all three axes;
  wino_interior B=1, 16x16x4: interior blocks only.

SP3D_SKIP_FOLD_RECORD=<file.json>: write the measured errors (profiles/r11_skip_fold_errors.json)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

CASES = {   # name: (kind, B, X, Y, Z)
    "direct_edges": ("direct", 2, 20, 12, 6),
    "direct_walk": ("direct", 3, 80, 80, 8),
    "wino_edges": ("wino", 2, 12, 10, 3),
    "wino_interior": ("wino", 1, 16, 16, 4),
}
WIDTHS = {"direct": (32, 32, 16), "wino": (64, 64, 32)}            # (C, O, CS)
BOUND = {"direct": 4.7e-6, "wino": 2.3e-6}
_cache = {}


def make_case(name):
    """inputs of a case (h, xs ~ N(0,1); weights scaled for unit-variance terms), its records and its float64 referee: made
    once, never written"""
    if name not in _cache:
        from selfpose3d_amd import _lib
        kind, B, X, Y, Z = CASES[name]
        Cc, O, CS = WIDTHS[kind]
        g = torch.Generator().manual_seed(23)
        cl = torch.channels_last_3d
        c = dict(kind=kind,
                 h=torch.randn(B, Cc, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 xs=torch.randn(B, CS, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 w2=(torch.randn(O, Cc, 3, 3, 3, generator=g) / (27 * Cc) ** 0.5).cuda(),
                 ws=(torch.randn(O, CS, 1, 1, 1, generator=g) / CS ** 0.5).cuda(),
                 shift=(0.5 * torch.randn(O, generator=g)).cuda())
        if kind == "direct":
            c["W"] = _lib.conv_weights_split(c["w2"])
            c["S"] = _lib.conv_weights_split(c["ws"])
        else:
            c["U"] = _lib.wino_weights(c["w2"])
            c["W"] = _lib.wino_weights_split(c["U"], 16)
            c["S"] = _lib.wino_weights_split(c["ws"].reshape(O, CS).t().reshape(1, CS, O).contiguous(), 16)
        c["ref"] = referee(c, c["xs"])
        pos = float((c["ref"] > 0).double().mean())
        assert 0.1 <= pos <= 0.9 and 0.5 <= float(c["ref"].max()) <= 20.0, (pos, float(c["ref"].max()))
        _cache[name] = c
    return _cache[name]


def referee(c, xs):
    return F.relu(F.conv3d(c["h"].double(), c["w2"].double(), padding=1) + F.conv3d(xs.double(), c["ws"].double())
                  + c["shift"].double().view(1, -1, 1, 1, 1))


def conv(c, mode, residual=None, xs=None, skip_w=None):
    from selfpose3d_amd import _lib
    if c["kind"] == "direct":
        return _lib.conv3_split_(c["h"], c["W"], c["shift"], mode, residual, xs=xs, skip_w=skip_w)
    return _lib.wino_fused_conv3d_(c["h"], c["U"], c["shift"], mode, residual, c["W"], xs=xs, skip_w=skip_w)


def folded(c, xs=None, skip_w=None):
    return conv(c, 1, xs=c["xs"] if xs is None else xs, skip_w=c["S"] if skip_w is None else skip_w)


def gemm_path(c):
    """what the plan ran before: the projection as a library GEMM on the channels-last view, mode 2 on its product"""
    xs, ws = c["xs"], c["ws"]
    B, CS, X, Y, Z = xs.shape
    O = ws.shape[0]
    p = torch.matmul(xs.permute(0, 2, 3, 4, 1).reshape(-1, CS), ws.reshape(O, CS).t()).view(B, X, Y, Z, O).permute(0, 4, 1, 2, 3)
    return conv(c, 2, residual=p)


def err(got, ref):
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def poison(like):
    """leave NaN in the free blocks the next results of ``like``'s size come from (allocate, fill, free)"""
    ts = [torch.full((like.numel(),), float("nan"), device=like.device) for _ in range(3)]
    torch.cuda.synchronize()
    del ts


@pytest.fixture(autouse=True)
def fold_on(monkeypatch):
    monkeypatch.delenv("SP3D_FOLD_SKIP", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_folded_skip_against_float64(name):
    c = make_case(name)
    ref = c["ref"]
    old = gemm_path(c)
    poison(old)
    got = folded(c)
    assert got.shape == ref.shape and got.stride() == old.stride() and got.dtype == torch.float32
    assert not bool(torch.isnan(got).any()), "an output the kernel never wrote"
    e_old, e_new = err(old, ref), err(got, ref)
    print(f"{name}: gemm + mode 2 {e_old:.3e}  folded {e_new:.3e}  bound {BOUND[c['kind']]:.1e}")
    path = os.environ.get("SP3D_SKIP_FOLD_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = dict(shape=list(CASES[name][1:]), widths=list(WIDTHS[c["kind"]]), gemm_mode2=e_old, folded=e_new,
                         bound=BOUND[c["kind"]])
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
    assert e_new <= BOUND[c["kind"]], (e_new, BOUND[c["kind"]])
    assert e_new <= 1.5 * e_old, (e_new, e_old)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["direct_edges", "wino_edges"])
def test_comparison_has_signal_from_the_skip_term(name):
    """zeroed records: the mode 1 kernel on h alone, within the bound; real records: far from it"""
    c = make_case(name)
    plain = conv(c, 1)
    zero = folded(c, skip_w=torch.zeros_like(c["S"]))
    scale = max(1.0, float(plain.abs().max()))
    assert float((zero - plain).abs().max()) / scale <= BOUND[c["kind"]]
    spread = float(c["ref"].max() - c["ref"].min())
    assert float((folded(c) - plain).abs().max()) > 1e-3 * spread


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["direct_edges", "wino_edges"])
def test_folded_skip_nonfinite_inputs(name):
    """one +inf and one NaN in xs reach the outputs of their own voxel and nothing else (a 1x1x1 term).  The NaN voxel: all O
    channels.  The inf voxel: every output the float64 referee has non-finite - a negative weight makes -inf, which ReLU turns
    into 0, and the split product may turn an inf into NaN, which ReLU lets through: both stay inside the voxel."""
    c = make_case(name)
    kind, B, X, Y, Z = CASES[name]
    CS = WIDTHS[kind][2]
    xs = c["xs"].clone()
    v_inf, v_nan = (0, 1, 2, 1), (B - 1, X - 1, Y - 2, 0)          # an interior-block voxel, an edge-block voxel
    xs[v_inf[0], 5, v_inf[1], v_inf[2], v_inf[3]] = float("inf")
    xs[v_nan[0], CS - 3, v_nan[1], v_nan[2], v_nan[3]] = float("nan")
    got = folded(c, xs=xs)
    bad = ~torch.isfinite(got)
    ref_bad = ~torch.isfinite(referee(c, xs))

    def voxel(v):
        m = torch.zeros_like(bad)
        m[v[0], :, v[1], v[2], v[3]] = True
        return m
    m_inf, m_nan = voxel(v_inf), voxel(v_nan)
    assert int(m_nan.sum()) == got.shape[1]
    assert bool((torch.isnan(got) & m_nan).sum() == m_nan.sum()), "NaN voxel: every channel"
    assert not bool((bad & ~(m_inf | m_nan)).any()), "a neighbour is non-finite"
    assert bool(ref_bad.any()) and not bool((ref_bad & ~bad).any()), "a non-finite output of the layer came out finite"
    keep = ~(m_inf | m_nan)
    assert torch.equal(got[keep], folded(c)[keep])


@pytest.mark.gpu
def test_binding_refuses_incomplete_skip_operands():
    from selfpose3d_amd import _lib
    c = make_case("direct_edges")
    with pytest.raises(_lib.Sp3dError):
        conv(c, 1, xs=c["xs"])                                     # no records
    with pytest.raises(_lib.Sp3dError):
        conv(c, 2, residual=c["h"], xs=c["xs"], skip_w=c["S"])     # a residual next to the skip
    with pytest.raises(_lib.Sp3dError):
        conv(c, 0, xs=c["xs"], skip_w=c["S"])                      # the folded form is relu(. + shift) only
    with pytest.raises(_lib.Sp3dError):
        conv(c, 1, xs=c["xs"], skip_w=c["S"][:, :1].contiguous())  # half the records
    with pytest.raises(_lib.Sp3dError):
        conv(c, 1, xs=c["xs"][:, :, :8].contiguous(memory_format=torch.channels_last_3d), skip_w=c["S"])   # another grid


def _plan_net():
    from selfpose3d_amd.v2v_net import V2VNet
    torch.manual_seed(31)
    net = V2VNet(15, 1)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._NormBase):
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
    net.eval().cuda().to(memory_format=torch.channels_last_3d)
    x = torch.rand(2, 15, 48, 48, 12, generator=g).cuda()
    return net, x


@pytest.mark.gpu
def test_switch_restores_the_gemm_path(monkeypatch):
    """SP3D_FOLD_SKIP=0: the plan's forward is, bit for bit, the forward with the fold taken out of the plan (GEMM + mode 2 in
    every block), and the two skip GEMMs 16 -> 32 and 32 -> 64 are called; without the switch they are not, the two entries
    get their skip operands, and the result agrees within the layers' bounds."""
    from selfpose3d_amd import _lib
    from selfpose3d_amd.v2v_net import _FoldedV2V
    net, x = _plan_net()
    gemms, skips = [], []
    matmul, c3, wf = torch.matmul, _lib.conv3_split_, _lib.wino_fused_conv3d_

    def mm(a, b):
        gemms.append((int(a.shape[-1]), int(b.shape[-1])))
        return matmul(a, b)

    def spy(fn, tag):
        def call(*a, **k):
            if k.get("xs") is not None:
                skips.append(tag)
            return fn(*a, **k)
        return call
    monkeypatch.setattr(torch, "matmul", mm)
    monkeypatch.setattr(_lib, "conv3_split_", spy(c3, "direct"))
    monkeypatch.setattr(_lib, "wino_fused_conv3d_", spy(wf, "wino"))

    def forward():
        del gemms[:], skips[:]
        with torch.no_grad():
            y = net(x).clone()
        torch.cuda.synchronize()
        return y, sorted(gemms), sorted(skips)
    y_on, g_on, s_on = forward()
    assert (16, 32) not in g_on and (32, 64) not in g_on and s_on == ["direct", "wino"], (g_on, s_on)
    monkeypatch.setenv("SP3D_FOLD_SKIP", "0")
    y_off, g_off, s_off = forward()
    assert g_off.count((16, 32)) == 1 and g_off.count((32, 64)) == 1 and s_off == [], (g_off, s_off)
    monkeypatch.delenv("SP3D_FOLD_SKIP")
    monkeypatch.setattr(_FoldedV2V, "_folded_skip", lambda self, x, h, r: None)      # the plan as it was before the fold
    y_old, g_old, s_old = forward()
    assert g_old == g_off and s_old == []
    assert torch.equal(y_off, y_old)
    scale = max(1.0, float(y_old.abs().max()))
    assert 0.0 < float((y_on - y_old).abs().max()) / scale <= 6.0e-6
