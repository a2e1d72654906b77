"""The y,z form of the half-resolution fused Winograd kernel (wino_fused16_kernel<..., XD = true>: F(2x2,3x3) in y and z, a
plain 3-tap convolution along x; SP3D_CONV3_WINO_YZ on sp3d_wino_fused_split64 / sp3d_wino_fused_split64_skip), through
_lib.wino_fused_conv3d_(..., U3, U3yz=...), channels-last fp32.

Grids (the kernel's output block is 8x8x2):
  one_block  B=1,  8x8x2   exactly one block, the interior epilogue;
  ragged     B=1,  9x7x3   edge blocks and partial tiles in all three dimensions, the bounds-checked epilogue;
  many       B=2, 16x8x4   several blocks per axis and the batch stride.
Cases: C in {32, 64} x modes 0..3, and the folded skip (C = 64, CS = 32, relu(conv3(x) + WS . xs + shift)).

Every result lands in the middle of a buffer filled with a NaN of a bit pattern no computation produces, with guard zones on
both sides: an output the kernel did not write keeps the pattern, a write outside the result changes a guard.

Referee: F.conv3d in float64 on the GPU plus the same epilogue, once per (grid, C); error = max |got - f64| / max(1, max |f64|).
  * bound of this route, tests/test_gpu_v2v_plan_f64.py BOUNDS["wino_fused_conv3d_"] = 2.3e-6;
  * at most 1.5x the error of the shipped 64-point form on the same inputs (SP3D_WINO_YZ=0, same run, same referee), with a
    floor of one fp32 ulp of the output range, in the error's unit: where the shipped form is within an ulp, so may this be.
SP3D_WINO_YZ_RECORD=<file.json>: write the measured errors (profiles/r22_wino_yz_errors.json)."""
import ctypes as C
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

GRIDS = {"one_block": (1, 8, 8, 2), "ragged": (1, 9, 7, 3), "many": (2, 16, 8, 4)}
BOUND = 2.3e-6
O, CS = 64, 32
GUARD = 4096                                   # floats on either side of a result
PATTERN = 0x7FC0DEAD                           # a quiet NaN with a payload: no arithmetic result carries it
_cache = {}


def make_case(grid, Cc):
    """inputs, records of both forms and the float64 conv of a (grid, C): made once, never written"""
    key = (grid, Cc)
    if key not in _cache:
        from selfpose3d_amd import _lib
        B, X, Y, Z = GRIDS[grid]
        g = torch.Generator().manual_seed(1000 * Cc + 7 * X + Y)
        cl = torch.channels_last_3d
        c = dict(x=torch.randn(B, Cc, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 res=torch.randn(B, O, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 xs=torch.randn(B, CS, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 w=(torch.randn(O, Cc, 3, 3, 3, generator=g) / (27 * Cc) ** 0.5).cuda(),
                 ws=(torch.randn(O, CS, 1, 1, 1, generator=g) / CS ** 0.5).cuda(),
                 shift=(0.5 * torch.randn(O, generator=g)).cuda())
        c["U"] = _lib.wino_weights(c["w"])
        c["U3"] = _lib.wino_weights_split(c["U"], 16)
        c["U3yz"] = _lib.wino_yz_weights_split(c["w"])
        c["S"] = _lib.wino_weights_split(c["ws"].reshape(O, CS).t().reshape(1, CS, O).contiguous(), 16)
        c["conv64"] = conv64(c, c["x"])
        _cache[key] = c
    return _cache[key]


def conv64(c, x):
    return F.conv3d(x.double(), c["w"].double(), padding=1) + c["shift"].double().view(1, -1, 1, 1, 1)


def epilogue64(c, conv, mode, xs=None):
    """mode 0 shift, 1 relu(shift), 2 relu(shift + res), 3 relu(shift) + res; "skip": relu(. + WS . xs)"""
    if mode == "skip":
        return F.relu(conv + F.conv3d((c["xs"] if xs is None else xs).double(), c["ws"].double()))
    r = c["res"].double()
    return (conv, F.relu(conv), F.relu(conv + r), F.relu(conv) + r)[mode]


def guarded(c):
    """(buffer, the result view in its middle) - everything holds PATTERN"""
    B, _, X, Y, Z = c["x"].shape
    n = B * O * X * Y * Z
    buf = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    out = buf[GUARD:GUARD + n].view(B, X, Y, Z, O).permute(0, 4, 1, 2, 3)
    return buf, out


def check_guards(buf, out):
    bits = buf.view(torch.int32)
    n = out.numel()
    assert bool((bits[:GUARD] == PATTERN).all()) and bool((bits[GUARD + n:] == PATTERN).all()), "a write outside the result"
    assert not bool((bits[GUARD:GUARD + n] == PATTERN).any()), "an output the kernel never wrote"


def run(c, mode, yz=True, x=None, xs=None):
    """the layer through the binding into a guarded buffer; yz=False: the same call without the records of the new form"""
    from selfpose3d_amd import _lib
    buf, out = guarded(c)
    kw = dict(U3yz=c["U3yz"]) if yz else {}
    x = c["x"] if x is None else x
    if mode == "skip":
        y = _lib.wino_fused_conv3d_(x, c["U"], c["shift"], 1, None, c["U3"], xs=c["xs"] if xs is None else xs, skip_w=c["S"],
                                    out=out, **kw)
    else:
        y = _lib.wino_fused_conv3d_(x, c["U"], c["shift"], mode, c["res"] if mode >= 2 else None, c["U3"], out=out, **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    check_guards(buf, out)
    return y


def err(got, ref):
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def ulp_floor(ref):
    """one fp32 ulp of the largest output, in the unit of err()"""
    m = float(ref.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 23) / max(1.0, m)


CASES = [(g, Cc, m) for g in GRIDS for Cc in (32, 64) for m in (0, 1, 2, 3)] + [(g, 64, "skip") for g in GRIDS]


@pytest.fixture(autouse=True)
def yz_on(monkeypatch):
    monkeypatch.delenv("SP3D_WINO_YZ", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("grid,Cc,mode", CASES, ids=["%s-c%d-%s" % t for t in CASES])
def test_yz_form_against_float64_and_the_shipped_form(grid, Cc, mode, monkeypatch):
    c = make_case(grid, Cc)
    ref = epilogue64(c, c["conv64"], mode)
    got = run(c, mode)
    monkeypatch.setenv("SP3D_WINO_YZ", "0")
    old = run(c, mode)
    monkeypatch.delenv("SP3D_WINO_YZ")
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.stride() == old.stride()
    e_new, e_old, floor = err(got, ref), err(old, ref), ulp_floor(ref)
    print(f"{grid} C={Cc} mode={mode}: shipped {e_old:.3e}  yz {e_new:.3e}  ulp {floor:.3e}  bound {BOUND:.1e}")
    path = os.environ.get("SP3D_WINO_YZ_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec["%s-c%d-%s" % (grid, Cc, mode)] = dict(grid=list(GRIDS[grid]), C=Cc, mode=mode, shipped=e_old, yz=e_new, ulp_floor=floor,
                                                   bound=BOUND)
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
    assert float((got - old).abs().max()) > 0.0 or e_old == 0.0, "the switch selected nothing: both runs are the same kernel"
    assert e_new <= BOUND, (e_new, BOUND)
    assert e_new <= max(1.5 * e_old, floor), (e_new, e_old, floor)


@pytest.mark.gpu
@pytest.mark.parametrize("Cc,mode", [(32, 1), (64, 2), (64, "skip")])
def test_switch_off_is_the_shipped_entry_bit_for_bit(Cc, mode, monkeypatch):
    """SP3D_WINO_YZ=0 with the new records at hand == a direct call of the C entry without the flag"""
    from selfpose3d_amd import _lib
    c = make_case("ragged", Cc)
    monkeypatch.setenv("SP3D_WINO_YZ", "0")
    got = run(c, mode, yz=True)
    lib = _lib.load()
    B, _, X, Y, Z = c["x"].shape
    buf, out = guarded(c)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    if mode == "skip":
        rc = lib.sp3d_wino_fused_split64_skip(p(c["x"]), p(c["U3"]), p(out), p(c["shift"]), p(c["xs"]), p(c["S"]), B, X, Y, Z, Cc, O,
                                              CS, s)
    else:
        rc = lib.sp3d_wino_fused_split64(p(c["x"]), p(c["U3"]), p(out), p(c["shift"]), p(c["res"]) if mode >= 2 else None, mode,
                                         B, X, Y, Z, Cc, O, s)
    torch.cuda.synchronize()
    assert rc == 0
    check_guards(buf, out)
    assert torch.equal(got, out)
    assert torch.equal(got, run(c, mode, yz=False))               # ... and == the call that never had the records


@pytest.mark.gpu
@pytest.mark.parametrize("grid,Cc,mode", [("ragged", 32, 0), ("many", 64, 0), ("ragged", 64, "skip")])
def test_one_nan_reaches_every_output_of_its_window(grid, Cc, mode):
    """one NaN in x: every output whose 3x3x3 window holds it is NaN, all 64 channels (mode 0 and the folded skip, whose ReLU
    keeps NaN; the ReLU of the other modes is fmaxf, which does not); nothing non-finite outside the Winograd tiles around
    it, and the guards stay"""
    c = make_case(grid, Cc)
    B, _, X, Y, Z = c["x"].shape
    at = (B - 1, Cc - 5, X - 2, 3, 1)
    x = c["x"].clone()
    x[at] = float("nan")
    got = run(c, mode, x=x)
    nan = torch.isnan(got)
    b, _, px, py, pz = at
    win = torch.zeros_like(nan)
    win[b, :, max(px - 1, 0):px + 2, max(py - 1, 0):py + 2, max(pz - 1, 0):pz + 2] = True
    assert int(win.sum()) >= 64 * 12
    assert bool((nan & win).sum() == win.sum()), "an output whose window holds the NaN is finite"
    # a y,z tile is 2x2 outputs reading 4x4 inputs: the NaN can reach at most one more output on either side in y and z
    reach = torch.zeros_like(nan)
    reach[b, :, max(px - 1, 0):px + 2, max(py - 2, 0):py + 3, max(pz - 2, 0):pz + 3] = True
    assert not bool((~torch.isfinite(got) & ~reach).any()), "a NaN far from its source"
    clean = run(c, mode)
    assert torch.equal(got[~reach], clean[~reach])


@pytest.mark.gpu
def test_binding_refuses_other_records():
    from selfpose3d_amd import _lib
    c = make_case("one_block", 64)
    with pytest.raises(_lib.Sp3dError):
        _lib.wino_fused_conv3d_(c["x"], c["U"], c["shift"], 1, None, c["U3"], U3yz=c["U3"])            # 64 points: the other form
    with pytest.raises(_lib.Sp3dError):
        _lib.wino_fused_conv3d_(c["x"], c["U"], c["shift"], 1, None, c["U3"], U3yz=c["U3yz"].float())  # another type
    with pytest.raises(_lib.Sp3dError):
        _lib.wino_fused_conv3d_(c["x"], c["U"], c["shift"], 1, None, c["U3"], U3yz=c["U3yz"].cpu())


@pytest.mark.gpu
def test_plan_routes_the_half_resolution_layers_to_the_yz_form(monkeypatch):
    """the plan hands the 48-point records to wino_fused_conv3d_ for its 32 -> 64 and 64 -> 64 layers and to no other layer,
    and SP3D_WINO_YZ=0 gives the forward of the shipped form, close to it but not equal"""
    from selfpose3d_amd import _lib
    from selfpose3d_amd.v2v_net import V2VNet
    torch.manual_seed(5)
    net = V2VNet(15, 1)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():      # unit-gain weights: in the fresh net (std 0.001) a layer's conv term fades below an ulp of its shift
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._NormBase):
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
            elif isinstance(m, torch.nn.ConvTranspose3d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[0] ** 0.5)
            elif isinstance(m, torch.nn.Conv3d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight[0].numel() ** 0.5)
    net.eval().cuda().to(memory_format=torch.channels_last_3d)
    x = torch.rand(1, 15, 16, 16, 8, generator=g).cuda()
    seen, wf = [], _lib.wino_fused_conv3d_

    def spy(x_, U, *a, **k):
        seen.append((int(x_.shape[1]), int(U.shape[2]), k.get("U3yz") is not None))
        return wf(x_, U, *a, **k)
    monkeypatch.setattr(_lib, "wino_fused_conv3d_", spy)
    with torch.no_grad():
        y_on = net(x).clone()
    assert seen and all(have == (o == 64) for _, o, have in seen), seen
    assert sorted({(ci, o) for ci, o, have in seen if have}) == [(32, 64), (64, 64)], seen
    monkeypatch.setenv("SP3D_WINO_YZ", "0")
    with torch.no_grad():
        y_off = net(x).clone()
    torch.cuda.synchronize()
    # six layers change form, each within BOUND of float64 in either form: 6 x 2 x 2.3e-6 were the differences to add up
    scale = max(1.0, float(y_off.abs().max()))
    assert 0.0 < float((y_on - y_off).abs().max()) / scale <= 12 * BOUND
