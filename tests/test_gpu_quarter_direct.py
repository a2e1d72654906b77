"""conv3_split128_kernel (csrc/sp3d_conv3_quarter.hip), the direct 3x3x3 convolution of the quarter-resolution layers, against
float64 F.conv3d + the epilogue.  Every output buffer is NaN before the launch, so a row the kernel does not write fails.
Metric and bound: max|got - f64| / max(1, max|f64|) <= 2.0e-6, the bound of the conv3_split128_ entry in the plan
(tests/test_gpu_v2v_plan_f64.py BOUNDS); with two samples of different magnitude it is taken per sample.
Measured on the MI355X (profiles/r15_quarter_direct_errors.json)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BOUND = 2.0e-6

# (B, C, grid, mode): one block exactly; ragged in every axis with two samples; several blocks along x and a z boundary inside
# the grid; both widths and all four epilogue modes
CASES = [(1, 64, (5, 5, 5), 0), (2, 128, (7, 6, 3), 2), (1, 128, (11, 5, 6), 3), (1, 64, (11, 5, 6), 1), (2, 64, (7, 6, 3), 1)]


def metric(got, ref):
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@functools.lru_cache(maxsize=None)
def case(B, C, grid, mode):
    """inputs on the GPU and the float64 reference, once per case"""
    O = 128
    g = torch.Generator(device="cpu").manual_seed(1000 * C + 10 * sum(grid) + mode)
    x = torch.randn((B, C) + grid, generator=g)
    if B > 1:
        x[1:] *= 1.0e3             # a halo that reached into the neighbouring sample would swamp sample 0
    w = torch.randn((O, C, 3, 3, 3), generator=g) * 0.05
    shift = torch.randn((O,), generator=g)
    res = torch.randn((B, O) + grid, generator=g)
    ref = F.conv3d(x.double(), w.double(), padding=1) + shift.double().view(1, O, 1, 1, 1)
    if mode == 2:
        ref = ref + res.double()
    if mode >= 1:
        ref = ref.clamp_min(0)
    if mode == 3:
        ref = ref + res.double()
    cl = torch.channels_last_3d
    return (x.cuda().contiguous(memory_format=cl), w.cuda(), shift.cuda(), res.cuda().contiguous(memory_format=cl), ref)


def run_direct(x, w, shift, res, mode):
    from selfpose3d_amd import _lib
    B, _, X, Y, Z = x.shape
    out = torch.full((B, 128, X, Y, Z), float("nan"), device=x.device).contiguous(memory_format=torch.channels_last_3d)
    y = _lib.conv3_split128_(x, _lib.conv_weights_split24(w), shift, mode, res if mode >= 2 else None, out=out)
    assert y is out and y.is_contiguous(memory_format=torch.channels_last_3d)
    return y.cpu()


@pytest.mark.parametrize("B,C,grid,mode", CASES)
def test_direct_kernel_against_float64(B, C, grid, mode):
    x, w, shift, res, ref = case(B, C, grid, mode)
    y = run_direct(x, w, shift, res, mode)
    assert bool(torch.isfinite(y).all())                 # every row written
    errs = [metric(y[b], ref[b]) for b in range(B)]
    print("quarter_direct", (B, C, grid, mode), errs)
    assert max(errs) <= BOUND, errs


def test_nonfinite_inputs_reach_exactly_the_outputs_of_a_convolution():
    """one +inf and one NaN activation, mode 0: non-finite are exactly the outputs a float64 convolution makes non-finite
    (the pattern of test_gpu_parity.py::test_direct_conv3_split_kernel_nonfinite_inputs)"""
    x, w, shift, res, _ = case(1, 128, (11, 5, 6), 0)
    x = x.clone()
    x[0, 5, 4, 2, 3] = float("inf")            # inside block 0, next to the block boundary at x = 5
    x[0, 77, 10, 4, 5] = float("nan")          # a corner of the grid, in the z block that holds one layer
    ref = F.conv3d(x.cpu().double(), w.cpu().double(), padding=1) + shift.cpu().double().view(1, -1, 1, 1, 1)
    y = run_direct(x, w, shift, res, 0)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(y), fin)
    assert int((~fin).sum()) == (27 + 8) * 128
    assert bool(torch.isnan(y)[torch.isnan(ref)].all())
    assert metric(torch.where(fin, y, torch.zeros_like(y)), torch.where(fin, ref, torch.zeros_like(ref))) <= BOUND


def test_direct_and_three_launch_forms_agree():
    """the same layer through the direct kernel and through the three-launch Winograd form: they differ by at most the sum
    of their two errors against float64"""
    from selfpose3d_amd import _lib
    x, w, shift, res, ref = case(1, 128, (11, 5, 6), 3)
    yd = run_direct(x, w, shift, res, 3)
    yw = _lib.wino_conv3d_(x, _lib.wino_weights(w), shift, 3, res).cpu()
    ed, ew = metric(yd, ref), metric(yw, ref)
    print("quarter_direct forms", ed, ew, metric(yd, yw.double()))
    assert ed <= BOUND
    assert metric(yd, yw.double()) <= ed + ew


def bare_plan():
    """a plan object with the default switches and no layers: _conv3 dispatches a record made by _conv3_record"""
    import types
    from selfpose3d_amd.v2v_net import _FoldedV2V
    return _FoldedV2V(types.SimpleNamespace(winograd=True, wino_split=True, direct_conv=True))


def test_plan_takes_the_direct_kernel_where_it_covers(monkeypatch):
    """the plan's dispatch (_conv3 on a record of _conv3_record) IS conv3_split128_ on a grid of whole 5x5x5 blocks (bit for
    bit) and stays the three launches on a ragged grid; each entry runs its own form only"""
    from selfpose3d_amd import _lib
    monkeypatch.delenv("SP3D_QUARTER_DIRECT", raising=False)
    g = torch.Generator(device="cpu").manual_seed(5)
    cl = torch.channels_last_3d
    w = (torch.randn((128, 64, 3, 3, 3), generator=g) * 0.05).cuda()
    shift = torch.randn((128,), generator=g).cuda()
    U, rec = _lib.wino_weights(w), _lib.conv_weights_split24(w)
    plan = bare_plan()
    c = plan._conv3_record(w, shift)
    assert torch.equal(c.u, U) and torch.equal(c.direct24, rec) and c.direct is None
    x = torch.randn((1, 64, 10, 5, 5), generator=g).cuda().contiguous(memory_format=cl)
    direct, three = _lib.conv3_split128_(x, rec, shift, 1), _lib.wino_conv3d_(x, U, shift, 1)
    assert not torch.equal(direct, three)                # the comparison below can tell the two forms apart
    assert plan._route(x, c) == "conv3_split128_"
    assert torch.equal(plan._conv3(x, c, 1), direct)
    xr = torch.randn((1, 64, 6, 5, 5), generator=g).cuda().contiguous(memory_format=cl)
    assert plan._route(xr, c) == "wino_conv3d_"
    assert torch.equal(plan._conv3(xr, c, 1), _lib.wino_conv3d_(xr, U, shift, 1))
    assert not torch.equal(_lib.wino_conv3d_(xr, U, shift, 1), _lib.conv3_split128_(xr, rec, shift, 1))
    # a record without the 24-byte form stays on the three launches
    assert torch.equal(plan._conv3(x, c._replace(direct24=None), 1), three)
    with pytest.raises(_lib.Sp3dError):
        _lib.conv3_split128_(x, rec[:, :4].contiguous(), shift, 1)
    with pytest.raises(TypeError):
        _lib.wino_conv3d_(x, U, shift, 1, direct=rec)


def test_switch_off_is_the_three_launch_form_bit_for_bit(monkeypatch):
    """SP3D_QUARTER_DIRECT=0 (read at every call): the plan's dispatch gives the bits of the three-launch entry"""
    from selfpose3d_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(5)
    cl = torch.channels_last_3d
    w = (torch.randn((128, 128, 3, 3, 3), generator=g) * 0.05).cuda()
    shift = torch.randn((128,), generator=g).cuda()
    x = torch.randn((2, 128, 10, 5, 5), generator=g).cuda().contiguous(memory_format=cl)
    res = torch.randn((2, 128, 10, 5, 5), generator=g).cuda().contiguous(memory_format=cl)
    plan = bare_plan()
    c = plan._conv3_record(w, shift)
    monkeypatch.setenv("SP3D_QUARTER_DIRECT", "0")
    for m in (1, 2):
        r = res if m >= 2 else None
        assert torch.equal(plan._conv3(x, c, m, r), _lib.wino_conv3d_(x, c.u, shift, m, r))
    monkeypatch.delenv("SP3D_QUARTER_DIRECT")
    assert not torch.equal(plan._conv3(x, c, 2, res), _lib.wino_conv3d_(x, c.u, shift, 2, res))
    assert torch.equal(plan._conv3(x, c, 2, res), _lib.conv3_split128_(x, c.direct24, shift, 2, res))


def test_plan_runs_the_six_quarter_layers_in_one_launch_each(monkeypatch):
    """a V2V net on 40x40x20 (quarter resolution 10x10x5: whole blocks): encoder_res2, mid_res and decoder_res2 reach the
    direct kernel, six launches; with the switch off none does, and the two fp32 forms of the net agree within the whole-net
    bound of tests/test_gpu_v2v_plan_f64.py (E2E_BOUND = 6.0e-6, as tests/test_gpu_skip_fold.py holds its two forms)"""
    from selfpose3d_amd import _lib
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
    x = torch.rand(1, 15, 40, 40, 20, generator=g).cuda()
    calls, real = [], _lib.conv3_split128_

    def spy(*a, **k):
        calls.append(tuple(a[0].shape))
        return real(*a, **k)
    monkeypatch.setattr(_lib, "conv3_split128_", spy)
    monkeypatch.delenv("SP3D_QUARTER_DIRECT", raising=False)
    with torch.no_grad():
        y1 = net(x).clone()
    assert calls == [(1, 64, 10, 10, 5)] + [(1, 128, 10, 10, 5)] * 5, calls
    monkeypatch.setenv("SP3D_QUARTER_DIRECT", "0")
    with torch.no_grad():
        y0 = net(x).clone()
    assert len(calls) == 6
    d = metric(y1.cpu(), y0.cpu().double())
    print("quarter_direct plan", d)
    assert 0.0 < d <= 6.0e-6
