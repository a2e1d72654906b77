"""The z-spectrum result of the unprojection at 17..32 joints (SP3D_OUT_ZSPECTRUM at Jp = 32: one launch per channel group
into one spectrum) and the root net's opening conv fed by it (``SP3D_WIDE_FRONT``, default off).  The plan and the refusals are
pinned on the host by tests/test_wide_front_host.py; this file holds the values:

1. bits: the fused spectrum equals the two-kernel HIP form (planar cubes at Jp = 32 -> zdft_fwd_cl per channel group) bit for
   bit, and numpy's float64 rfft of the ORACLE's cubes within 2e-6 x scale (the bound of
   tests/test_gpu_unproject_block_map.py::test_fused_zspectrum_vs_oracle_cubes for this transform);
2. coverage: every element of a NaN-filled spectrum is written, nothing around it is, a skipped sample is all zero;
3. Jp = 16 with the flag is sp3d_unproject_fwd_zdft;
4. the opening conv fed by it against the library route on planar cubes, both against float64;
5. the root net with the switch on against the switch off;
6. GraphedRootNet replay with the switch on."""
import numpy as np
import pytest
import torch

from tests import front_sweep_cases as fs

pytestmark = pytest.mark.gpu

IMG, HM = (96, 72), (24, 18)                         # (w, h): heat-maps of 18 x 24 pixels
SZ, K = 28, 15
GUARD = 4096                                         # floats on either side of a guarded result


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


_scenes = {}


def scene(B, V, cube, seed, valid=None):
    """heat-maps of 32 channels (a test reads the first J), camera table, centres and the oracle's cubes for them, computed
    once per key and left unchanged"""
    key = (B, V, tuple(cube), seed, None if valid is None else tuple(valid))
    if key not in _scenes:
        from oracle import oracle
        from selfpose3d_amd import synthetic as syn
        from selfpose3d_amd.camera_pack import pack_cameras
        meta = syn.make_meta(B, V, list(IMG))
        hms = syn.random_heatmaps(B, V, 32, HM[1], HM[0], seed=seed)
        cam = pack_cameras(meta, B, list(IMG))
        centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), B, 0)
        centers[:, 0] += 250.0 * np.arange(B, dtype=np.float32)                   # the samples see different voxels
        val = np.ones(B, np.uint8) if valid is None else np.asarray(valid, np.uint8)
        cubes, _ = oracle.unproject_fwd([h.numpy() for h in hms], cam, centers, val, syn.SPACE_SIZE, list(cube), list(IMG),
                                        want_grids=False)
        _scenes[key] = dict(hms=hms, cam=cam, centers=centers, valid=val, cubes=cubes, grid_size=syn.SPACE_SIZE, meta=meta)
    return _scenes[key]


def device_args(s, J, jp, dev):
    from selfpose3d_amd import _lib
    packed = _lib.pack_heatmaps([h[:, :J].contiguous().to(dev) for h in s["hms"]], jp=jp)
    views = [packed[c] for c in range(len(s["hms"]))]
    return views, tuple(torch.from_numpy(s[a]).to(dev) for a in ("cam", "centers", "valid"))


def two_kernel_spectrum(views, args, B, J, cube, grid_size):
    """the HIP form the fused launches replace: planar cubes at jp = 32, channels 0-15 and 16..J-1 (zero-padded to 16) as
    channels-last tensors through zdft_fwd_cl, tiled 4 x 4 -> (B, J, 15, X/4, Y/4, 16), and the cubes"""
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    cubes, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, 32, *args, B, J, HM[1], HM[0], cube, grid_size, IMG, False)
    parts = []
    for lo, hi in ((0, 16), (16, J)):
        x = torch.zeros((B, X, Y, Z, 16), device=cubes.device)
        x[..., :hi - lo] = cubes[:, lo:hi].permute(0, 2, 3, 4, 1)
        parts.append(fs.tile44(_lib.zdft_fwd_cl(x.permute(0, 4, 1, 2, 3), hi - lo, (X, Y, SZ))))
    return torch.cat(parts, 1), cubes


# ---- 1. bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("cube,V", [((12, 20, 20), 3), ((80, 80, 20), 5)])
def test_spectrum_bits_and_oracle(dev, cube, V, B):
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    s = scene(B, V, cube, 900 + B)
    for J in (17, 21, 29, 32):
        views, args = device_args(s, J, 32, dev)
        spec = _lib.unproject_fwd_zspectrum(views, 32, *args, B, J, HM[1], HM[0], cube, s["grid_size"], IMG, SZ)
        torch.cuda.synchronize(dev)
        assert tuple(spec.shape) == (B, J, K, X // 4, Y // 4, 16) and spec.dtype == torch.complex64
        two, cubes = two_kernel_spectrum(views, args, B, J, cube, s["grid_size"])
        assert np.array_equal(cubes.cpu().numpy(), s["cubes"][:, :J]), (J, "the planar cubes are not the oracle's")
        assert torch.equal(torch.view_as_real(spec), torch.view_as_real(two)), \
            (cube, B, J, float((spec - two).abs().max()))
        f64 = np.fft.rfft(s["cubes"][:, :J].astype(np.float64), n=SZ, axis=4).transpose(0, 1, 4, 2, 3)
        got = fs.untile44(spec, X, Y).cpu().numpy()
        scale = float(np.abs(f64).max())
        d64 = float(np.abs(got - f64).max())
        print("wide z-spectrum", cube, "B", B, "J", J, "d64 / scale %.3e" % (d64 / scale), "scale %.3f" % scale)
        assert scale > 10.0
        assert d64 <= 2e-6 * scale, (cube, B, J, d64, scale)


# ---- 2. coverage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [17, 21, 32])
def test_every_element_written_and_nothing_else(dev, J):
    from selfpose3d_amd import _lib
    cube, B, V = (12, 20, 20), 3, 3
    X, Y, Z = cube
    s = scene(B, V, cube, 911, valid=(1, 0, 1))
    views, args = device_args(s, J, 32, dev)
    shape = (B, J, K, X // 4, Y // 4, 16)
    n = 2 * int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 32,), float("nan"), dtype=torch.float32, device=dev)
    off = GUARD + (-(buf.data_ptr() + 4 * GUARD) % 128) // 4                         # a 128-byte aligned interior
    out = torch.view_as_complex(buf[off:off + n].view(shape + (2,)))
    assert out.data_ptr() % 128 == 0
    spec = _lib.unproject_fwd_zspectrum(views, 32, *args, B, J, HM[1], HM[0], cube, s["grid_size"], IMG, SZ, out=out)
    torch.cuda.synchronize(dev)
    assert spec.data_ptr() == out.data_ptr()
    assert bool(torch.isfinite(torch.view_as_real(out)).all()), "an element of the spectrum was not written"
    assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all()), "a store outside the spectrum"
    real = torch.view_as_real(out)
    assert int(torch.count_nonzero(real[1])) == 0, "the skipped sample's planes are not exactly zero"
    assert int(torch.count_nonzero(real[1, :16])) == 0 and int(torch.count_nonzero(real[1, 16:])) == 0    # both groups
    for b in (0, 2):
        assert float(real[b, :16].abs().max()) > 1.0 and float(real[b, 16:].abs().max()) > 1.0
        assert all(float(real[b, c].abs().max()) > 0.0 for c in range(J)), "a channel plane is empty"
    two, _ = two_kernel_spectrum(views, args, B, J, cube, s["grid_size"])
    assert torch.equal(real, torch.view_as_real(two))


# ---- 3. Jp = 16 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cube,B", [((12, 20, 20), 2), ((80, 80, 20), 1)])
def test_jp16_with_the_flag_is_the_zdft_entry(dev, cube, B):
    from selfpose3d_amd import _lib
    J = 15
    s = scene(B, 3, cube, 920 + B)
    views, args = device_args(s, J, 16, dev)
    tail = (B, J, HM[1], HM[0], cube, s["grid_size"], IMG, SZ)
    a = _lib.unproject_fwd_zspectrum(views, 16, *args, *tail)
    b = _lib.unproject_fwd_zdft(views, 16, *args, *tail)
    torch.cuda.synchronize(dev)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    assert float(a.abs().max()) > 10.0


def test_refusals_with_real_tensors(dev):
    """the refusals of tests/test_wide_front_host.py through the C entries on device buffers large enough for whatever a
    library that ignored the flag would launch: SP3D_EUNSUPPORTED (-4), and not one word of the result buffers written"""
    import ctypes as C
    from selfpose3d_amd import _lib
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    lib = _lib.load()
    z, NHWC, PLANAR = _lib.OUT_ZSPECTRUM, _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
    B, V, h, w = 1, 2, 8, 8
    cam = torch.from_numpy(pack_cameras(syn.make_meta(B, V, [32, 32]), B, [32, 32])).to(dev)
    maps = torch.rand((V, 1 << 16), device=dev)                       # each view: room for any (h, w, Jp) read below
    views = (C.c_void_p * V)(*[maps[c].data_ptr() for c in range(V)])
    centers = torch.tensor([syn.SPACE_CENTER], dtype=torch.float32, device=dev)
    valid, so = torch.ones(1, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    res = torch.full((3, 1 << 21), float("nan"), device=dev)         # spectrum / cubes, grids, pass mask
    spec, grids, mask = (res[i].data_ptr() for i in range(3))
    assert spec % 128 == 0
    gs = (C.c_float * 3)(*[float(v) for v in syn.SPACE_SIZE])
    f, fi = lib.sp3d_unproject_fwd, lib.sp3d_unproject_fwd_indexed
    ptrs = (cam.data_ptr(), centers.data_ptr(), valid.data_ptr())

    def both(layout, jp, cubes, g, J=17, hw=(h, w), cube=(8, 8, 20)):
        tail = (B, V, J, hw[0], hw[1], *cube, gs, 32, 32, None)
        a = f(views, layout, jp, *ptrs, cubes, g, *tail)
        b = fi(views, layout, jp, ptrs[0], so.data_ptr(), *ptrs[1:], cubes, g, *tail)
        assert a == b, (a, b)
        return a
    for other in (_lib.OUT_CHANNELS_LAST, _lib.HM_BF16, _lib.OUT_BF16, _lib.HM_ONE_CHANNEL, _lib.HM_WIDE_MASK):
        assert both(NHWC | z | other, 32, spec, None) == -4, hex(other)
        assert both(NHWC | z | other, 16, spec, None, J=16) == -4, hex(other)
    assert both(PLANAR | z, 17, spec, None) == -4
    for jp in (4, 8, 12, 20, 36):
        assert both(NHWC | z, jp, spec, None, J=min(jp, 17)) == -4, jp
    assert both(NHWC | z, 32, spec, None, J=33) == -4 and both(NHWC | z, 16, spec, None, J=17) == -4
    for Z in (16, 24, 32):
        assert both(NHWC | z, 32, spec, None, cube=(8, 8, Z)) == -4, Z
    for X, Y in ((6, 8), (8, 10), (7, 7)):
        assert both(NHWC | z, 32, spec, None, cube=(X, Y, 20)) == -4, (X, Y)
    for hw in ((1, 8), (8, 1)):
        assert both(NHWC | z, 32, spec, None, hw=hw) == -4, hw
    for jp, J in ((32, 17), (16, 15)):
        tail = (B, V, J, h, w, 8, 8, 20, gs, 32, 32, None)
        assert both(NHWC | z, jp, spec, grids, J=J) == -4
        for off in (4, 8, 16, 64):
            assert both(NHWC | z, jp, spec + off, None, J=J) == -4, off
        st = (C.c_int64 * 4)(J * 1280, 1280, 160, 20)
        assert lib.sp3d_unproject_fwd_strided(views, NHWC | z, jp, ptrs[0], None, *ptrs[1:], spec, st, *tail) == -4
        assert lib.sp3d_unproject_fwd_train(views, NHWC | z, jp, ptrs[0], None, *ptrs[1:], spec, None, mask, *tail) == -4
    assert lib.sp3d_unproject_one_fwd_train(views, PLANAR | z, 5, ptrs[0], None, *ptrs[1:], spec, None, mask, B, V, 1, h, w, 8, 8, 20,
                                            gs, 32, 32, None) == -4
    assert lib.sp3d_unproject_fwd_zdft(views, 32, *ptrs, spec, B, V, 17, h, w, 8, 8, 20, gs, 32, 32, 28, None) == -4
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(res).all()), "a refused call wrote to its result"
    # ... and the same request without anything wrong next to it runs
    assert both(NHWC | z, 32, spec, None) == 0
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(res[0, :2 * 17 * 15 * 2 * 2 * 16]).all())


# ---- 4. the front -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [17, 32])
def test_front_from_the_wide_spectrum_vs_library_route(dev, cin):
    """The opening conv of V2VNet(cin, 1) (channels-last stack) on grid (76, 80, 20), B = 2, fed by the two fused launches
    (_front_zspectrum), next to the library route on the planar cubes of the same maps (_front_fft, switch off), both against
    a float64 conv3d of the folded taps + shift + ReLU on the ORACLE's cubes; error per sample as in
    tests/front_sweep_cases.py, max|got - f64| / max(1, max|f64|).  Rule: e_wide <= 1.5 * e_generic + 1e-7 (F_HAND) with
    e_generic <= LIB_CAP.  The sweep's convention is "sample 1 is 1e3 x sample 0"; the unprojection clamps its cubes to
    [0, 1], so the ratio is made downwards: sample 1 has U[0, 1) heat-maps, sample 0 the same kind times 1e-3.

    Measured (MI355X, per sample (0, 1); also profiles/r20_coco17_wide_front.json, "front_errors"):
        cin   e_wide                    e_generic                 allowed for e_wide
        17    4.136e-08, 3.814e-07      4.147e-08, 3.058e-07      1.622e-07, 5.587e-07
        32    3.381e-08, 2.694e-07      3.382e-08, 2.331e-07      1.507e-07, 4.497e-07"""
    from selfpose3d_amd import _lib
    from selfpose3d_amd.v2v_net import TiledZSpectrum
    from oracle import oracle
    cube, B, V = (76, 80, 20), 2, 3
    s = scene(B, V, cube, 930)
    hms = [h[:, :cin] * torch.tensor([1e-3, 1.0]).view(2, 1, 1, 1) for h in s["hms"]]
    ref_cubes, _ = oracle.unproject_fwd([h.numpy() for h in hms], s["cam"], s["centers"], s["valid"], s["grid_size"], list(cube),
                                        list(IMG), want_grids=False)
    assert 500.0 < float(ref_cubes[1].max()) / float(ref_cubes[0].max()) < 2000.0
    net = fs.front_net(cin, True).to(dev)
    plan = net._get_plan()
    plan._ensure_built()
    w0, s0 = plan.layers["front"][:2]
    from tests.test_gpu_v2v_plan_f64 import conv3d_slabs          # float64 F.conv3d over x-slabs, as the front sweep's referee
    ref = fs.ref_front(torch.from_numpy(ref_cubes).to(dev), w0, s0, conv=lambda xd, wd: conv3d_slabs(xd, wd, None)).cpu()
    packed = _lib.pack_heatmaps([h.contiguous().to(dev) for h in hms], jp=32)
    views = [packed[c] for c in range(V)]
    args = tuple(torch.from_numpy(s[a]).to(dev) for a in ("cam", "centers", "valid"))
    with torch.no_grad():
        net.wide_front = True
        assert net.wants_zspectrum(*cube, cin) == SZ
        spec = _lib.unproject_fwd_zspectrum(views, 32, *args, B, cin, HM[1], HM[0], cube, s["grid_size"], IMG, SZ)
        wide = plan._front_zspectrum(TiledZSpectrum(spec, *cube, SZ), w0, s0).clone()
        net.wide_front = False
        assert net.wants_zspectrum(*cube, cin) is None
        planar, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, 32, *args, B, cin, HM[1], HM[0], cube, s["grid_size"], IMG, False)
        generic = plan._front_fft(planar, w0, s0).clone()
    torch.cuda.synchronize(dev)
    assert tuple(wide.shape) == tuple(generic.shape) == tuple(ref.shape)
    e_wide, e_gen = fs.compare(wide.cpu(), ref), fs.compare(generic.cpu(), ref)
    print("wide front cin", cin, "e_wide", ["%.3e" % e for e in e_wide["err"]], "e_generic", ["%.3e" % e for e in e_gen["err"]],
          "range", ["%.3f" % r for r in e_wide["range"]], "pos", ["%.2f" % p for p in e_wide["pos"]])
    assert all(0.0 < p < 1.0 for p in e_wide["pos"]), e_wide["pos"]
    assert all(e <= fs.LIB_CAP for e in e_gen["err"]), (e_gen["err"], fs.LIB_CAP)
    assert fs.within(fs.F_HAND, e_wide["err"], e_gen["err"]), (e_wide["err"], e_gen["err"])


# ---- 5. the root net --------------------------------------------------------------------------------------------------------
def _switch(root, on):
    root.project_layer.wide_zspectrum = root.v2v_net.wide_front = bool(on)


def test_root_net_with_the_switch_on(dev, monkeypatch):
    from selfpose3d_amd import _lib
    from tests.test_gpu_coco17 import _nets, _people_heatmaps, wide_calls
    B = 4
    cfg, root, _ = _nets(dev)
    root.use_channels_last(True)
    assert root.project_layer.wide_zspectrum is False and root.v2v_net.wide_front is False     # the default
    hms, meta = _people_heatmaps(cfg, B, seed=11)
    hms = [h.to(dev) for h in hms]
    calls = wide_calls(monkeypatch)
    fused = []
    real = _lib.unproject_fwd_zspectrum
    monkeypatch.setattr(_lib, "unproject_fwd_zspectrum", lambda views, jp, *a, **k: (fused.append(jp), real(views, jp, *a, **k))[1])
    with torch.no_grad():
        off = root(hms, meta)[0].clone()
        assert calls == [(_lib.LAYOUT_NHWC, 32)] and fused == []
        calls.clear()
        _switch(root, True)
        on = root(hms, meta)[0].clone()
        assert calls == [] and fused == [32], (calls, fused)
        _switch(root, False)
        again = root(hms, meta)[0].clone()
    assert torch.equal(again, off)                                   # the switch leaves nothing behind
    d, scale = float((on - off).abs().max()), max(1.0, float(off.abs().max()))
    print("root net, switch on vs off: max diff %.3e, scale %.3f" % (d, scale))
    assert float(off.abs().max()) > 0.0
    assert d <= 1e-4 * scale, (d, scale)


# ---- 6. the graph -----------------------------------------------------------------------------------------------------------
def test_graphed_root_net_with_the_switch_on(dev):
    from selfpose3d_amd.graphs import GraphedRootNet
    from tests.test_gpu_coco17 import _nets, _people_heatmaps
    B = 4
    cfg, root, _ = _nets(dev)
    root.use_channels_last(True)
    _switch(root, True)
    hms, meta = _people_heatmaps(cfg, B, seed=12)
    static = [h.to(dev).contiguous() for h in hms]
    with torch.no_grad():
        eager_cubes, eager_centers = (t.clone() for t in root(static, meta))
    g = GraphedRootNet(root, static, meta)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    out_cubes, out_centers = g()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before, "a replay allocated device memory"
    assert torch.equal(out_cubes, eager_cubes) and torch.equal(out_centers, eager_centers)
    hms2, _ = _people_heatmaps(cfg, B, seed=13)                       # new heat-maps through the same graph
    for st, h in zip(g.static_hms, hms2):
        st.copy_(h.to(dev))
    out_cubes, out_centers = g()
    torch.cuda.synchronize()
    with torch.no_grad():
        out_cubes, out_centers = out_cubes.clone(), out_centers.clone()
        e2, c2 = root([h.to(dev) for h in hms2], meta)
    assert torch.equal(out_cubes, e2) and torch.equal(out_centers, c2)
