"""The one-channel z-spectrum front (SP3D_HM_ONE_ZSPECTRUM, unproject_one_zd_kernel; ``SP3D_ONE_FRONT``, default off): one
heat-map channel read where it lies, the z-spectrum of its cubes out, and the ROOTNET_ROOTHM root nets fed by it.  The plan
and the refusals are pinned on the host by tests/test_one_front_host.py; this file holds the values:

1. bits: the spectrum equals the two-kernel HIP form (unproject_one_kernel's cubes as channel 0 of a channels-last tensor ->
   zdft_fwd_cl -> 4 x 4 tiles) bit for bit, those cubes are the oracle's, and the spectrum lies within 2e-6 x scale of numpy's
   float64 rfft of the oracle's cubes (the bound of tests/test_gpu_unproject_block_map.py::test_fused_zspectrum_vs_oracle_cubes
   and tests/test_gpu_wide_front.py for this transform);
2. coverage: every element of a NaN-filled spectrum is written, nothing around it is, a skipped sample is all zero;
3. sample_of: more cubes than samples through sp3d_unproject_fwd_indexed;
4. the opening conv fed by it against today's route on the same one-channel cubes, both against float64;
5. the root nets with the switch on against the switch off, both against the float64 net; proposals exactly equal;
6. GraphedRootNet replay with the switch on."""
import numpy as np
import pytest
import torch

from tests import front_sweep_cases as fs

pytestmark = pytest.mark.gpu

IMG, HM = (96, 72), (24, 18)                         # (w, h): heat-maps of 18 x 24 pixels
SZ, K = 28, 15
GUARD = 4096                                         # floats on either side of a guarded result
J, CHANNELS = 15, (2, 14)                            # channels of the 15-channel maps the sources point at
# max |rfft| of the oracle's cubes of the scenes below is their largest z-column sum (the DC bin): 12.9 .. 17.1 for the seeds
# committed here (scale_floor_report() prints them without a GPU); an empty scene has 0
SCALE_FLOOR = 12.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


_scenes = {}


def scene(B, V, cube, seed, valid=None, P=None):
    """15-channel heat-maps, camera table, centres (shifted per cube: the samples see different voxels) and the oracle's cubes
    of channels CHANNELS, computed once per key and left unchanged.  ``P``: cubes (> B) read through sample_of (p mod B); the
    oracle then runs on the gathered samples"""
    key = (B, V, tuple(cube), seed, None if valid is None else tuple(valid), P)
    if key not in _scenes:
        from oracle import oracle
        from selfpose3d_amd import synthetic as syn
        from selfpose3d_amd.camera_pack import pack_cameras
        n = B if P is None else P
        sample_of = np.arange(n, dtype=np.int32) % B
        meta = syn.make_meta(B, V, list(IMG))
        hms = syn.random_heatmaps(B, V, J, HM[1], HM[0], seed=seed)
        cam = pack_cameras(meta, B, list(IMG))
        centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), n, 0)
        centers[:, 0] += 250.0 * np.arange(n, dtype=np.float32)
        centers[:, 1] -= 130.0 * np.arange(n, dtype=np.float32)
        val = np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8)
        two = [np.ascontiguousarray(h.numpy()[sample_of][:, list(CHANNELS)]) for h in hms]
        cubes, _ = oracle.unproject_fwd(two, np.ascontiguousarray(cam[sample_of]), centers, val, syn.SPACE_SIZE, list(cube),
                                        list(IMG), want_grids=False)
        _scenes[key] = dict(hms=hms, cam=cam, centers=centers, valid=val, cubes={c: cubes[:, i:i + 1] for i, c in enumerate(CHANNELS)},
                            grid_size=syn.SPACE_SIZE, meta=meta, sample_of=sample_of)
    return _scenes[key]


BITS_CASES = [((12, 20, 20), 3, 1), ((12, 20, 20), 3, 2), ((12, 20, 20), 3, 4), ((12, 20, 20), 7, 1), ((12, 20, 20), 7, 2),
              ((12, 20, 20), 7, 4), ((80, 80, 20), 5, 4)]


def scale_floor_report():
    """max |rfft| of the oracle's cubes for every scene of test 1 (CPU only): what SCALE_FLOOR is taken from"""
    out = {}
    for cube, V, B in BITS_CASES:
        s = scene(B, V, cube, 700 + 10 * V + B)
        for ch in CHANNELS:
            out[cube, V, B, ch] = float(np.abs(np.fft.rfft(s["cubes"][ch].astype(np.float64), n=SZ, axis=4)).max())
    return out


def sources(s, dev):
    """[(name, ch, views)]: the channel as a slice of planar (B,15,h,w) tensors (channels 2 and 14), of a (V,B,h,w,16) and of
    a (V,B,h,w,32) buffer whose other channels hold noise (a tap at the wrong stride or channel cannot pass), and a contiguous
    (B,1,h,w) tensor"""
    hms = s["hms"]
    V = len(hms)
    B = hms[0].shape[0]
    d_h = [h.to(dev) for h in hms]
    out = [("planar2", 2, [x[:, 2:3] for x in d_h]), ("planar14", 14, [x[:, 14:15] for x in d_h])]
    rng = np.random.default_rng(5)
    for ps in (16, 32):
        buf = torch.from_numpy(rng.random((V, B, HM[1], HM[0], ps), dtype=np.float32) * 3.0 - 1.0)
        for c in range(V):
            buf[c, ..., :J] = hms[c].permute(0, 2, 3, 1)
        buf = buf.to(dev)
        out.append((f"nhwc{ps}", 2, [buf[c].permute(0, 3, 1, 2)[:, 2:3] for c in range(V)]))
    out.append(("contiguous", 2, [x[:, 2:3].contiguous() for x in d_h]))
    return out


def classify(views):
    from selfpose3d_amd.project_layer import one_channel_source
    one = one_channel_source(views)
    assert one is not None
    return one


def device_args(s, dev):
    return tuple(torch.from_numpy(s[a]).to(dev) for a in ("cam", "centers", "valid"))


def two_kernel_spectrum(views, layout, jp, args, P, cube, grid_size, sample_of=None):
    """the HIP form the fused launch replaces: unproject_one_kernel's planar cubes as channel 0 of a zeroed channels-last
    16-channel tensor through zdft_fwd_cl, tiled 4 x 4 -> (P, 1, 15, X/4, Y/4, 16), and the cubes"""
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    cubes, _ = _lib.unproject_fwd(views, layout, jp, *args, P, 1, HM[1], HM[0], cube, grid_size, IMG, False, one_channel=True,
                                  sample_of=sample_of)
    x = torch.zeros((P, X, Y, Z, 16), device=cubes.device)
    x[..., 0] = cubes[:, 0]
    return fs.tile44(_lib.zdft_fwd_cl(x.permute(0, 4, 1, 2, 3), 1, (X, Y, SZ))), cubes


# ---- 1. bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cube,V,B", BITS_CASES)
def test_spectrum_bits_and_oracle(dev, cube, V, B):
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    s = scene(B, V, cube, 700 + 10 * V + B)
    args = device_args(s, dev)
    f64 = {ch: np.fft.rfft(s["cubes"][ch].astype(np.float64), n=SZ, axis=4).transpose(0, 1, 4, 2, 3) for ch in CHANNELS}
    for name, ch, views in sources(s, dev):
        layout, jp = classify(views)
        spec = _lib.unproject_one_fwd_zspectrum(views, layout, jp, *args, B, HM[1], HM[0], cube, s["grid_size"], IMG, SZ)
        torch.cuda.synchronize(dev)
        assert tuple(spec.shape) == (B, 1, K, X // 4, Y // 4, 16) and spec.dtype == torch.complex64
        two, cubes = two_kernel_spectrum(views, layout, jp, args, B, cube, s["grid_size"])
        assert np.array_equal(cubes.cpu().numpy(), s["cubes"][ch]), (name, "the one-channel cubes are not the oracle's")
        assert torch.equal(torch.view_as_real(spec), torch.view_as_real(two)), (cube, V, B, name, float((spec - two).abs().max()))
        got = fs.untile44(spec, X, Y).cpu().numpy()
        scale = float(np.abs(f64[ch]).max())
        d64 = float(np.abs(got - f64[ch]).max())
        print("one-channel z-spectrum", cube, "V", V, "B", B, name, "d64 / scale %.3e" % (d64 / scale), "scale %.3f" % scale)
        assert scale > SCALE_FLOOR
        assert d64 <= 2e-6 * scale, (cube, V, B, name, d64, scale)


# ---- 2. coverage ------------------------------------------------------------------------------------------------------------
def test_every_element_written_and_nothing_else(dev):
    from selfpose3d_amd import _lib
    cube, B, V = (12, 20, 20), 3, 3
    X, Y, Z = cube
    s = scene(B, V, cube, 711, valid=(1, 0, 1))
    full = scene(B, V, cube, 711)                                                    # the same maps without the skip
    args, args_full = device_args(s, dev), device_args(full, dev)
    shape = (B, 1, K, X // 4, Y // 4, 16)
    n = 2 * int(np.prod(shape))
    for name, ch, views in sources(s, dev)[:3]:
        layout, jp = classify(views)
        buf = torch.full((n + 2 * GUARD + 32,), float("nan"), dtype=torch.float32, device=dev)
        off = GUARD + (-(buf.data_ptr() + 4 * GUARD) % 128) // 4                     # a 128-byte aligned interior
        out = torch.view_as_complex(buf[off:off + n].view(shape + (2,)))
        assert out.data_ptr() % 128 == 0
        spec = _lib.unproject_one_fwd_zspectrum(views, layout, jp, *args, B, HM[1], HM[0], cube, s["grid_size"], IMG, SZ, out=out)
        torch.cuda.synchronize(dev)
        assert spec.data_ptr() == out.data_ptr()
        real = torch.view_as_real(out)
        assert bool(torch.isfinite(real).all()), (name, "an element of the spectrum was not written")
        assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all()), (name, "a store outside the spectrum")
        assert int(torch.count_nonzero(real[1])) == 0, (name, "the skipped sample's planes are not exactly zero")
        whole = _lib.unproject_one_fwd_zspectrum(views, layout, jp, *args_full, B, HM[1], HM[0], cube, s["grid_size"], IMG, SZ)
        for b in (0, 2):
            assert float(real[b].abs().max()) > SCALE_FLOOR
            assert torch.equal(real[b], torch.view_as_real(whole)[b]), (name, b)
        assert float(torch.view_as_real(whole)[1].abs().max()) > SCALE_FLOOR
        two, _ = two_kernel_spectrum(views, layout, jp, args, B, cube, s["grid_size"])
        assert torch.equal(real, torch.view_as_real(two)), name


# ---- 3. sample_of -----------------------------------------------------------------------------------------------------------
def test_more_cubes_than_samples_through_sample_of(dev):
    from selfpose3d_amd import _lib
    cube, B, V, P = (12, 20, 20), 2, 3, 5
    X, Y, Z = cube
    s = scene(B, V, cube, 721, P=P)
    args = device_args(s, dev)
    so = torch.from_numpy(s["sample_of"]).to(dev)
    assert s["sample_of"].tolist() == [0, 1, 0, 1, 0]
    for name, ch, views in sources(s, dev):
        layout, jp = classify(views)
        if B > 1:
            assert (layout, jp) == {"planar2": (0, J), "planar14": (0, J), "nhwc16": (1, 16), "nhwc32": (1, 32), "contiguous": (0, 1)}[name]
        spec = _lib.unproject_one_fwd_zspectrum(views, layout, jp, *args, P, HM[1], HM[0], cube, s["grid_size"], IMG, SZ, sample_of=so)
        torch.cuda.synchronize(dev)
        assert tuple(spec.shape) == (P, 1, K, X // 4, Y // 4, 16)
        two, cubes = two_kernel_spectrum(views, layout, jp, args, P, cube, s["grid_size"], sample_of=so)
        assert np.array_equal(cubes.cpu().numpy(), s["cubes"][ch]), name
        assert torch.equal(torch.view_as_real(spec), torch.view_as_real(two)), name
        assert not torch.equal(spec[0], spec[2]) and float(spec.abs().max()) > SCALE_FLOOR      # the centres differ per cube


def test_refusals_with_real_tensors(dev):
    """the refusals of tests/test_one_front_host.py through the C entries on device buffers large enough for whatever a
    library that ignored the flag would launch: the refusal code, and not one word of the result buffers written"""
    import ctypes as C
    from selfpose3d_amd import _lib
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    lib = _lib.load()
    z, NHWC, PLANAR = _lib.HM_ONE_ZSPECTRUM, _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
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

    def both(layout, jp, cubes, g, Jc=1, hw=(h, w), cube=(8, 8, 20)):
        tail = (B, V, Jc, hw[0], hw[1], *cube, gs, 32, 32, None)
        a = f(views, layout, jp, *ptrs, cubes, g, *tail)
        b = fi(views, layout, jp, ptrs[0], so.data_ptr(), *ptrs[1:], cubes, g, *tail)
        assert a == b, (a, b)
        return a
    for layout, jp in ((PLANAR, 15), (NHWC, 16)):
        for other in (_lib.OUT_CHANNELS_LAST, _lib.HM_BF16, _lib.OUT_BF16, _lib.HM_ONE_CHANNEL, _lib.HM_WIDE_MASK, _lib.OUT_ZSPECTRUM):
            assert both(layout | z | other, jp, spec, None) == -4, hex(other)
        for Jc in (2, 4, 16):
            assert both(layout | z, jp, spec, None, Jc=Jc) == -4, Jc
        for Z in (16, 24, 32):
            assert both(layout | z, jp, spec, None, cube=(8, 8, Z)) == -4, Z
        for X, Y in ((6, 8), (8, 10), (7, 7)):
            assert both(layout | z, jp, spec, None, cube=(X, Y, 20)) == -4, (X, Y)
        for hw in ((1, 8), (8, 1)):
            assert both(layout | z, jp, spec, None, hw=hw) == -4, hw
        assert both(layout | z, jp, spec, grids) == -4
        for off in (4, 8, 16, 64):
            assert both(layout | z, jp, spec + off, None) == -4, off
        assert both(layout | z, 0, spec, None) == -1
        tail = (B, V, 1, h, w, 8, 8, 20, gs, 32, 32, None)
        st = (C.c_int64 * 4)(1280, 1280, 160, 20)
        assert lib.sp3d_unproject_fwd_strided(views, layout | z, jp, ptrs[0], None, *ptrs[1:], spec, st, *tail) == -4
        assert lib.sp3d_unproject_fwd_train(views, layout | z, jp, ptrs[0], None, *ptrs[1:], spec, None, mask, *tail) == -4
        assert lib.sp3d_unproject_one_fwd_train(views, layout | z, jp, ptrs[0], None, *ptrs[1:], spec, None, mask, *tail) == -4
    assert both(2 | z, 15, spec, None) == -1
    assert both(NHWC | _lib.HM_ONE_CHANNEL | _lib.OUT_ZSPECTRUM, 16, spec, None) == -4          # the older pair, as before
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(res).all()), "a refused call wrote to its result"
    # ... and the same request without anything wrong next to it runs
    assert both(NHWC | z, 16, spec, None) == 0
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(res[0, :2 * 15 * 2 * 2 * 16]).all()) and bool(torch.isnan(res[0, 2 * 15 * 2 * 2 * 16:]).all())


# ---- 4. the front -----------------------------------------------------------------------------------------------------------
def test_front_from_the_one_channel_spectrum_vs_todays_route(dev):
    """The opening conv of V2VNet(1, 1) (channels-last stack, random taps and BatchNorm: fs.front_net) on grid (76, 80, 20),
    B = 2, fed by the fused launch (_front_zspectrum), next to today's route on the same one-channel cubes (_front_fft: the
    library's 3-D real transforms), both against a float64 conv3d of the folded taps + shift + ReLU on the
    ORACLE's cubes.  Error = max |got - f64| / max |f64| over the batch.  Rule: e_new <= 1.5 x e_current.

    Measured (MI355X; also DESIGN.md §4.2a, "front errors"): e_new 2.714e-07, e_current 2.257e-07, range 3.775."""
    from selfpose3d_amd import _lib
    from selfpose3d_amd.v2v_net import TiledZSpectrum
    from tests.test_gpu_v2v_plan_f64 import conv3d_slabs          # float64 F.conv3d over x-slabs, as the front sweep's referee
    cube, B, V = (76, 80, 20), 2, 3
    s = scene(B, V, cube, 730)
    net = fs.front_net(1, True).to(dev)
    plan = net._get_plan()
    plan._ensure_built()
    w0, s0 = plan.layers["front"][:2]
    assert tuple(w0.shape) == (16, 1, 7, 7, 7)
    with torch.no_grad():
        ref = fs.ref_front(torch.from_numpy(s["cubes"][2]).to(dev), w0, s0, conv=lambda xd, wd: conv3d_slabs(xd, wd, None)).cpu()
    views = [h.to(dev)[:, 2:3] for h in s["hms"]]
    layout, jp = classify(views)
    args = device_args(s, dev)
    with torch.no_grad():
        net.one_front = True
        assert net.wants_zspectrum(*cube, 1) == SZ
        spec = _lib.unproject_one_fwd_zspectrum(views, layout, jp, *args, B, HM[1], HM[0], cube, s["grid_size"], IMG, SZ)
        new = plan._front_zspectrum(TiledZSpectrum(spec, *cube, SZ), w0, s0).clone()
        net.one_front = False
        assert net.wants_zspectrum(*cube, 1) is None
        cubes, _ = _lib.unproject_fwd(views, layout, jp, *args, B, 1, HM[1], HM[0], cube, s["grid_size"], IMG, False, one_channel=True)
        current = plan._front_fft(cubes, w0, s0).clone()
    torch.cuda.synchronize(dev)
    assert np.array_equal(cubes.cpu().numpy(), s["cubes"][2])
    assert tuple(new.shape) == tuple(current.shape) == tuple(ref.shape)
    rng = float(ref.abs().max())
    pos = float((ref > 0).double().mean())
    e_new = float((new.cpu().double() - ref).abs().max()) / rng
    e_cur = float((current.cpu().double() - ref).abs().max()) / rng
    print("one-channel front: e_new %.3e e_current %.3e range %.3f positive %.2f" % (e_new, e_cur, rng, pos))
    assert rng > 0.1 and 0.0 < pos < 1.0
    assert e_new <= 1.5 * e_cur, (e_new, e_cur)


# ---- 5. the root nets -------------------------------------------------------------------------------------------------------
def _switch(net, on):
    net.project_layer.one_zspectrum = net.v2v_net.one_front = bool(on)


_roots = {}


def _root_setup(dev):
    """CuboidProposalNet and CuboidProposalNetSoft (eval, channels-last, one state dict) from configs/cam5_posenet.yaml at the
    24 x 18 heat-map geometry, people heat-maps of 15 channels in both hand-overs, the oracle's root-channel cubes"""
    if "r" not in _roots:
        import os
        from oracle import oracle
        from selfpose3d_amd import _lib, synthetic as syn
        from selfpose3d_amd.camera_pack import pack_cameras
        from selfpose3d_amd.config import load_config
        from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
        from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
        from selfpose3d_amd.project_layer import nhwc_heatmap_views
        yaml = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cam5_posenet.yaml")
        cfg = load_config(yaml, NETWORK__IMAGE_SIZE=list(IMG), NETWORK__HEATMAP_SIZE=list(HM))
        assert bool(cfg.NETWORK.ROOTNET_ROOTHM) and [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE] == [80, 80, 20]
        B, V = 2, 5
        soft = CuboidProposalNetSoft(cfg)
        syn.fill_parameters_deterministic(soft, seed=5, scale=0.05)
        soft.to(dev).eval().use_channels_last(True)
        plain = CuboidProposalNet(cfg)
        plain.load_state_dict(soft.state_dict())
        plain.to(dev).eval().use_channels_last(True)
        assert plain.root_id == soft.root_id
        meta = syn.make_meta(B, V, list(IMG))
        cpu = syn.people_heatmaps(B, V, J, HM[1], HM[0], IMG, seed=41)[0]
        planar = [h.to(dev) for h in cpu]
        nhwc = nhwc_heatmap_views(_lib.pack_heatmaps(planar, jp=16), J)
        ch = int(plain.root_id)
        centers = np.repeat(np.asarray([cfg.MULTI_PERSON.SPACE_CENTER], np.float32), B, 0)
        cubes, _ = oracle.unproject_fwd([np.ascontiguousarray(h.numpy()[:, ch:ch + 1]) for h in cpu], pack_cameras(meta, B, list(IMG)),
                                        centers, np.ones(B, np.uint8), [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE], [80, 80, 20],
                                        list(IMG), want_grids=False)
        _roots["r"] = dict(cfg=cfg, plain=plain, soft=soft, meta=meta, planar=planar, nhwc=nhwc, cubes=cubes, B=B)
    return _roots["r"]


def _f64_root_cubes(dev, r):
    """the V2V net in float64 on the oracle's cubes, once"""
    if "f64" not in r:
        from tests.test_gpu_v2v_plan_f64 import Referee
        with torch.no_grad():
            r["f64"] = Referee(r["plain"].v2v_net).chain(torch.from_numpy(r["cubes"]).to(dev).double()).squeeze(1).cpu()
    return r["f64"]


class _Spy:
    """counts the calls of the fused entry and of everything the routes it replaces launch"""

    def __init__(self, monkeypatch):
        from selfpose3d_amd import _lib
        self.n = {"fused": 0, "unproject_fwd": 0, "pack_heatmaps": 0}
        for key, name in (("fused", "unproject_one_fwd_zspectrum"), ("unproject_fwd", "unproject_fwd"), ("pack_heatmaps", "pack_heatmaps")):
            inner = getattr(_lib, name)
            monkeypatch.setattr(_lib, name, (lambda inner, key: lambda *a, **k: (self.n.__setitem__(key, self.n[key] + 1), inner(*a, **k))[1])(inner, key))

    def reset(self):
        for k in self.n:
            self.n[k] = 0


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
@pytest.mark.parametrize("which", ["plain", "soft"])
def test_root_nets_switch_on_vs_off(dev, monkeypatch, which, hand_over):
    """Root cubes: both routes against the float64 net on the oracle's cubes, error = max |got - f64| / max |f64|; rule as in
    test 4, e_on <= 1.5 x e_off.  Proposals: exactly equal, on a scene where the oracle's top-k values (CPU) lie further apart
    than twice that bound, so that no tie decides.

    Measured (MI355X, all four cases): e_on 1.657e-06, e_off 2.025e-06, range 6.1685, max |on - off| / range 1.527e-06."""
    from oracle import oracle
    r = _root_setup(dev)
    net, meta, B = r[which], r["meta"], r["B"]
    hms = r[hand_over]
    run = (lambda: net(hms, meta)) if which == "plain" else (lambda: net.get_grid_centres(hms, meta))
    assert net.project_layer.one_zspectrum is False and net.v2v_net.one_front is False       # the default
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        off = [t.clone() for t in run()]
        assert spy.n["fused"] == 0 and spy.n["unproject_fwd"] == 1
        spy.reset()
        _switch(net, True)
        on = [t.clone() for t in run()]
        assert spy.n == {"fused": 1, "unproject_fwd": 0, "pack_heatmaps": 0}, spy.n        # one launch, no re-tiling pass
        spy.reset()
    # with grad enabled the switch changes nothing: the same tensors bit for bit
    g_on = [t.detach().clone() for t in run()]
    assert spy.n["fused"] == 0
    _switch(net, False)
    g_off = [t.detach().clone() for t in run()]
    assert torch.equal(g_on[0], g_off[0]) and torch.equal(g_on[1], g_off[1])
    with torch.no_grad():
        again = [t.clone() for t in run()]
    assert torch.equal(again[0], off[0]) and torch.equal(again[1], off[1])                   # the switch leaves nothing behind
    f64 = _f64_root_cubes(dev, r)
    rng = float(f64.abs().max())
    e_on = float((on[0].cpu().double() - f64).abs().max()) / rng
    e_off = float((off[0].cpu().double() - f64).abs().max()) / rng
    print("root net", which, hand_over, "e_on %.3e e_off %.3e range %.4f max |on - off| / range %.3e"
          % (e_on, e_off, rng, float((on[0] - off[0]).abs().max()) / rng))
    assert rng > 0.0
    assert e_on <= 1.5 * e_off, (e_on, e_off)
    # the proposals: no tie within the bound among the oracle's top-k (+ 1) values of the float64 cubes, then exact equality
    k = int(off[1].shape[1])
    vals, _ = oracle.nms_topk(f64.float().numpy(), k + 1)
    gaps = np.abs(np.diff(vals.astype(np.float64), axis=1))
    assert float(gaps.min()) > 2.0 * 1.5 * e_off * rng, (float(gaps.min()), e_off * rng)
    thr = float(r["cfg"].MULTI_PERSON.THRESHOLD)                      # ... nor a score within the bound of the flag's threshold
    assert float(np.abs(vals.astype(np.float64) - thr).min()) > 2.0 * 1.5 * e_off * rng
    assert torch.equal(on[1][..., :4], off[1][..., :4]), "proposal positions / flags differ"
    assert float((on[1][..., 4] - off[1][..., 4]).abs().max()) <= float((on[0] - off[0]).abs().max())


# ---- 6. the graph -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
def test_graphed_root_net_with_the_switch_on(dev, hand_over):
    from selfpose3d_amd import _lib, synthetic as syn
    from selfpose3d_amd.graphs import GraphedRootNet
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    r = _root_setup(dev)
    net, meta, B = r["plain"], r["meta"], r["B"]
    _switch(net, True)
    try:
        planar2 = [h.to(dev) for h in syn.people_heatmaps(B, 5, J, HM[1], HM[0], IMG, seed=42)[0]]
        hms2 = planar2 if hand_over == "planar" else nhwc_heatmap_views(_lib.pack_heatmaps(planar2, jp=16), J)
        with torch.no_grad():
            eager = [t.clone() for t in net(r[hand_over], meta)]
            eager2 = [t.clone() for t in net(hms2, meta)]
        assert not torch.equal(eager[0], eager2[0])
        if hand_over == "planar":
            static = [x.clone() for x in r["planar"]]
        else:
            static_buf = _lib.pack_heatmaps(r["planar"], jp=16)
            static = nhwc_heatmap_views(static_buf, J)
        g = GraphedRootNet(net, static, meta)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
        out = g()
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before, "a replay allocated device memory"
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
        if hand_over == "planar":                                       # new heat-maps through the same graph
            for dst, src in zip(static, planar2):
                dst.copy_(src)
        else:
            static_buf.copy_(_lib.pack_heatmaps(planar2, jp=16))
        out = g()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager2[0]) and torch.equal(out[1], eager2[1])
    finally:
        _switch(net, False)
