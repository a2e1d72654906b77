"""One heat-map channel unprojected where it lies (SP3D_HM_ONE_CHANNEL, unproject_one_kernel) against the CPU oracle.

The reference is always the oracle on a CONTIGUOUS copy of the channel, compared with np.array_equal over every voxel:
through the C ABI on a sweep of shapes (planar slice; channels-last slice at the pixel stride jp_for(Jt) and at an odd one;
dense, padded, channels-last and strided results; a sample_of permutation), at full size with poisoned destinations, through
ProjectLayer (switch on vs off, no re-tiling pass, gradient path unchanged) and through the ROOTNET_ROOTHM root nets."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_v2v_plan_f64 import poison_free_blocks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _cases():
    rng = np.random.default_rng(2025)
    out = [  # (B, V, Jt, ch, (w,h) heat-map, cube)
        (1, 1, 1, 0, (2, 2), (1, 1, 1)), (2, 16, 15, 2, (9, 7), (5, 3, 7)), (3, 2, 16, 15, (33, 17), (6, 6, 6)),
        (2, 5, 15, 2, (96, 72), (17, 13, 9)), (1, 10, 4, 3, (48, 36), (32, 32, 8)), (4, 4, 13, 12, (24, 18), (16, 4, 4)),
        (2, 7, 32, 16, (5, 64), (4, 4, 33)), (4, 5, 15, 2, (240, 128), (20, 20, 20)),
    ]
    for _ in range(12):
        Jt = int(rng.integers(1, 33))
        out.append((int(rng.integers(1, 5)), int(rng.integers(1, 17)), Jt, int(rng.integers(0, Jt)),
                    (int(rng.integers(2, 80)), int(rng.integers(2, 60))),
                    (int(rng.integers(1, 20)), int(rng.integers(1, 20)), int(rng.integers(1, 24)))))
    return out


def _inputs(idx, case):
    """rigs, flips, centres and `valid` as tests/test_gpu_random_sweep.py generates them"""
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    B, V, Jt, ch, (w, h), cube = case
    rng = np.random.default_rng(1000 + idx)
    img = (w * 4, h * 4)
    meta = syn.random_meta(B, V, img, seed=idx, augment=(idx % 2 == 0), ssv_style=(idx % 3 == 0))
    flip = torch.from_numpy(rng.random(B) < 0.4) if idx % 2 == 0 else None
    cam = pack_cameras(meta, B, img, flip)
    hms = [torch.from_numpy((rng.random((B, Jt, h, w), dtype=np.float32) * 1.6 - 0.3)) for _ in range(V)]
    if idx % 2 == 1:
        centers = np.stack([rng.uniform(-2500, 2500, B), rng.uniform(-3000, 2000, B), rng.uniform(0, 1800, B)], 1).astype(np.float32)
        gs = [float(rng.uniform(500, 3000))] * 3
    else:
        centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), B, 0)
        gs = list(syn.SPACE_SIZE)
    valid = (rng.random(B) < 0.8).astype(np.uint8)
    valid[0] = 1
    return img, cam, hms, centers, gs, valid, rng


def _channel(hms, ch):
    return [np.ascontiguousarray(x.numpy()[:, ch:ch + 1]) for x in hms]


def _hand_overs(dev, hms, ch, strides, rng):
    """[(name, layout, jp, views)]: the channel as a slice of the planar tensors and of channels-last buffers whose other
    channels hold noise (a tap at the wrong stride or channel cannot pass)"""
    from selfpose3d_amd import _lib
    V = len(hms)
    B, Jt, h, w = hms[0].shape
    d_h = [x.to(dev) for x in hms]
    out = [("planar", _lib.LAYOUT_PLANAR, Jt, [x[:, ch:ch + 1] for x in d_h])]
    for ps in strides:
        assert ps > ch
        buf = torch.from_numpy(rng.random((V, B, h, w, ps), dtype=np.float32) * 3.0 - 1.0)
        for c in range(V):
            buf[c, ..., ch] = hms[c][:, ch]
        buf = buf.to(dev)
        out.append((f"nhwc{ps}", _lib.LAYOUT_NHWC, ps, [buf[c].permute(0, 3, 1, 2)[:, ch:ch + 1] for c in range(V)]))
    return out


def _check_all_results(dev, name, views, layout, jp, cam, centers, valid, P, h, w, cube, gs, img, ref_c, ref_g, sample_of=None):
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    camd, cen, val = torch.from_numpy(cam).to(dev), torch.from_numpy(centers).to(dev), torch.from_numpy(valid).to(dev)
    so = None if sample_of is None else torch.from_numpy(sample_of.astype(np.int32)).to(dev)
    kw = dict(sample_of=so, one_channel=True)
    # dense J = 1 + grids
    got, grids = _lib.unproject_fwd(views, layout, jp, camd, cen, val, P, 1, h, w, cube, gs, img, True, **kw)
    assert np.array_equal(grids.cpu().numpy(), ref_g), name
    g = got.cpu().numpy()
    assert g.shape == ref_c.shape and np.array_equal(g, ref_c), (name, "dense1", float(np.nanmax(np.abs(g - ref_c))))
    # dense J = 4: the value and three zero channels
    got, none = _lib.unproject_fwd(views, layout, jp, camd, cen, val, P, 4, h, w, cube, gs, img, False, **kw)
    g = got.cpu().numpy()
    assert none is None and g.shape == (P, 4, X, Y, Z)
    assert np.array_equal(g[:, :1], ref_c), (name, "dense4", float(np.nanmax(np.abs(g[:, :1] - ref_c))))
    assert np.array_equal(g[:, 1:], np.zeros_like(g[:, 1:])), (name, "dense4 pad")
    # channels-last J = 4
    got, _ = _lib.unproject_fwd(views, layout, jp, camd, cen, val, P, 4, h, w, cube, gs, img, False, channels_last=True, **kw)
    assert tuple(got.permute(0, 2, 3, 4, 1).stride()) == tuple(torch.empty(P, X, Y, Z, 4).stride())
    g = got.cpu().numpy()
    assert np.array_equal(g[:, :1], ref_c), (name, "cl4", float(np.nanmax(np.abs(g[:, :1] - ref_c))))
    assert np.array_equal(g[:, 1:], np.zeros_like(g[:, 1:])), (name, "cl4 pad")
    # strided J = 1 into a NaN-prefilled padded buffer: the padding stays NaN
    buf = torch.full((P + 1, 2, X + 2, Y + 1, Z + 3), float("nan"), device=dev)
    view = buf[:P, 1:2, 1:X + 1, :Y, 2:Z + 2]
    _lib.unproject_fwd(views, layout, jp, camd, cen, val, P, 1, h, w, cube, gs, img, False, out=view, **kw)
    g = view.cpu().numpy()
    assert np.array_equal(g, ref_c), (name, "strided", float(np.nanmax(np.abs(g - ref_c))), int(np.isnan(g).sum()))
    rest = buf.clone()
    rest[:P, 1:2, 1:X + 1, :Y, 2:Z + 2] = float("nan")
    assert bool(torch.isnan(rest).all()), (name, "the kernel wrote outside its view of the padded buffer")


@pytest.mark.parametrize("idx,case", list(enumerate(_cases())))
def test_cabi_sweep_bit_exact(dev, idx, case):
    from oracle import oracle
    from selfpose3d_amd.project_layer import ProjectLayer
    B, V, Jt, ch, (w, h), cube = case
    img, cam, hms, centers, gs, valid, rng = _inputs(idx, case)
    ref_c, ref_g = oracle.unproject_fwd(_channel(hms, ch), cam, centers, valid, gs, cube, img)
    odd = Jt + 1 if (Jt + 1) % 2 else Jt + 2
    overs = _hand_overs(dev, hms, ch, (ProjectLayer.jp_for(Jt), odd), rng)
    for name, layout, jp, views in overs:
        _check_all_results(dev, name, views, layout, jp, cam, centers, valid, B, h, w, cube, gs, img, ref_c, ref_g)
    # one pass with a sample_of permutation: cube p reads sample sample_of[p], with its own centre and valid flag
    sample_of = rng.permutation(B)
    cen_p = np.stack([rng.uniform(-2000, 2000, B), rng.uniform(-2500, 1500, B), rng.uniform(200, 1600, B)], 1).astype(np.float32)
    val_p = valid[::-1].copy()
    ref_c, ref_g = oracle.unproject_fwd([x[sample_of] for x in _channel(hms, ch)], cam[sample_of], cen_p, val_p, gs, cube, img)
    for name, layout, jp, views in overs:
        _check_all_results(dev, name + "/sample_of", views, layout, jp, cam, cen_p, val_p, B, h, w, cube, gs, img, ref_c, ref_g,
                           sample_of=sample_of)


def test_sweep_covers_clamps_skips_and_zeros():
    """what the sweep exercises, measured on the oracle: values clamped at 0 and at 1, a skipped sample, exact zeros"""
    from oracle import oracle
    lo = hi = skipped = False
    zero_share = []
    for idx, case in enumerate(_cases()):
        if int(np.prod(case[5])) * case[0] > 40000:
            continue
        img, cam, hms, centers, gs, valid, _ = _inputs(idx, case)
        c, _ = oracle.unproject_fwd(_channel(hms, case[3]), cam, centers, valid, gs, case[5], img)
        lo, hi, skipped = lo or bool((c == 0).any()), hi or bool((c == 1).any()), skipped or not valid.all()
        zero_share.append(float((c == 0).mean()))
    assert lo and hi and skipped, (lo, hi, skipped)
    assert min(zero_share) < 0.01 and sum(z > 0.3 for z in zero_share) >= 3, zero_share      # from none to many exact zeros


IMG, HM, V = (960, 512), (240, 128), 5


def _scene(B, seed, centers=None):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    meta = syn.make_meta(B, V, list(IMG))
    hms = syn.random_heatmaps(B, V, 15, HM[1], HM[0], seed=seed)
    cam = pack_cameras(meta, B, list(IMG))
    if centers is None:
        centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), B, 0)
    return meta, hms, cam, centers


def _full_size_hand_overs(dev, hms, ch):
    from selfpose3d_amd import _lib
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    d_h = [x.to(dev) for x in hms]
    packed = _lib.pack_heatmaps(d_h, jp=16)
    return [("planar", _lib.LAYOUT_PLANAR, 15, [x[:, ch:ch + 1] for x in d_h]),
            ("nhwc", _lib.LAYOUT_NHWC, 16, [v[:, ch:ch + 1] for v in nhwc_heatmap_views(packed, 15)])]


@pytest.mark.parametrize("B", [1, 2, 4])
def test_root_grid_full_size_poisoned(dev, B):
    """80 x 80 x 20, 5 x 240 x 128, channel 2 of 15: fresh results land in NaN-filled allocator blocks, `out=` in a NaN buffer"""
    from oracle import oracle
    from selfpose3d_amd import _lib, synthetic as syn
    cube, ch = (80, 80, 20), 2
    meta, hms, cam, centers = _scene(B, 900 + B)
    valid = np.ones(B, np.uint8)
    want, want_g = oracle.unproject_fwd(_channel(hms, ch), cam, centers, valid, syn.SPACE_SIZE, cube, list(IMG))
    assert float(want.max()) > 0.5
    args = (torch.from_numpy(cam).to(dev), torch.from_numpy(centers).to(dev), torch.from_numpy(valid).to(dev))
    for name, layout, jp, views in _full_size_hand_overs(dev, hms, ch):
        poison_free_blocks(dev)
        c1, g1 = _lib.unproject_fwd(views, layout, jp, *args, B, 1, HM[1], HM[0], cube, syn.SPACE_SIZE, IMG, True, one_channel=True)
        c4, _ = _lib.unproject_fwd(views, layout, jp, *args, B, 4, HM[1], HM[0], cube, syn.SPACE_SIZE, IMG, False, one_channel=True)
        cl, _ = _lib.unproject_fwd(views, layout, jp, *args, B, 4, HM[1], HM[0], cube, syn.SPACE_SIZE, IMG, False,
                                   channels_last=True, one_channel=True)
        out = torch.full((B, 1, 88, 88, 28), float("nan"), device=dev)[:, :, :80, :80, :20]
        _lib.unproject_fwd(views, layout, jp, *args, B, 1, HM[1], HM[0], cube, syn.SPACE_SIZE, IMG, False, out=out, one_channel=True)
        torch.cuda.synchronize(dev)
        assert np.array_equal(g1.cpu().numpy(), want_g), name
        for tag, got in (("dense1", c1), ("dense4", c4), ("cl4", cl), ("out", out)):
            g = got.cpu().numpy()
            assert np.array_equal(g[:, :1], want), (name, tag, B, float(np.nanmax(np.abs(g[:, :1] - want))), int(np.isnan(g).sum()))
            assert not np.any(g[:, 1:]), (name, tag)


def test_person_cubes_full_size_through_sample_of(dev):
    """eight 64^3 cubes read from two samples through sample_of, one of them skipped"""
    from oracle import oracle
    from selfpose3d_amd import _lib
    cube, gs, ch, B, P = (64, 64, 64), [2000.0, 2000.0, 2000.0], 2, 2, 8
    meta, hms, cam, _ = _scene(B, 930)
    rng = np.random.default_rng(8)
    sample_of = np.array([p % B for p in range(P)][::-1], np.int64)
    centers = np.stack([rng.uniform(-1500, 1500, P), rng.uniform(-1500, 1500, P), rng.uniform(700, 1100, P)], 1).astype(np.float32)
    valid = np.ones(P, np.uint8)
    valid[3] = 0
    want, _ = oracle.unproject_fwd([x[sample_of] for x in _channel(hms, ch)], cam[sample_of], centers, valid, gs, cube, list(IMG),
                                   want_grids=False)
    assert not np.any(want[3]) and float(want.max()) > 0.5
    so = torch.from_numpy(sample_of.astype(np.int32)).to(dev)
    args = (torch.from_numpy(cam).to(dev), torch.from_numpy(centers).to(dev), torch.from_numpy(valid).to(dev))
    for name, layout, jp, views in _full_size_hand_overs(dev, hms, ch):
        poison_free_blocks(dev)
        cl, _ = _lib.unproject_fwd(views, layout, jp, *args, P, 4, HM[1], HM[0], cube, gs, IMG, False, channels_last=True,
                                   sample_of=so, one_channel=True)
        buf = torch.full((P, 1, 72, 72, 72), float("nan"), device=dev)
        out = buf[:, :, :64, :64, :64]
        _lib.unproject_fwd(views, layout, jp, *args, P, 1, HM[1], HM[0], cube, gs, IMG, False, sample_of=so, out=out, one_channel=True)
        torch.cuda.synchronize(dev)
        g = cl.cpu().numpy()
        assert np.array_equal(g[:, :1], want) and not np.any(g[:, 1:]), (name, float(np.nanmax(np.abs(g[:, :1] - want))))
        assert np.array_equal(out.cpu().numpy(), want), name
        buf[:, :, :64, :64, :64] = float("nan")
        assert bool(torch.isnan(buf).all()), name


def test_cabi_refusals_with_real_tensors(dev):
    """the refusals of tests/test_one_channel_host.py with device buffers large enough that a library which misses one
    (and launches) reads and writes in bounds"""
    from selfpose3d_amd import _lib
    lib = _lib.load()
    one = _lib.HM_ONE_CHANNEL
    hm = torch.zeros(2, 32, 8, 8, device=dev)
    cam = torch.zeros(2, 2, 64, device=dev)
    cen, val = torch.zeros(2, 3, device=dev), torch.ones(2, dtype=torch.uint8, device=dev)
    cubes, grids = torch.zeros(2, 16, 4, 4, 4, device=dev), torch.zeros(2, 64, 3, device=dev)
    mask = torch.zeros(2, 64, dtype=torch.int16, device=dev)
    views = (C.c_void_p * 2)(hm.data_ptr(), hm.data_ptr())
    gs = (C.c_float * 3)(8000, 8000, 2000)
    st = (C.c_int64 * 4)(16 * 64, 64, 16, 4)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = _lib._stream(dev)
    f, fi, fs, ft = lib.sp3d_unproject_fwd, lib.sp3d_unproject_fwd_indexed, lib.sp3d_unproject_fwd_strided, lib.sp3d_unproject_fwd_train
    for layout, jp in ((_lib.LAYOUT_PLANAR, 15), (_lib.LAYOUT_NHWC, 16)):
        for J in (2, 3):
            assert f(views, layout | one, jp, p(cam), p(cen), p(val), p(cubes), p(grids), 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, s) == -4
            assert fi(views, layout | one, jp, p(cam), None, p(cen), p(val), p(cubes), None, 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, s) == -4
            assert fs(views, layout | one, jp, p(cam), None, p(cen), p(val), p(cubes), st, 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, s) == -4
        assert f(views, layout | one | _lib.OUT_CHANNELS_LAST, jp, p(cam), p(cen), p(val), p(cubes), None, 1, 2, 1, 8, 8, 4, 4, 4,
                 gs, 96, 72, s) == -4
        assert f(views, layout | one | _lib.OUT_BF16, jp, p(cam), p(cen), p(val), p(cubes), None, 1, 2, 4, 8, 8, 4, 4, 4, gs, 96, 72, s) == -4
        assert f(views, layout | one | _lib.HM_BF16, jp, p(cam), p(cen), p(val), p(cubes), None, 1, 2, 4, 8, 8, 4, 4, 4, gs, 96, 72, s) == -4
        assert f(views, layout | one, jp, p(cam), p(cen), p(val), p(cubes), None, 1, 2, 4, 8, 1, 4, 4, 4, gs, 96, 72, s) == -4
    assert ft(views, _lib.LAYOUT_NHWC | one, 16, p(cam), None, p(cen), p(val), p(cubes), None, p(mask), 1, 2, 4, 8, 8, 4, 4, 4,
              gs, 96, 72, s) == -4
    torch.cuda.synchronize(dev)
    assert not bool(cubes.any())


# ---- ProjectLayer ----------------------------------------------------------------------------------------------------------
SMALL = dict(NETWORK__IMAGE_SIZE=[384, 288], NETWORK__HEATMAP_SIZE=[96, 72], MULTI_PERSON__INITIAL_CUBE_SIZE=[24, 24, 8])


def _small_scene(dev, B, seed, J=15):
    from selfpose3d_amd import _lib, synthetic as syn
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    meta = syn.make_meta(B, 5, (384, 288))
    planar = [h.to(dev) for h in syn.people_heatmaps(B, 5, J, 72, 96, (384, 288), seed=seed)[0]]
    packed = _lib.pack_heatmaps(planar, jp=16)
    return meta, planar, nhwc_heatmap_views(packed, J)


class _PackSpy:
    def __init__(self, monkeypatch):
        from selfpose3d_amd import _lib
        self.calls = 0
        inner = _lib.pack_heatmaps

        def spy(*a, **k):
            self.calls += 1
            return inner(*a, **k)
        monkeypatch.setattr(_lib, "pack_heatmaps", spy)


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
@pytest.mark.parametrize("B", [1, 2])
def test_project_layer_reads_the_slice_in_place(dev, monkeypatch, hand_over, B):
    from oracle import oracle
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    cfg = load_config(None, **SMALL)
    meta, planar, nhwc = _small_scene(dev, B, 40 + B)
    ch = 2
    hms = [a[:, ch:ch + 1] for a in (planar if hand_over == "planar" else nhwc)]
    layer = ProjectLayer(cfg)
    spy = _PackSpy(monkeypatch)
    results = {}
    for on in (True, False):
        layer.one_channel = on
        clear_pack_cache()
        spy.calls = 0
        with torch.no_grad():
            res = [layer(hms, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8]),
                   layer.get_voxel(hms, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8], want_grids=False,
                                   pad_channels=True, channels_last=True),
                   layer.get_voxel(hms, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8], want_grids=False,
                                   pad_channels=True)]
            out = torch.full((B, 1, 30, 30, 12), float("nan"), device=dev)[:, :, :24, :24, :8]
            layer.get_voxel(hms, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8], want_grids=False, out=out)
        results[on] = res + [(out, None)]
        assert (spy.calls == 0) if on else (spy.calls >= 1), (on, spy.calls)      # no re-tiling pass on the new path
    for (c1, g1), (c0, g0) in zip(results[True], results[False]):
        assert c1.shape == c0.shape and c1.stride() == c0.stride() and torch.equal(c1, c0)
        assert (g1 is None and g0 is None) or torch.equal(g1, g0)
    assert results[True][1][0].shape == (B, 4, 24, 24, 8)
    assert results[True][1][0].is_contiguous(memory_format=torch.channels_last_3d)
    cam = pack_cameras(meta, B, (384, 288))
    centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), B, 0)
    want, want_g = oracle.unproject_fwd([np.ascontiguousarray(h.cpu().numpy()) for h in hms], cam, centers, np.ones(B, np.uint8),
                                        syn.SPACE_SIZE, (24, 24, 8), (384, 288))
    assert np.array_equal(results[True][0][0].cpu().numpy(), want) and np.array_equal(results[True][0][1].cpu().numpy(), want_g)
    assert float(want.max()) > 0.2


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
def test_project_layer_gradient_keeps_the_packed_path(dev, monkeypatch, hand_over):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    cfg = load_config(None, **SMALL)
    B = 2
    meta, planar, nhwc = _small_scene(dev, B, 50)
    layer = ProjectLayer(cfg)
    layer.deterministic_backward = True
    spy = _PackSpy(monkeypatch)
    w = torch.from_numpy(np.random.default_rng(3).random((B, 1, 24, 24, 8), dtype=np.float32)).to(dev)
    grads, cubes = {}, {}
    for on in (True, False):
        layer.one_channel = on
        clear_pack_cache()
        spy.calls = 0
        src = [a.clone().requires_grad_(True) for a in (planar if hand_over == "planar" else nhwc)]
        c, _ = layer([a[:, 2:3] for a in src], meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])
        assert spy.calls >= 1, "a heat-map gradient keeps the packed forward and its pass mask"
        (c * w).sum().backward()
        grads[on], cubes[on] = [a.grad.clone() for a in src], c.detach()
    assert torch.equal(cubes[True], cubes[False])
    for a, b in zip(grads[True], grads[False]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
        assert not bool(a[:, :2].any()) and not bool(a[:, 3:].any())


# ---- the ROOTNET_ROOTHM root nets ------------------------------------------------------------------------------------------
def _set_switch(net, on):
    net.project_layer.one_channel = on


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
@pytest.mark.parametrize("size", ["small", "full"])
def test_root_nets_switch_on_equals_off(dev, monkeypatch, hand_over, size):
    from selfpose3d_amd import _lib, synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
    from selfpose3d_amd.graphs import GraphedRootNet
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    over = dict(NETWORK__ROOTNET_ROOTHM=True, NETWORK__ROOTNET_TRAIN_SYNTH=True)
    if size == "small":
        B = 2
        cfg = load_config(None, **SMALL, **over)
        meta, planar, nhwc = _small_scene(dev, B, 60)
    else:
        B = 1
        cfg = load_config(None, **over)
        meta = syn.make_meta(B, 5, list(IMG))
        planar = [h.to(dev) for h in syn.people_heatmaps(B, 5, 15, HM[1], HM[0], IMG, seed=61)[0]]
        nhwc = nhwc_heatmap_views(_lib.pack_heatmaps(planar, jp=16), 15)
    hms = planar if hand_over == "planar" else nhwc
    spy = _PackSpy(monkeypatch)
    soft = CuboidProposalNetSoft(cfg)
    syn.fill_parameters_deterministic(soft, seed=5, scale=0.05)
    soft.to(dev).eval()
    nets = []
    for cl in (False, True):
        plain = CuboidProposalNet(cfg)
        plain.load_state_dict(soft.state_dict())
        nets.append(plain.to(dev).eval().use_channels_last(cl))
    for net in nets + [soft]:
        outs = {}
        for on in (True, False):
            _set_switch(net, on)
            spy.calls = 0
            with torch.no_grad():
                r = net(hms, meta) if net is not soft else soft.get_grid_centres(hms, meta)
            outs[on] = [t.clone() for t in r]
            assert (spy.calls == 0) if on else (spy.calls >= 1), (type(net).__name__, on, spy.calls)
        assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
        assert float(outs[True][0].abs().max()) > 0
    # training mode with the synthetic-root branch: rendered (B,1,h,w) maps take the new kernel too (planar, Jp = 1)
    soft.train()
    outs = {}
    for on in (True, False):
        _set_switch(soft, on)
        soft.generator = torch.Generator().manual_seed(7)
        spy.calls = 0
        rc, syn_cubes, target, gc = soft(hms, meta)
        outs[on] = [t.detach().clone() for t in (rc, syn_cubes, target, gc)]
        assert (spy.calls == 0) if on else (spy.calls >= 2), (on, spy.calls)
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    assert float(outs[True][1].abs().max()) > 0 and float(outs[True][2].max()) > 0.5
    # a captured graph replays the new path, equals eager, and reads the caller's buffers: new heat-maps written into them
    # (the planar tensors / the channels-last buffer behind the views) reach the kernel on the next replay
    net = nets[1]
    _set_switch(net, True)
    seed2 = 62 if size == "small" else 63
    h, w, img = (72, 96, (384, 288)) if size == "small" else (HM[1], HM[0], IMG)
    planar2 = [x.to(dev) for x in syn.people_heatmaps(B, 5, 15, h, w, img, seed=seed2)[0]]
    hms2 = planar2 if hand_over == "planar" else nhwc_heatmap_views(_lib.pack_heatmaps(planar2, jp=16), 15)
    with torch.no_grad():
        eager = [t.clone() for t in net(hms, meta)]
        eager2 = [t.clone() for t in net(hms2, meta)]
    assert not torch.equal(eager[0], eager2[0])
    if hand_over == "planar":
        static = [x.clone() for x in planar]
    else:
        static_buf = _lib.pack_heatmaps(planar, jp=16)
        static = nhwc_heatmap_views(static_buf, 15)
    spy.calls = 0
    g = GraphedRootNet(net, static, meta)
    assert spy.calls == 0
    out = g()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    if hand_over == "planar":
        for dst, src in zip(static, planar2):
            dst.copy_(src)
    else:
        static_buf.copy_(_lib.pack_heatmaps(planar2, jp=16))
    out = g()
    assert torch.equal(out[0], eager2[0]) and torch.equal(out[1], eager2[1])


class _FwdSpy:
    """records the one_channel keyword of every _lib.unproject_fwd call"""

    def __init__(self, monkeypatch):
        from selfpose3d_amd import _lib
        self.seen = []
        inner = _lib.unproject_fwd

        def spy(*a, **k):
            self.seen.append(bool(k.get("one_channel", False)))
            return inner(*a, **k)
        monkeypatch.setattr(_lib, "unproject_fwd", spy)


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
def test_project_layer_when_the_new_path_is_taken_and_when_not(dev, monkeypatch, hand_over):
    """mode "auto" and "nhwc" with fp32 storage take it; mode "planar", bf16 storage, the switch off and J != 1 do not"""
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    cfg = load_config(None, **SMALL)
    B = 2
    meta, planar, nhwc = _small_scene(dev, B, 70)
    full = planar if hand_over == "planar" else nhwc
    hms = [a[:, 2:3] for a in full]
    spy = _FwdSpy(monkeypatch)
    args = (meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])

    def run(layer, maps, on=True, **kw):
        layer.one_channel = on
        clear_pack_cache()
        spy.seen.clear()
        with torch.no_grad():
            c, _ = layer.get_voxel(maps, *args, **kw)
        assert len(spy.seen) == 1
        return spy.seen[0], c
    took, ref = run(ProjectLayer(cfg), hms)
    assert took
    took, c = run(ProjectLayer(cfg, mode="nhwc"), hms)
    assert took and torch.equal(c, ref)
    took, c = run(ProjectLayer(cfg, mode="planar"), hms)
    assert not took and torch.equal(c, ref)
    took, c = run(ProjectLayer(cfg), hms, on=False)
    assert not took and torch.equal(c, ref)
    took, _ = run(ProjectLayer(cfg), [a[:, 2:4] for a in full])                  # two channels
    assert not took
    took, _ = run(ProjectLayer(cfg), [a[:, 2:3].double() for a in full])         # float64 callers keep the packed path
    assert not took
    # bf16 storage applies from 13 joints on, where the classifier (J == 1) never answers; one joint is refused as before
    took, _ = run(ProjectLayer(cfg, io_dtype=torch.bfloat16), full)
    assert not took
    with pytest.raises(Exception):
        ProjectLayer(cfg, io_dtype=torch.bfloat16).get_voxel(hms, *args)


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
def test_project_layer_sample_of_more_cubes_than_samples(dev, monkeypatch, hand_over):
    """P = 5 cubes read from B = 2 samples: forward() sizes the result by the cubes while the classifier looks at the batch"""
    from oracle import oracle
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    cfg = load_config(None, **SMALL)
    B, P, cube, gs = 2, 5, [16, 16, 16], [2000.0, 2000.0, 2000.0]
    meta, planar, nhwc = _small_scene(dev, B, 71)
    hms = [a[:, 2:3] for a in (planar if hand_over == "planar" else nhwc)]
    rng = np.random.default_rng(5)
    sample_of = np.array([1, 0, 0, 1, 1], np.int64)
    gc = np.zeros((P, 5), np.float32)
    gc[:, :3] = np.stack([rng.uniform(-1500, 1500, P), rng.uniform(-1500, 1500, P), rng.uniform(700, 1100, P)], 1)
    gc[2, 3] = -1.0                                                                      # a skipped cube
    spy = _FwdSpy(monkeypatch)
    layer = ProjectLayer(cfg)
    got = {}
    for on in (True, False):
        layer.one_channel = on
        clear_pack_cache()
        spy.seen.clear()
        with torch.no_grad():
            got[on] = layer.get_voxel(hms, meta, gs, torch.from_numpy(gc).to(dev), cube, sample_of=torch.from_numpy(sample_of).to(dev))
        assert spy.seen == [on]
    assert got[True][0].shape == (P, 1, 16, 16, 16) and got[True][1].shape == (P, 16 ** 3, 3)
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    cam = pack_cameras(meta, B, (384, 288))
    want, want_g = oracle.unproject_fwd([np.ascontiguousarray(x.cpu().numpy())[sample_of] for x in hms], cam[sample_of],
                                        np.ascontiguousarray(gc[:, :3]), (gc[:, 3] >= 0).astype(np.uint8), gs, cube, (384, 288))
    assert np.array_equal(got[True][0].cpu().numpy(), want) and np.array_equal(got[True][1].cpu().numpy(), want_g)
    assert not np.any(want[2]) and float(want.max()) > 0.2
