"""bf16 heat-maps through the fused fronts (SP3D_HM_BF16_IN; ``ProjectLayer.bf16_maps``, ``use_bf16_heatmaps()``, default off).
The plans and the refusals are pinned on the host by tests/test_bf16_front_host.py; this file holds the values.

Every comparison is BITWISE (the raw 32-bit words, a NaN equal to a NaN) unless it says otherwise, and the referee is always the
existing fp32 route run on the widened maps (``hm.bfloat16().float()``), which the older tests pin to the oracle:

1. the brick-h kernel with the z-spectrum result: 13..16 joints against zdft_fwd_cl of the fp32 channels-last cubes, 17..32
   joints against unproject_fwd_zspectrum on the widened packed maps; B = 1, a skipped sample, more cubes than samples;
2. the one-channel kernels, cubes and spectrum: the channel read in place at odd and even indices of planar and channels-last
   bf16 tensors, every result form, against the fp32 one-channel kernel;
3. the rounding bound max |cubes(bf16 maps) - cubes(maps before rounding)| <= 2^-8 max |hm| x 1.001 (derived: bf16 has a unit
   round-off of 2^-8, bilinear weights are non-negative and sum to at most 1, view fusion divides by the count, the clamp is
   1-Lipschitz; the factor 1.001 = 6.6e-6 at this range covers the fp32 rounding of both runs, ~1e-7 x range); for a
   z-spectrum the DFT is linear with unit-modulus twiddles, so a bin moves by at most Z = 20 times that;
4. the model classes under ``use_bf16_heatmaps()`` against the same net on the widened maps, the route counted;
5. the fall-backs, autograd, and the refusals that stay."""
import numpy as np
import pytest
import torch

from tests import front_sweep_cases as fs

pytestmark = pytest.mark.gpu

SZ, K = 28, 15
GUARD = 4096                                         # floats on either side of a guarded result
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def same_bits(a, b):
    """the raw words are equal, or both values are NaN"""
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def guarded(shape, dev, complex_=False):
    """a NaN-filled buffer, and a 128-byte aligned dense tensor of ``shape`` inside it with GUARD floats on either side"""
    n = int(np.prod(shape)) * (2 if complex_ else 1)
    buf = torch.full((n + 2 * GUARD + 32,), float("nan"), dtype=F32, device=dev)
    off = GUARD + (-(buf.data_ptr() + 4 * GUARD) % 128) // 4
    inner = buf[off:off + n]
    out = torch.view_as_complex(inner.view(tuple(shape) + (2,))) if complex_ else inner.view(tuple(shape))
    return buf, off, n, out


def guards_untouched(buf, off, n):
    return bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all())


_scenes = {}


def scene(dev, B, V, hw, C, seed, P=None, valid=None, nan=True):
    """maps (V,B,h,w,C) uniform in [-0.7, 1.7) so that the clamp acts, before rounding (``raw``), rounded to bf16 (``bf``) and
    widened again (``wide``); one NaN pixel in one view of the rounded maps; camera table, centres shifted per cube, valid
    flags, sample_of (p mod B) for P cubes.  Built once per key and left unchanged."""
    key = (B, V, hw, C, seed, P, valid, nan)
    if key not in _scenes:
        from selfpose3d_amd import synthetic as syn
        from selfpose3d_amd.camera_pack import pack_cameras
        h, w = hw
        img = [4 * w, 4 * h]
        rng = np.random.default_rng(seed)
        raw = torch.from_numpy(rng.random((V, B, h, w, C), dtype=np.float32) * 2.4 - 0.7)
        bf = raw.to(BF)
        if nan:
            bf[V // 2, B - 1, h // 2, w // 2, :] = float("nan")
        n = B if P is None else P
        centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), n, 0)
        centers[:, 0] += 250.0 * np.arange(n, dtype=np.float32)
        centers[:, 1] -= 130.0 * np.arange(n, dtype=np.float32)
        val = np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8)
        meta = syn.make_meta(B, V, img)
        _scenes[key] = dict(raw=raw.to(dev), bf=bf.to(dev), wide=bf.float().to(dev), img=img, meta=meta, grid_size=syn.SPACE_SIZE,
                            args=(torch.from_numpy(pack_cameras(meta, B, img)).to(dev), torch.from_numpy(centers).to(dev),
                                  torch.from_numpy(val).to(dev)),
                            sample_of=None if P is None else torch.arange(n, dtype=torch.int32, device=dev) % B, n=n,
                            hmax=float(raw.abs().max()))
    return _scenes[key]


# ---- 1. the brick-h kernel with the z-spectrum result -------------------------------------------------------------------------
MODES = [dict(B=1), dict(B=3, valid=(1, 0, 1)), dict(B=2, P=4)]


def zspectrum_referee(s, maps, jp, J, cube):
    """fp32 maps -> the spectrum of the existing routes: at Jp = 16 zdft_fwd_cl of the channels-last cubes, tiled 4 x 4; at
    Jp = 32 unproject_fwd_zspectrum.  A cube that ``valid`` skips is zeros either way."""
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    V, B, h, w, _ = maps.shape
    views = [maps[c] for c in range(V)]
    if jp == 16:
        if s["sample_of"] is not None:      # the spectrum entries of the C ABI take sample_of; the channels-last cubes do as well
            cubes, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, 16, *s["args"], s["n"], 16, h, w, cube, s["grid_size"], s["img"], False,
                                          channels_last=True, sample_of=s["sample_of"])
        else:
            cubes, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, 16, *s["args"], s["n"], 16, h, w, cube, s["grid_size"], s["img"], False,
                                          channels_last=True)
        return fs.tile44(_lib.zdft_fwd_cl(cubes, J, (X, Y, SZ)))
    assert s["sample_of"] is None
    return _lib.unproject_fwd_zspectrum(views, 32, *s["args"], B, J, h, w, cube, s["grid_size"], s["img"], SZ)


def zspectrum_bf16(s, maps, jp, J, cube, out):
    """the new launch(es) through the C entry that takes sample_of (unproject_fwd_zspectrum has none), into ``out``"""
    from selfpose3d_amd import _lib
    V, B, h, w, _ = maps.shape
    X, Y, Z = cube
    flags = _lib.LAYOUT_NHWC | _lib.OUT_ZSPECTRUM | (_lib.HM_BF16_IN if maps.dtype == BF else 0)
    cam, centers, valid = s["args"]
    rc = _lib.load().sp3d_unproject_fwd_indexed(_lib._ptr_array([maps[c] for c in range(V)]), flags, jp, cam.data_ptr(),
                                               _lib._opt(s["sample_of"]), centers.data_ptr(), valid.data_ptr(), out.data_ptr(), None,
                                               s["n"], V, J, h, w, X, Y, Z, _lib._f3(s["grid_size"]), s["img"][0], s["img"][1],
                                               _lib._stream(maps.device))
    _lib.check(rc, "sp3d_unproject_fwd_indexed (bf16 z-spectrum)")
    return out


@pytest.mark.parametrize("V", [1, 3, 5])
@pytest.mark.parametrize("hw", [(2, 2), (9, 7), (18, 24)])
@pytest.mark.parametrize("cube", [(4, 4, 20), (8, 12, 20)])
def test_zspectrum_from_bf16_pixels(dev, cube, hw, V):
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    for jp, joints in ((16, (13, 15, 16)), (32, (17, 21, 32))):
        for mi, mode in enumerate(MODES):
            s = scene(dev, mode["B"], V, hw, jp, 100 * V + 10 * mi + jp, P=mode.get("P"), valid=mode.get("valid"))
            clean = scene(dev, mode["B"], V, hw, jp, 100 * V + 10 * mi + jp, P=mode.get("P"), valid=mode.get("valid"), nan=False)
            for J in joints:
                shape = (s["n"], J, K, X // 4, Y // 4, 16)
                buf, off, n, out = guarded(shape, dev, complex_=True)
                got = zspectrum_bf16(s, s["bf"], jp, J, cube, out)
                if mode.get("P") is not None and jp == 32:
                    # more cubes than samples at Jp = 32: the fp32 form of the same entry is the referee
                    ref = zspectrum_bf16(s, s["wide"], jp, J, cube, torch.empty(shape, dtype=torch.complex64, device=dev))
                else:
                    ref = zspectrum_referee(s, s["wide"], jp, J, cube)
                torch.cuda.synchronize(dev)
                tag = (cube, hw, V, jp, J, mode)
                assert guards_untouched(buf, off, n), (tag, "a store outside the spectrum")
                assert same_bits(got, ref), (tag, float(torch.nan_to_num(torch.view_as_real(got) - torch.view_as_real(ref)).abs().max()))
                if mode.get("valid") is not None:
                    assert int(torch.count_nonzero(torch.view_as_real(got[1]))) == 0, (tag, "the skipped sample's lines are not zero")
                    assert float(torch.nan_to_num(torch.view_as_real(got[0])).abs().max()) > 0.0
                # the rounding bound, on maps without the NaN pixel, Z times the cubes' bound per bin
                a = zspectrum_bf16(clean, clean["bf"], jp, J, cube, torch.empty(shape, dtype=torch.complex64, device=dev))
                b = zspectrum_bf16(clean, clean["raw"], jp, J, cube, torch.empty(shape, dtype=torch.complex64, device=dev))
                d = float((a - b).abs().max())
                assert bool(torch.isfinite(torch.view_as_real(a)).all()) and float(a.abs().max()) > 0.0
                assert d <= Z * 2.0 ** -8 * clean["hmax"] * 1.001, (tag, d)
    # the Python binding derives the flag from the views' type
    s = scene(dev, 1, V, hw, 32, 100 * V + 32)
    got = _lib.unproject_fwd_zspectrum([s["bf"][c] for c in range(V)], 32, *s["args"], 1, 21, hw[0], hw[1], cube, s["grid_size"], s["img"], SZ)
    ref = _lib.unproject_fwd_zspectrum([s["wide"][c] for c in range(V)], 32, *s["args"], 1, 21, hw[0], hw[1], cube, s["grid_size"], s["img"], SZ)
    assert same_bits(got, ref)


# ---- 2. the one-channel kernels -----------------------------------------------------------------------------------------------
def one_sources(s):
    """[(name, bf16 views, widened fp32 views of the same form)]: the channel where it lies in a planar (B,15,h,w) tensor (an
    even and an odd index), in the (V,B,h,w,16) and (V,B,h,w,32) buffers (odd indices included: pointers that are 2-byte
    aligned only), and as a contiguous (B,1,h,w) tensor"""
    V = s["bf"].shape[0]
    out = []
    for name, maps in (("bf", s["bf"]), ("wide", s["wide"])):
        planar = [maps[c, ..., :15].permute(0, 3, 1, 2).contiguous() for c in range(V)]          # (B,15,h,w)
        p16 = maps[..., :16].contiguous()
        forms = [("planar2", [x[:, 2:3] for x in planar]), ("planar7", [x[:, 7:8] for x in planar]),
                 ("nhwc16_4", [p16[c].permute(0, 3, 1, 2)[:, 4:5] for c in range(V)]),
                 ("nhwc16_5", [p16[c].permute(0, 3, 1, 2)[:, 5:6] for c in range(V)]),
                 ("nhwc32_19", [maps[c].permute(0, 3, 1, 2)[:, 19:20] for c in range(V)]),
                 ("contiguous", [x[:, 3:4].contiguous() for x in planar])]
        out.append(forms)
    return [(n, b, w) for (n, b), (_, w) in zip(*out)]


def classify(views, dtype):
    from selfpose3d_amd.project_layer import one_channel_source
    one = one_channel_source(views, dtype)
    assert one is not None
    return one


@pytest.mark.parametrize("V", [1, 5, 7, 11, 16])
def test_one_channel_cubes_from_bf16_maps(dev, V):
    from selfpose3d_amd import _lib
    cube, hw = (5, 7, 3), (9, 7)
    X, Y, Z = cube
    for mode in (dict(B=2), dict(B=2, P=5)):
        s = scene(dev, mode["B"], V, hw, 32, 300 + V, P=mode.get("P"))
        clean = scene(dev, mode["B"], V, hw, 32, 300 + V, P=mode.get("P"), nan=False)
        P, so = s["n"], s["sample_of"]
        kw = dict(sample_of=so, one_channel=True)
        for (name, bf, wide), (_, cbf, _) in zip(one_sources(s), one_sources(clean)):
            layout, jp = classify(bf, BF)
            assert (layout, jp) == classify(wide, F32)
            assert bf[0].data_ptr() % 2 == 0
            run = lambda views, J, **k: _lib.unproject_fwd(views, layout, jp, *s["args"], P, J, hw[0], hw[1], cube, s["grid_size"],
                                                           s["img"], k.pop("grids", False), **kw, **k)
            for J in (1, 4):                                                         # dense
                got, gg = run(bf, J, grids=True)
                ref, rg = run(wide, J, grids=True)
                assert got.dtype == F32 and tuple(got.shape) == (P, J, X, Y, Z)
                assert same_bits(got, ref) and same_bits(gg, rg), (V, mode, name, J)
            got, _ = run(bf, 4, channels_last=True)                                  # channels-last (P,X,Y,Z,4)
            ref, _ = run(wide, 4, channels_last=True)
            assert got.is_contiguous(memory_format=torch.channels_last_3d) and same_bits(got, ref), (V, mode, name, "channels-last")
            for J in (1, 4):                                                         # strided into a larger buffer, guarded
                buf, off, n, big = guarded((P, J + 1, X + 2, Y + 1, Z + 3), dev)
                out = big[:, :J, 1:X + 1, :Y, 2:Z + 2]
                run(bf, J, out=out)
                ref, _ = run(wide, J)
                torch.cuda.synchronize(dev)
                assert same_bits(out, ref), (V, mode, name, J, "strided")
                mask = torch.ones_like(big, dtype=torch.bool)
                mask[:, :J, 1:X + 1, :Y, 2:Z + 2] = False
                assert bool(torch.isnan(big[mask]).all()) and guards_untouched(buf, off, n), (name, "a store outside the cubes")
            # the rounding bound: the same channel of the maps before rounding, no NaN pixel
            a, _ = _lib.unproject_fwd(cbf, layout, jp, *clean["args"], P, 1, hw[0], hw[1], cube, clean["grid_size"], clean["img"], False, **kw)
            raw = [x.float() for x in cbf]                                          # the widened form, then the unrounded values
            for c in range(V):
                raw[c].copy_({"planar2": clean["raw"][c, ..., 2:3], "planar7": clean["raw"][c, ..., 7:8], "nhwc16_4": clean["raw"][c, ..., 4:5],
                              "nhwc16_5": clean["raw"][c, ..., 5:6], "nhwc32_19": clean["raw"][c, ..., 19:20],
                              "contiguous": clean["raw"][c, ..., 3:4]}[name].permute(0, 3, 1, 2))
            lay32, jp32 = classify(raw, F32)
            b, _ = _lib.unproject_fwd(raw, lay32, jp32, *clean["args"], P, 1, hw[0], hw[1], cube, clean["grid_size"], clean["img"], False, **kw)
            d = float((a - b).abs().max())
            assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0
            assert d <= 2.0 ** -8 * clean["hmax"] * 1.001, (V, mode, name, d)


@pytest.mark.parametrize("V", [1, 5, 7, 11, 16])
def test_one_channel_spectrum_from_bf16_maps(dev, V):
    from selfpose3d_amd import _lib
    cube, hw = (8, 12, 20), (9, 7)
    X, Y, Z = cube
    for mode in (dict(B=2), dict(B=3, valid=(1, 0, 1)), dict(B=2, P=5)):
        s = scene(dev, mode["B"], V, hw, 32, 400 + V, P=mode.get("P"), valid=mode.get("valid"))
        P = s["n"]
        for name, bf, wide in one_sources(s):
            layout, jp = classify(bf, BF)
            shape = (P, 1, K, X // 4, Y // 4, 16)
            buf, off, n, out = guarded(shape, dev, complex_=True)
            got = _lib.unproject_one_fwd_zspectrum(bf, layout, jp, *s["args"], P, hw[0], hw[1], cube, s["grid_size"], s["img"], SZ,
                                                   sample_of=s["sample_of"], out=out)
            ref = _lib.unproject_one_fwd_zspectrum(wide, layout, jp, *s["args"], P, hw[0], hw[1], cube, s["grid_size"], s["img"], SZ,
                                                   sample_of=s["sample_of"])
            torch.cuda.synchronize(dev)
            assert got.data_ptr() == out.data_ptr() and guards_untouched(buf, off, n), (name, "a store outside the spectrum")
            assert same_bits(got, ref), (V, mode, name)
            if mode.get("valid") is not None:
                assert int(torch.count_nonzero(torch.view_as_real(got[1]))) == 0
            assert float(torch.nan_to_num(torch.view_as_real(got)).abs().max()) > 0.0
    # the rounding bound (Z times the cubes' bound per bin), the maps before rounding as a contiguous fp32 channel
    clean = scene(dev, 2, V, hw, 32, 400 + V, nan=False)
    bf = [clean["bf"][c, ..., 19:20].permute(0, 3, 1, 2) for c in range(V)]
    raw = [clean["raw"][c, ..., 19:20].permute(0, 3, 1, 2).contiguous() for c in range(V)]
    a = _lib.unproject_one_fwd_zspectrum(bf, *classify(bf, BF), *clean["args"], 2, hw[0], hw[1], cube, clean["grid_size"], clean["img"], SZ)
    b = _lib.unproject_one_fwd_zspectrum(raw, *classify(raw, F32), *clean["args"], 2, hw[0], hw[1], cube, clean["grid_size"], clean["img"], SZ)
    assert bool(torch.isfinite(torch.view_as_real(a)).all()) and float(a.abs().max()) > 0.0
    assert float((a - b).abs().max()) <= Z * 2.0 ** -8 * clean["hmax"] * 1.001


def test_project_layer_one_channel_route(dev, monkeypatch):
    """``ProjectLayer.bf16_maps`` with ``one_channel``: a bf16 one-channel list goes through the bf16 one-channel kernel in every
    result form of ``get_voxel``; with ``one_channel`` off there is no bf16 kernel for one joint and the widened maps take the
    fp32 path.  Both equal the fp32 layer on the widened tensors."""
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    img, hm, B, V = (96, 72), (24, 18), 2, 3
    cfg = load_config(None, NETWORK__IMAGE_SIZE=list(img), NETWORK__HEATMAP_SIZE=list(hm))
    meta = syn.make_meta(B, V, list(img))
    full = [h.to(dev).to(BF) for h in syn.random_heatmaps(B, V, 15, hm[1], hm[0], seed=12)]
    bf, wide = [a[:, 7:8] for a in full], [a.float()[:, 7:8] for a in full]
    geo = (meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])

    def forms(layer, hms):
        with torch.no_grad():
            res = list(layer.get_voxel(hms, *geo))
            res.append(layer.get_voxel(hms, *geo, want_grids=False, pad_channels=True, channels_last=True)[0])
            res.append(layer.get_voxel(hms, *geo, want_grids=False, pad_channels=True)[0])
            out = torch.full((B, 1, 30, 30, 12), float("nan"), device=dev)[:, :, :24, :24, :8]
            layer.get_voxel(hms, *geo, want_grids=False, out=out)
        return res + [out]
    ref_layer = ProjectLayer(cfg)
    ref_layer.one_channel = True
    ref = forms(ref_layer, wide)
    for one in (True, False):
        layer = ProjectLayer(cfg)
        layer.bf16_maps, layer.one_channel = True, one
        clear_pack_cache()
        spy = _Spy(monkeypatch)
        got = forms(layer, bf)
        assert set(spy.n) == ({("unproject_fwd", BF)} if one else {("pack_heatmaps", F32), ("unproject_fwd", F32)}), spy.n
        for g, r in zip(got, ref):
            assert g.dtype == F32 and g.stride() == r.stride() and same_bits(g, r), one
    assert float(ref[0].abs().max()) > 0.0


# ---- 4. the model classes -----------------------------------------------------------------------------------------------------
class _Spy:
    """counts the calls of the spectrum entries (by the type of the views they get), of the cube-writing entry and of the
    re-tiling pass"""

    def __init__(self, monkeypatch):
        from selfpose3d_amd import _lib
        self.n = {}
        for name in ("unproject_fwd_zspectrum", "unproject_one_fwd_zspectrum", "unproject_fwd_zdft", "unproject_fwd", "pack_heatmaps"):
            inner = getattr(_lib, name)

            def spy(views, *a, _inner=inner, _name=name, **k):
                key = (_name, views[0].dtype)
                self.n[key] = self.n.get(key, 0) + 1
                return _inner(views, *a, **k)
            monkeypatch.setattr(_lib, name, spy)


def _bf16_and_widened(planar, J, jp):
    """fp32 (B,J,h,w) maps -> the views of a bf16 (V,B,h,w,jp) buffer, and the views of the fp32 buffer of the same values"""
    from selfpose3d_amd import _lib
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    packed = _lib.pack_heatmaps(planar, jp=jp).to(BF)
    return nhwc_heatmap_views(packed, J), nhwc_heatmap_views(packed.float(), J)


def _run_pair(net, run, bf, wide, monkeypatch, want_route):
    """``run(hms)`` with the switch off on the widened maps, then with ``use_bf16_heatmaps()`` on the bf16 views: the same
    tensors, bit for bit, and exactly the route ``want_route`` = {(entry, dtype): calls}"""
    with torch.no_grad():
        ref = [t.clone() for t in run(wide)]
        spy = _Spy(monkeypatch)
        net.use_bf16_heatmaps()
        try:
            got = [t.clone() for t in run(bf)]
        finally:
            net.use_bf16_heatmaps(False)
    assert spy.n == want_route, spy.n
    assert bool(torch.isfinite(ref[0]).all()) and float(ref[0].abs().max()) > 0.0
    for g, r in zip(got, ref):
        assert same_bits(g.float(), r.float())
    return got


def test_root_net_15_joints(dev, monkeypatch):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    img, hm, J, B, V = (96, 72), (24, 18), 15, 1, 5
    cfg = load_config(None, NETWORK__IMAGE_SIZE=list(img), NETWORK__HEATMAP_SIZE=list(hm))
    assert [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE] == [80, 80, 20] and not bool(cfg.NETWORK.ROOTNET_ROOTHM)
    net = CuboidProposalNet(cfg)
    syn.fill_parameters_deterministic(net, seed=5, scale=0.05)
    net.to(dev).eval().use_channels_last(True)
    meta = syn.make_meta(B, V, list(img))
    planar = [h.to(dev) for h in syn.people_heatmaps(B, V, J, hm[1], hm[0], img, seed=41)[0]]
    bf, wide = _bf16_and_widened(planar, J, 16)
    _run_pair(net, lambda hms: net(hms, meta), bf, wide, monkeypatch, {("unproject_fwd_zspectrum", BF): 1})


@pytest.mark.parametrize("which", ["plain", "soft"])
def test_roothm_root_nets(dev, monkeypatch, which):
    import os
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
    img, hm, J, B, V = (96, 72), (24, 18), 15, 1, 5
    yaml = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cam5_posenet.yaml")
    cfg = load_config(yaml, NETWORK__IMAGE_SIZE=list(img), NETWORK__HEATMAP_SIZE=list(hm))
    assert bool(cfg.NETWORK.ROOTNET_ROOTHM)
    net = (CuboidProposalNet if which == "plain" else CuboidProposalNetSoft)(cfg)
    syn.fill_parameters_deterministic(net, seed=5, scale=0.05)
    net.to(dev).eval().use_channels_last(True)
    net.project_layer.one_zspectrum = net.v2v_net.one_front = True
    meta = syn.make_meta(B, V, list(img))
    planar = [h.to(dev) for h in syn.people_heatmaps(B, V, J, hm[1], hm[0], img, seed=41)[0]]
    run = (lambda hms: net(hms, meta)) if which == "plain" else (lambda hms: net.get_grid_centres(hms, meta))
    bf, wide = _bf16_and_widened(planar, J, 16)
    _run_pair(net, run, bf, wide, monkeypatch, {("unproject_one_fwd_zspectrum", BF): 1})
    # planar bf16 tensors hand the channel over in place as well
    pbf = [h.to(BF) for h in planar]
    _run_pair(net, run, pbf, [h.float() for h in pbf], monkeypatch, {("unproject_one_fwd_zspectrum", BF): 1})


def test_root_net_17_joints(dev, monkeypatch):
    from tests.test_gpu_coco17 import _nets, _people_heatmaps
    cfg, root, _ = _nets(dev)
    root.use_channels_last(True)
    root.project_layer.wide_zspectrum = root.v2v_net.wide_front = True
    hms, meta = _people_heatmaps(cfg, 1, seed=11)
    bf, wide = _bf16_and_widened([h.to(dev) for h in hms], 17, 32)
    _run_pair(root, lambda x: root(x, meta), bf, wide, monkeypatch, {("unproject_fwd_zspectrum", BF): 1})


@pytest.mark.parametrize("chunk", [1, 8])
def test_pose_net_forward_batched(dev, monkeypatch, chunk):
    import os
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.pose_regression_net import PoseRegressionNet
    yaml = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "synthetic_small.yaml")
    cfg = load_config(yaml)
    img, hm = [int(v) for v in cfg.NETWORK.IMAGE_SIZE], [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]
    J, B, V = 15, 2, 4
    net = PoseRegressionNet(cfg)
    syn.fill_parameters_deterministic(net, seed=7, scale=0.05)
    net.to(dev).eval()
    meta = syn.make_meta(B, V, img)
    planar = [h.to(dev) for h in syn.people_heatmaps(B, V, J, hm[1], hm[0], img, seed=43)[0]]
    bf, wide = _bf16_and_widened(planar, J, 16)
    centers = torch.zeros(B, 2, 5, device=dev)                                  # 3 valid proposals and 1 invalid
    centers[..., :3] = torch.tensor(syn.SPACE_CENTER, device=dev) + torch.tensor([[[0.0, 0, 0], [300, -200, 50]], [[-250, 150, 0], [0, 0, 0]]], device=dev)
    centers[..., 3] = torch.tensor([[0.0, 1.0], [0.0, -1.0]], device=dev)
    run = lambda hms: [net.forward_batched(hms, meta, centers, max_cubes_per_call=chunk)]
    got = _run_pair(net, run, bf, wide, monkeypatch, {("unproject_fwd", BF): 1})[0]
    assert tuple(got.shape) == (B, 2, J, 3) and int(torch.count_nonzero(got[1, 1])) == 0 and float(got[1, 0].abs().max()) > 0.0


def test_top_level_model_hands_bf16_over(dev):
    """MultiPersonPoseNet (configs/synthetic_small.yaml, ResNet-18) from images: under ``use_bf16_heatmaps()`` the backbone
    hands over bf16 views of one bf16 (V,B,h,w,16) buffer, and the model's result equals the switched-off model fed those maps
    widened; with grad enabled the hand-over stays fp32"""
    import os
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.multi_person_posenet import get_multi_person_pose_net
    from selfpose3d_amd.project_layer import _packed_source
    from selfpose3d_amd.synthetic_dataset import SyntheticPanoptic
    yaml = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "synthetic_small.yaml")
    cfg = load_config(yaml, MULTI_PERSON__THRESHOLD=-1e9)            # every proposal slot valid: the pose net has cubes to work on
    torch.manual_seed(1)
    model = get_multi_person_pose_net(cfg, is_train=False).to(dev).eval()
    inputs, _, _, _, meta, _ = next(iter(torch.utils.data.DataLoader(SyntheticPanoptic(cfg, num_frames=2, seed=3), batch_size=2)))
    views = [v.to(dev) for v in inputs]
    model.use_bf16_heatmaps()
    with torch.no_grad():
        pred, hms, centers = model(views=views, meta=meta)[:3]
    assert all(h.dtype == BF and tuple(h.shape[:2]) == (2, 15) for h in hms)
    packed = _packed_source(hms, 16, BF)
    assert packed is not None and packed.dtype == BF and tuple(packed.shape[:2]) == (len(views), 2)
    assert model.heatmaps(views, None)[0].dtype == F32                 # grad enabled: the switch is ignored
    model.use_bf16_heatmaps(False)
    with torch.no_grad():
        assert model.heatmaps(views, None)[0].dtype == F32
        ref, _, ref_centers = model(meta=meta, input_heatmaps=[h.float() for h in hms])[:3]
    assert same_bits(pred, ref) and same_bits(centers, ref_centers)
    assert float(pred[..., :3].abs().max()) > 0.0 and bool((pred[..., 3] >= 0).all())


# ---- 5. fall-backs, autograd, refusals ----------------------------------------------------------------------------------------
def test_fallback_widens_and_takes_the_fp32_path(dev, monkeypatch):
    """a 48 x 48 x 12 root grid (no z-spectrum front) at 15 joints re-tiles the planar bf16 maps into bf16 pixels and keeps them on
    the cube-writing kernels; a 4-joint net has no bf16 kernel at all and runs the fp32 path on the widened maps: both equal
    the widened fp32 run"""
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    img, hm, B, V = (96, 72), (24, 18), 2, 3
    meta = syn.make_meta(B, V, list(img))
    for J, jp, route in ((15, 16, {("pack_heatmaps", BF): 1, ("unproject_fwd", BF): 1}), (4, 4, {("pack_heatmaps", F32): 1, ("unproject_fwd", F32): 1})):
        cfg = load_config(None, NETWORK__IMAGE_SIZE=list(img), NETWORK__HEATMAP_SIZE=list(hm), NETWORK__NUM_JOINTS=J,
                          MULTI_PERSON__INITIAL_CUBE_SIZE=[48, 48, 12])
        net = CuboidProposalNet(cfg)
        syn.fill_parameters_deterministic(net, seed=5, scale=0.05)
        net.to(dev).eval()
        pbf = [h.to(dev).to(BF) for h in syn.people_heatmaps(B, V, J, hm[1], hm[0], img, seed=44)[0]]
        _run_pair(net, lambda hms: net(hms, meta), pbf, [h.float() for h in pbf], monkeypatch, route)


def test_autograd_ignores_the_switch(dev):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    img, hm, J, B, V = (96, 72), (24, 18), 15, 2, 3
    cfg = load_config(None, NETWORK__IMAGE_SIZE=list(img), NETWORK__HEATMAP_SIZE=list(hm))
    meta = syn.make_meta(B, V, list(img))
    maps = [h.to(dev) for h in syn.random_heatmaps(B, V, J, hm[1], hm[0], seed=9)]
    res = {}
    for on in (False, True):
        layer = ProjectLayer(cfg)
        layer.deterministic_backward = True
        layer.bf16_maps = on
        clear_pack_cache()
        hms = [m.clone().requires_grad_(True) for m in maps]
        with torch.enable_grad():
            cubes, _ = layer.get_voxel(hms, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])
            (cubes * torch.linspace(0.5, 1.5, cubes.numel(), device=dev).view_as(cubes)).sum().backward()
        res[on] = [cubes.detach()] + [h.grad for h in hms]
        with torch.no_grad():                       # ... and without grad the same layer rounds the fp32 producer's maps
            res[on].append(layer.get_voxel(hms, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])[0])
    for a, b in zip(res[True][:-1], res[False][:-1]):
        assert same_bits(a, b)
    assert float(res[False][1].abs().max()) > 0.0
    assert same_bits(res[False][-1], res[False][0]) and not same_bits(res[True][-1], res[True][0])
    assert float((res[True][-1] - res[True][0]).abs().max()) <= 2.0 ** -8 * float(torch.stack(maps).abs().max()) * 1.001


def test_pinned_refusals_with_real_tensors(dev):
    import ctypes as C
    from selfpose3d_amd import _lib
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer
    lib = _lib.load()
    NHWC, PLANAR, H16 = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR, _lib.HM_BF16_IN
    B, V, h, w = 1, 2, 8, 8
    cam = torch.from_numpy(pack_cameras(syn.make_meta(B, V, [32, 32]), B, [32, 32])).to(dev)
    maps = torch.rand((V, 1 << 16), device=dev)                       # each view: room for any (h, w, Jp) read below
    views = (C.c_void_p * V)(*[maps[c].data_ptr() for c in range(V)])
    centers = torch.tensor([syn.SPACE_CENTER], dtype=F32, device=dev)
    valid = torch.ones(1, dtype=torch.uint8, device=dev)
    res = torch.full((2, 1 << 21), float("nan"), device=dev)
    gs = (C.c_float * 3)(*[float(v) for v in syn.SPACE_SIZE])

    def call(layout, jp, J, grids=None):
        return lib.sp3d_unproject_fwd(views, layout, jp, cam.data_ptr(), centers.data_ptr(), valid.data_ptr(), res[0].data_ptr(), grids,
                                      B, V, J, h, w, 8, 8, 20, gs, 32, 32, None)
    cases = ((_lib.OUT_ZSPECTRUM, NHWC, 16, 15), (_lib.HM_ONE_CHANNEL, PLANAR, 15, 1), (_lib.HM_ONE_ZSPECTRUM, PLANAR, 15, 1))
    for flag, layout, jp, J in cases:
        for other in (_lib.HM_BF16, _lib.OUT_BF16):
            assert call(layout | flag | other, jp, J) == -4 and call(layout | flag | other | H16, jp, J) == -4, (hex(flag), hex(other))
    for layout, jp, J in ((NHWC, 16, 15), (PLANAR, 15, 15)):
        assert call(layout | H16, jp, J) == -4 and call(layout | H16, jp, J, res[1].data_ptr()) == -4      # the flag on its own
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(res).all()), "a refused call wrote to its result"
    for flag, layout, jp, J in cases:                                  # ... and each of the three runs with the new bit alone
        assert call(layout | flag | H16, jp, J) == 0, hex(flag)
    torch.cuda.synchronize(dev)
    cfg = load_config(None, NETWORK__IMAGE_SIZE=[96, 72], NETWORK__HEATMAP_SIZE=[24, 18])
    layer = ProjectLayer(cfg, io_dtype=BF)
    meta = syn.make_meta(2, 3, [96, 72])
    one = [x[:, 2:3] for x in (h.to(dev) for h in syn.random_heatmaps(2, 3, 15, 18, 24, seed=3))]
    with torch.no_grad(), pytest.raises(_lib.Sp3dError):
        layer.get_voxel(one, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])
    layer.bf16_maps = True
    with torch.no_grad(), pytest.raises(_lib.Sp3dError):
        layer.get_voxel(one, meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])
