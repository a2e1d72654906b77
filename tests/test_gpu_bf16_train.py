"""Training through bf16 heat-maps (SP3D_HM_BF16_TRAIN; ``ProjectLayer.bf16_train``, ``use_bf16_training()``, default off).  The
plans, the refusals and the routes are pinned on the host by tests/test_bf16_train_host.py; this file holds the values.

Every comparison is BITWISE (the raw words, a NaN equal to a NaN) unless it says otherwise, and the referee is always the fp32
training forward (or the switched-off layer) on the same values, which the older tests pin to the oracle.  The scenes are those of
tests/test_gpu_bf16_front.py: maps uniform in [-0.7, 1.7) so that the clamp mask acts, one NaN pixel, 18 x 24 pixels, 3 views.

1. the packed training forward on bf16 pixels against the same call on the widened pixels: cubes, grids, mask words, nothing
   written outside the three results; Jp = 16 and the two-plane mask at Jp = 32;
2. the one-channel training forward on odd and even channels of planar and channels-last bf16 tensors against the widened
   tensors, and its mask words against the packed bf16 forward's bit for that channel;
3. the layer, switch off against switch on, deterministic scatter: the same cubes, a bf16 ``.grad`` with the same bits, and the
   route counted (no widened copy, no fp32 pack);
4. the fp32-atomic scatter: every element within one bf16 ulp (2^-7 |d|) of the deterministic element d - the upstream gradient
   is positive and the tap weights are non-negative, so nothing cancels, the fp32 summation error is at most (taps per pixel)
   x 2^-24 relative, far below the 2^-8 half-step of bf16, and the one rounding can therefore move by one step at most;
5. the rounding bound against the maps before rounding, max |cubes(bf16) - cubes(raw)| <= 2^-8 max |hm| x 1.001 (derived in
   tests/test_gpu_bf16_front.py);
6. CuboidProposalNet and PoseRegressionNet.forward_slots in train mode on bf16 leaves, off against on;
7. the fall-backs (today's route, bit for bit) and the refusals with real tensors (a refused call writes nothing)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_bf16_front import classify, guarded, guards_untouched, one_sources, same_bits, scene

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
HW, V = (18, 24), 3
MODES = [dict(B=1), dict(B=3, valid=(1, 0, 1)), dict(B=2, P=4)]
CUBES = [(5, 7, 3), (8, 12, 20), (8, 8, 32)]         # a ragged 64-voxel tile (N = 105), the pipe form, brick stacks
SENTINEL = 0x5a5a


@pytest.fixture(scope="module")
def dev():
    from selfpose3d_amd import _lib
    assert hasattr(_lib, "HM_BF16_TRAIN"), "a library without the flag would launch on half-sized buffers"
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def words(mask):
    return mask.to(torch.int32) & 0xffff


def guarded_mask(n, dev):
    """an int16 buffer of sentinel words with ``n`` words in the middle for a pass mask"""
    buf = torch.full((n + 2 * 4096,), SENTINEL, dtype=torch.int16, device=dev)
    return buf, buf[4096:4096 + n]


def mask_guards_untouched(buf, n):
    return bool((buf[:4096] == SENTINEL).all()) and bool((buf[4096 + n:] == SENTINEL).all())


def train_fwd_guarded(s, maps, jp, J, cube, flags=0):
    """sp3d_unproject_fwd_train straight through the C entry into guarded cubes, grids and mask: the flag from the maps' type"""
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    nv, _, h, w, _ = maps.shape
    P, N = s["n"], X * Y * Z
    planes = 2 if flags & _lib.HM_WIDE_MASK else 1
    cl = bool(flags & _lib.OUT_CHANNELS_LAST)
    cb, co, cn, cubes = guarded((P, X, Y, Z, J) if cl else (P, J, X, Y, Z), maps.device)
    gb, go, gn, grids = guarded((P, N, 3), maps.device)
    mb, mask = guarded_mask(planes * P * N, maps.device)
    cam, centers, valid = s["args"]
    word = _lib.LAYOUT_NHWC | flags | (_lib.HM_BF16_TRAIN if maps.dtype == BF else 0)
    rc = _lib.load().sp3d_unproject_fwd_train(_lib._ptr_array([maps[c] for c in range(nv)]), word, jp, cam.data_ptr(),
                                             _lib._opt(s["sample_of"]), centers.data_ptr(), valid.data_ptr(), cubes.data_ptr(),
                                             grids.data_ptr(), mask.data_ptr(), P, nv, J, h, w, X, Y, Z, _lib._f3(s["grid_size"]),
                                             s["img"][0], s["img"][1], _lib._stream(maps.device))
    _lib.check(rc, "sp3d_unproject_fwd_train")
    torch.cuda.synchronize(maps.device)
    clean = guards_untouched(cb, co, cn) and guards_untouched(gb, go, gn) and mask_guards_untouched(mb, planes * P * N)
    return cubes, grids, mask.view(planes, P, N), clean


def train_fwd(s, maps, jp, J, cube, wide_mask=False, channels_last=False, grids=True):
    """the binding: the flag is derived from the views' type"""
    from selfpose3d_amd import _lib
    X, Y, Z = cube
    nv, _, h, w, _ = maps.shape
    P = s["n"]
    mask = torch.full(((2,) if wide_mask else ()) + (P, X * Y * Z), SENTINEL, dtype=torch.int16, device=maps.device)
    cubes, g = _lib.unproject_fwd([maps[c] for c in range(nv)], _lib.LAYOUT_NHWC, jp, *s["args"], P, J, h, w, cube, s["grid_size"], s["img"],
                                  grids, channels_last=channels_last, sample_of=s["sample_of"], pass_mask=mask, wide_mask=wide_mask)
    return cubes, g, mask


# ---- 1. the packed training forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cube", CUBES)
def test_packed_training_forward_at_jp16(dev, cube):
    from selfpose3d_amd import _lib
    for mi, mode in enumerate(MODES):
        s = scene(dev, mode["B"], V, HW, 16, 500 + mi, P=mode.get("P"), valid=mode.get("valid"))
        forms = [(J, 0) for J in (13, 15, 16)] + [(16, _lib.OUT_CHANNELS_LAST)]
        for J, cl in forms:
            tag = (cube, mode, J, cl)
            got = train_fwd_guarded(s, s["bf"], 16, J, cube, cl)
            ref = train_fwd_guarded(s, s["wide"], 16, J, cube, cl)
            assert got[3] and ref[3], (tag, "a store outside the results")
            assert got[0].dtype == F32 and same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]), tag
            assert torch.equal(got[2], ref[2]), tag
            m = words(got[2][0])
            assert not bool((m >> J).any()) and bool(m.any()) and bool((m != (1 << J) - 1).any()), tag      # the clamp mask acts
            assert float(torch.nan_to_num(got[0]).abs().max()) > 0.0
            if mode.get("valid") is not None:
                assert not bool(got[0][1].any()) and not bool(got[2][0, 1].any()) and not bool(got[1][1].any())
            # the binding, with and without grids
            for grids in (True, False):
                c, g, mk = train_fwd(s, s["bf"], 16, J, cube, channels_last=bool(cl), grids=grids)
                assert c.stride() == (got[0].permute(0, 4, 1, 2, 3) if cl else got[0]).stride()
                assert same_bits(c, got[0].permute(0, 4, 1, 2, 3) if cl else got[0]) and torch.equal(mk, got[2][0]), (tag, grids)
                assert (g is None) if not grids else same_bits(g, got[1])


@pytest.mark.parametrize("cube", CUBES)
def test_packed_training_forward_with_the_wide_mask(dev, cube):
    from selfpose3d_amd import _lib
    W = _lib.HM_WIDE_MASK
    for mi, mode in enumerate(MODES):
        s = scene(dev, mode["B"], V, HW, 32, 520 + mi, P=mode.get("P"), valid=mode.get("valid"))
        for J in (16, 17, 21, 32):
            tag = (cube, mode, J)
            got = train_fwd_guarded(s, s["bf"], 32, J, cube, W)
            ref = train_fwd_guarded(s, s["wide"], 32, J, cube, W)
            assert got[3] and ref[3], (tag, "a store outside the results")
            assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]) and torch.equal(got[2], ref[2]), tag
            m0, m1 = words(got[2][0]), words(got[2][1])
            assert bool(m0.any()) and bool((m0 != 0xffff).any())
            if J == 16:
                assert not bool(m1.any()), (tag, "plane 1 is not zeros")
            else:
                assert not bool((m1 >> (J - 16)).any()) and bool(m1.any()), tag
            if mode.get("valid") is not None:
                assert not bool(got[0][1].any()) and not bool(got[2][:, 1].any())
            c, g, mk = train_fwd(s, s["bf"], 32, J, cube, wide_mask=True)
            assert same_bits(c, got[0]) and same_bits(g, got[1]) and torch.equal(mk, got[2]), tag


# ---- 2. the one-channel training forward --------------------------------------------------------------------------------------
CHANNEL = {"planar2": 2, "planar7": 7, "nhwc16_4": 4, "nhwc16_5": 5, "nhwc32_19": 19, "contiguous": 3}


@pytest.mark.parametrize("nv", [3, 7])
def test_one_channel_training_forward(dev, nv):
    from selfpose3d_amd import _lib
    cube = (5, 7, 3)
    X, Y, Z = cube
    h, w = HW
    for mi, mode in enumerate(MODES):
        s = scene(dev, mode["B"], nv, HW, 32, 540 + 10 * nv + mi, P=mode.get("P"), valid=mode.get("valid"))
        P, so = s["n"], s["sample_of"]
        # the packed bf16 training forwards over the same pixels: bit j of plane j / 16 is channel j's word
        _, _, packed = train_fwd(s, s["bf"], 32, 32, cube, wide_mask=True, grids=False)
        _, _, packed16 = train_fwd(s, s["bf"][..., :16].contiguous(), 16, 16, cube, grids=False)
        assert torch.equal(packed16, packed[0])
        for name, bf, wide in one_sources(s):
            layout, jp = classify(bf, BF)
            assert (layout, jp) == classify(wide, F32) and bf[0].data_ptr() % 2 == 0

            def run(views, J, cl):
                mask = torch.full((P, X * Y * Z), SENTINEL, dtype=torch.int16, device=dev)
                c, g = _lib.unproject_one_fwd_train(views, layout, jp, *s["args"], P, J, h, w, cube, s["grid_size"], s["img"], mask,
                                                    want_grids=True, channels_last=cl, sample_of=so)
                return c, g, mask
            ch = CHANNEL[name]
            want = (words(packed[ch // 16]) >> (ch % 16)) & 1
            for J, cl in ((1, False), (4, False), (4, True)):
                got, ref = run(bf, J, cl), run(wide, J, cl)
                tag = (nv, mode, name, J, cl)
                assert got[0].dtype == F32 and tuple(got[0].shape) == (P, J, X, Y, Z) and got[0].stride() == ref[0].stride(), tag
                assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1]) and torch.equal(got[2], ref[2]), tag
                assert torch.equal(words(got[2]), want), (tag, "the words are not the packed forward's for this channel")
                assert not cl or got[0].is_contiguous(memory_format=torch.channels_last_3d)
            assert bool(want.any()) and not bool(want.all())
    # a mixture of types is refused by the binding
    mixed = [bf[0], wide[1]] + list(bf[2:])
    with pytest.raises(_lib.Sp3dError, match="mixture"):
        _lib.unproject_one_fwd_train(mixed, layout, jp, *s["args"], P, 1, h, w, cube, s["grid_size"], s["img"],
                                     torch.zeros((P, X * Y * Z), dtype=torch.int16, device=dev))


# ---- 3. and 4. the layer ------------------------------------------------------------------------------------------------------
class _Spy:
    """counts the forward launchers by the type of the views they get, the re-tiling pass by (input type, result type), and the
    widened copies (project_layer._fp32_maps)"""

    def __init__(self, monkeypatch):
        from selfpose3d_amd import _lib, project_layer
        self.n = {}
        for name in ("unproject_fwd", "unproject_one_fwd_train"):
            inner = getattr(_lib, name)

            def spy(views, *a, _inner=inner, _name=name, **k):
                self._count((_name, views[0].dtype))
                return _inner(views, *a, **k)
            monkeypatch.setattr(_lib, name, spy)
        pack = _lib.pack_heatmaps

        def pack_spy(hms, *a, **k):
            out = pack(hms, *a, **k)
            self._count(("pack_heatmaps", hms[0].dtype, out.dtype))
            return out
        monkeypatch.setattr(_lib, "pack_heatmaps", pack_spy)
        widen = project_layer._fp32_maps

        def widen_spy(hms):
            if any(x.dtype != F32 for x in hms):
                self._count(("widened",))
            return widen(hms)
        monkeypatch.setattr(project_layer, "_fp32_maps", widen_spy)

    def _count(self, key):
        self.n[key] = self.n.get(key, 0) + 1


def _layer(**switches):
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer
    cfg = load_config(None, NETWORK__IMAGE_SIZE=[4 * HW[1], 4 * HW[0]], NETWORK__HEATMAP_SIZE=[HW[1], HW[0]])
    layer = ProjectLayer(cfg)
    for k, v in switches.items():
        setattr(layer, k, v)
    return layer


def _leaf_maps(s, kind, J):
    """-> (leaves that collect a gradient, the list[V] of (B,J,h,w) bf16 maps handed to the layer)"""
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    nv = s["bf"].shape[0]
    if kind == "planar":
        leaves = [s["bf"][c, ..., :J].permute(0, 3, 1, 2).contiguous().requires_grad_(True) for c in range(nv)]
        return leaves, leaves
    if kind == "producer":                       # ONE (V,B,h,w,16|32) bf16 buffer, the maps being its channels-last views
        buf = s["bf"].clone()
        buf[..., J:] = 0
        buf.requires_grad_(True)
        return [buf], nhwc_heatmap_views(buf, J)
    assert kind == "slice" and J == 1            # channel 7 of planar (B,15,h,w) tensors
    leaves = [s["bf"][c, ..., :15].permute(0, 3, 1, 2).contiguous().requires_grad_(True) for c in range(nv)]
    return leaves, [a[:, 7:8] for a in leaves]


# Today's route packs fp32 pixels: with the pack cache (the default) straight from the bf16 planes, a re-tile that exists at 16
# and 32 channels only; without it (``cache_packs = False``, as under ``static_camera_table``) from the widened copies of
# ``_fp32_maps``, at any width.  One joint is a pixel of 4 channels, so the one-channel case compares with the cache off (with it
# on, today's route raises: test_fallbacks_equal_todays_result).
LAYER_CASES = [  # (id, J, kind, switches besides bf16_train, route when on)
    ("15 joints", 15, "planar", {}, {("pack_heatmaps", BF, BF): 1, ("unproject_fwd", BF): 1}),
    ("15 joints, no pack cache", 15, "planar", dict(cache_packs=False), {("pack_heatmaps", BF, BF): 1, ("unproject_fwd", BF): 1}),
    ("15 joints, producer buffer", 15, "producer", {}, {("unproject_fwd", BF): 1}),
    ("17 joints", 17, "planar", dict(wide_grad=True), {("pack_heatmaps", BF, BF): 1, ("unproject_fwd", BF): 1}),
    ("17 joints, producer buffer", 17, "producer", dict(wide_grad=True), {("unproject_fwd", BF): 1}),
    ("one channel", 1, "slice", dict(one_channel_grad=True, cache_packs=False), {("unproject_one_fwd_train", BF): 1}),
]


def _fp32_route(route):
    """the switched-off route: a fp32 pack, fp32 pixels into the training forward"""
    return ("unproject_fwd", F32) in route and any(k[0] == "pack_heatmaps" and k[2] == F32 for k in route) and \
        not any(k[0] in ("unproject_fwd", "unproject_one_fwd_train") and k[1] == BF for k in route)


def _layer_run(s, layer, J, kind, cube, sample_of, spy, form=None):
    from selfpose3d_amd.project_layer import clear_pack_cache
    clear_pack_cache()
    spy.n = {}
    leaves, maps = _leaf_maps(s, kind, J)
    centers = s["args"][1] if sample_of else [list(s["args"][1][0].tolist())]
    with torch.enable_grad():
        cubes, grids = layer.get_voxel(maps, s["meta"], s["grid_size"], centers, list(cube), sample_of=s["sample_of"] if sample_of else None,
                                       **(form or {}))
        route = dict(spy.n)
        up = torch.linspace(0.5, 1.5, cubes.numel(), device=cubes.device).view(cubes.shape)
        cubes.backward(up)
    clear_pack_cache()
    return cubes.detach(), grids, [a.grad for a in leaves], route


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_layer_switch_on_equals_off(dev, monkeypatch, case):
    _, J, kind, switches, route_on = case
    spy = _Spy(monkeypatch)
    C_ = 32 if J > 16 else 16
    for cube, sample_of in (((8, 12, 20), False), ((5, 7, 3), True), ((8, 8, 32), False)):
        s = scene(dev, 2, V, HW, C_, 560 + J, P=4 if sample_of else None)
        forms = [None] if J > 16 else [None, dict(want_grids=False, pad_channels=True, channels_last=True)]
        for form in forms:
            got = {}
            for on in (False, True):
                layer = _layer(bf16_train=on, deterministic_backward=True, **switches)
                got[on] = _layer_run(s, layer, J, kind, cube, sample_of, spy, form)
            tag = (case[0], cube, sample_of, form)
            # switched on: no widened copy, no fp32 pack (a producer's buffer: no pack at all)
            assert got[True][3] == route_on and _fp32_route(got[False][3]), (tag, got[True][3], got[False][3])
            assert got[True][0].dtype == F32 and got[True][0].stride() == got[False][0].stride() and same_bits(got[True][0], got[False][0]), tag
            assert (got[True][1] is None) == (got[False][1] is None) and (got[True][1] is None or same_bits(got[True][1], got[False][1])), tag
            for a, b in zip(got[True][2], got[False][2]):
                assert a.dtype == BF and b.dtype == BF and a.shape == b.shape and same_bits(a.float(), b.float()), tag
                assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0.0, tag
            if kind == "slice":                      # nothing outside the one channel
                for a in got[True][2]:
                    rest = a.clone()
                    rest[:, 7] = 0
                    assert not bool(rest.any()), tag


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_fp32_atomic_scatter_within_one_bf16_step(dev, monkeypatch, case):
    _, J, kind, switches, _ = case
    spy = _Spy(monkeypatch)
    C_ = 32 if J > 16 else 16
    for cube, sample_of in (((8, 12, 20), False), ((8, 8, 32), True)):
        s = scene(dev, 2, V, HW, C_, 560 + J, P=4 if sample_of else None)
        det = _layer_run(s, _layer(bf16_train=True, deterministic_backward=True, **switches), J, kind, cube, sample_of, spy)
        atm = _layer_run(s, _layer(bf16_train=True, deterministic_backward=False, **switches), J, kind, cube, sample_of, spy)
        assert same_bits(det[0], atm[0])
        worst = 0.0
        for a, d in zip(atm[2], det[2]):
            assert a.dtype == BF and d.dtype == BF
            a, d = a.float(), d.float()
            assert bool(torch.isfinite(a).all()) and float(d.abs().max()) > 0.0
            excess = (a - d).abs() - 2.0 ** -7 * d.abs()
            worst = max(worst, float(((a - d).abs() / d.abs().clamp_min(1e-30)).max()) if bool((d != 0).any()) else 0.0)
            assert bool((excess <= 0).all()), (case[0], cube, float(excess.max()))
        print("fp32-atomic against deterministic, %s %s: worst relative step %.3g (bound 2^-7 = %.3g)" % (case[0], cube, worst, 2.0 ** -7))


# ---- 5. the rounding bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cube", CUBES)
def test_rounding_bound_against_the_unrounded_maps(dev, cube):
    from selfpose3d_amd import _lib
    for jp, J, wide in ((16, 15, False), (32, 21, True)):
        s = scene(dev, 2, V, HW, jp, 580 + jp, nan=False)
        a, _, ma = train_fwd(s, s["bf"], jp, J, cube, wide_mask=wide, grids=False)
        b, _, mb = train_fwd(s, s["raw"], jp, J, cube, wide_mask=wide, grids=False)
        d = float((a - b).abs().max())
        print("bf16 maps against the maps before rounding, Jp %d %s: max |d cubes| %.4g (bound %.4g)" % (jp, cube, d, 2.0 ** -8 * s["hmax"] * 1.001))
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0
        assert d <= 2.0 ** -8 * s["hmax"] * 1.001, (jp, cube, d)
    s = scene(dev, 2, V, HW, 32, 580 + 32, nan=False)
    h, w = HW
    X, Y, Z = cube
    bf = [s["bf"][c].permute(0, 3, 1, 2)[:, 19:20] for c in range(V)]
    raw = [s["raw"][c].permute(0, 3, 1, 2)[:, 19:20] for c in range(V)]
    res = []
    for views, dt in ((bf, BF), (raw, F32)):
        mask = torch.empty((2, X * Y * Z), dtype=torch.int16, device=dev)
        res.append(_lib.unproject_one_fwd_train(views, *classify(views, dt), *s["args"], 2, 1, h, w, cube, s["grid_size"], s["img"], mask,
                                                want_grids=False)[0])
    assert float(res[0].abs().max()) > 0.0 and float((res[0] - res[1]).abs().max()) <= 2.0 ** -8 * s["hmax"] * 1.001


# ---- 6. the nets --------------------------------------------------------------------------------------------------------------
def test_root_net_trains_switch_on_equals_off(dev, monkeypatch):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.project_layer import clear_pack_cache
    img, hm, J, B, nv = (96, 72), (24, 18), 15, 2, 3
    cfg = load_config(None, NETWORK__IMAGE_SIZE=list(img), NETWORK__HEATMAP_SIZE=list(hm), MULTI_PERSON__INITIAL_CUBE_SIZE=[24, 24, 8])
    assert not bool(cfg.NETWORK.ROOTNET_ROOTHM) and int(cfg.NETWORK.NUM_JOINTS) == J
    net = CuboidProposalNet(cfg)
    syn.fill_parameters_deterministic(net, seed=5, scale=0.05)
    net.to(dev).train()
    net.project_layer.deterministic_backward = True
    meta = syn.make_meta(B, nv, list(img))
    base = [h.to(dev).to(BF) for h in syn.people_heatmaps(B, nv, J, hm[1], hm[0], img, seed=41)[0]]
    w = torch.from_numpy(np.random.default_rng(4).standard_normal((B, 24, 24, 8)).astype(np.float32)).to(dev)
    spy = _Spy(monkeypatch)
    got = {}
    for on in (False, True):
        assert net.use_bf16_training(on) is net
        net.zero_grad(set_to_none=True)
        clear_pack_cache()
        spy.n = {}
        leaves = [a.clone().requires_grad_(True) for a in base]
        root_cubes = net(leaves, meta)[0]
        route = dict(spy.n)
        (root_cubes * w).sum().backward()
        got[on] = (root_cubes.detach().clone(), [a.grad for a in leaves], route)
    net.use_bf16_training(False)
    assert got[True][2] == {("pack_heatmaps", BF, BF): 1, ("unproject_fwd", BF): 1}, got[True][2]
    assert _fp32_route(got[False][2]), got[False][2]
    assert same_bits(got[True][0], got[False][0]) and bool(torch.isfinite(got[True][0]).all())
    for a, b in zip(got[True][1], got[False][1]):
        assert a.dtype == BF and b.dtype == BF and same_bits(a.float(), b.float()) and float(a.float().abs().max()) > 0.0


@pytest.mark.miopen_sensitive            # the same cubes go through the library's convolutions twice: collected last
def test_pose_net_forward_slots_switch_on_equals_off(dev, monkeypatch):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.pose_regression_net import PoseRegressionNet
    from selfpose3d_amd.project_layer import clear_pack_cache
    B, nv, J, img, hm = 2, 3, 15, (128, 96), (32, 24)
    cfg = load_config(None, NETWORK__IMAGE_SIZE=list(img), NETWORK__HEATMAP_SIZE=list(hm), NETWORK__NUM_JOINTS=J,
                      PICT_STRUCT__CUBE_SIZE=[16, 16, 16])
    gc = torch.zeros(B, 2, 5, device=dev)                       # two slots: both valid in sample 0, the first in sample 1
    gc[0, :, :3] = torch.tensor([[0.0, -500.0, 900.0], [600.0, -900.0, 800.0]], device=dev)
    gc[1, :, :3] = torch.tensor([[300.0, -300.0, 850.0], [0.0, 0.0, 0.0]], device=dev)
    gc[:, :, 3] = torch.tensor([[0.0, 1.0], [0.0, -1.0]], device=dev)
    meta = syn.make_meta(B, nv, img)
    base = [h.to(dev).to(BF) for h in syn.people_heatmaps(B, nv, J, hm[1], hm[0], img, seed=21)[0]]
    wgt = torch.randn(B, 2, J, 3, generator=torch.Generator().manual_seed(9)).to(dev)
    spy = _Spy(monkeypatch)
    got = {}
    for on in (False, True):
        net = PoseRegressionNet(cfg)                            # a fresh net each: the running statistics start equal
        syn.fill_parameters_deterministic(net, seed=5, scale=0.08)
        net.to(dev).train().use_channels_last(True)
        net.project_layer.deterministic_backward = True
        assert net.use_bf16_training(on) is net and net.can_batch_slots()
        clear_pack_cache()
        spy.n = {}
        leaves = [a.clone().requires_grad_(True) for a in base]
        pred = net.forward_slots([(leaves, meta, None)], gc)[0]
        route = dict(spy.n)
        (pred * wgt).sum().backward()
        got[on] = (pred.detach().clone(), [a.grad for a in leaves], route)
    assert got[True][2] == {("pack_heatmaps", BF, BF): 1, ("unproject_fwd", BF): 1}, got[True][2]
    assert _fp32_route(got[False][2]), got[False][2]
    assert got[True][0].dtype == F32 and tuple(got[True][0].shape) == (B, 2, J, 3)
    assert same_bits(got[True][0], got[False][0]) and bool(torch.isfinite(got[True][0]).all())
    assert not bool(got[True][0][1, 1].any()) and float(got[True][0][0].abs().max()) > 0.0
    for a, b in zip(got[True][1], got[False][1]):
        assert a.dtype == BF and b.dtype == BF and same_bits(a.float(), b.float()) and float(a.float().abs().max()) > 0.0


# ---- 7. fall-backs and refusals -----------------------------------------------------------------------------------------------
def test_fallbacks_equal_todays_result(dev, monkeypatch):
    spy = _Spy(monkeypatch)
    cube = (8, 12, 20)
    s16, s32 = scene(dev, 2, V, HW, 16, 600), scene(dev, 2, V, HW, 32, 601)

    def planar(s, J, dtype):
        return [s["wide"][c, ..., :J].permute(0, 3, 1, 2).contiguous().to(dtype).requires_grad_(True) for c in range(V)]

    def run(layer, hms, s):
        from selfpose3d_amd.project_layer import clear_pack_cache
        clear_pack_cache()
        spy.n = {}
        with torch.enable_grad():
            cubes, grids = layer.get_voxel(hms, s["meta"], s["grid_size"], [list(s["args"][1][0].tolist())], list(cube))
            cubes.backward(torch.linspace(0.5, 1.5, cubes.numel(), device=dev).view(cubes.shape))
        clear_pack_cache()
        return cubes.detach(), grids, [a.grad for a in hms], dict(spy.n)
    for name, s, J, dtype, switches in (("4 joints", s16, 4, BF, dict(cache_packs=False)), ("fp32 maps", s16, 15, F32, dict(bf16_maps=True)),
                                        ("fp32 maps, 4 joints", s16, 4, F32, {}), ("17 joints without wide_grad", s32, 17, BF, {})):
        off = run(_layer(deterministic_backward=True, **switches), planar(s, J, dtype), s)
        on = run(_layer(bf16_train=True, deterministic_backward=True, **switches), planar(s, J, dtype), s)
        assert on[3] == off[3] and ("unproject_fwd", BF) not in on[3], (name, on[3], off[3])
        assert same_bits(on[0], off[0]) and same_bits(on[1], off[1]), name
        for a, b in zip(on[2], off[2]):
            assert a.dtype == dtype and b.dtype == dtype and same_bits(a.float(), b.float()) and float(a.float().abs().max()) > 0.0, name
    # 4 bf16 joints with the pack cache on: there is no re-tile from bf16 planes into fp32 pixels of 4 channels, today's route
    # raises, and the switch leaves that as it is (fewer than 13 joints are none of its business)
    from selfpose3d_amd import _lib
    for on in (False, True):
        with pytest.raises(_lib.Sp3dError, match="sp3d_pack_heatmaps"):
            run(_layer(bf16_train=on, deterministic_backward=True), planar(s16, 4, BF), s16)


def test_refusals_with_real_tensors(dev):
    from selfpose3d_amd import _lib
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    lib = _lib.load()
    NHWC, PLANAR, T, W = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR, _lib.HM_BF16_TRAIN, _lib.HM_WIDE_MASK
    B, nv, h, w = 1, 2, 8, 8
    cam = torch.from_numpy(pack_cameras(syn.make_meta(B, nv, [32, 32]), B, [32, 32])).to(dev)
    maps = torch.rand((nv, 1 << 16), device=dev)                      # each view: room for any (h, w, Jp) read below
    views = (C.c_void_p * nv)(*[maps[c].data_ptr() for c in range(nv)])
    centers = torch.tensor([syn.SPACE_CENTER], dtype=F32, device=dev)
    valid = torch.ones(1, dtype=torch.uint8, device=dev)
    res = torch.full((2, 1 << 21), float("nan"), device=dev)
    mask = torch.full((1 << 16,), SENTINEL, dtype=torch.int16, device=dev)
    gs = (C.c_float * 3)(*[float(v) for v in syn.SPACE_SIZE])
    st = (C.c_int64 * 4)(32 * 1280, 1280, 160, 20)
    tail = lambda J, hw=(h, w): (B, nv, J, hw[0], hw[1], 8, 8, 20, gs, 32, 32, None)
    ptrs = (cam.data_ptr(), centers.data_ptr(), valid.data_ptr(), res[0].data_ptr())
    fwd = lambda layout, jp, J: lib.sp3d_unproject_fwd(views, layout, jp, *ptrs, res[1].data_ptr(), *tail(J))
    indexed = lambda layout, jp, J: lib.sp3d_unproject_fwd_indexed(views, layout, jp, ptrs[0], None, *ptrs[1:], res[1].data_ptr(), *tail(J))
    strided = lambda layout, jp, J: lib.sp3d_unproject_fwd_strided(views, layout, jp, ptrs[0], None, *ptrs[1:], st, *tail(J))
    train = lambda layout, jp, J, hw=(h, w): lib.sp3d_unproject_fwd_train(views, layout, jp, ptrs[0], None, *ptrs[1:], res[1].data_ptr(),
                                                                         mask.data_ptr(), *tail(J, hw))
    one_train = lambda layout, jp, J, hw=(h, w): lib.sp3d_unproject_one_fwd_train(views, layout, jp, ptrs[0], None, *ptrs[1:], res[1].data_ptr(),
                                                                                 mask.data_ptr(), *tail(J, hw))
    for f in (fwd, indexed, strided):
        for layout, jp, J in ((NHWC, 16, 15), (NHWC | W, 32, 21), (NHWC, 4, 4), (PLANAR, 15, 15), (PLANAR | _lib.HM_ONE_CHANNEL, 15, 1),
                              (NHWC | _lib.HM_ONE_CHANNEL, 16, 4), (NHWC | _lib.OUT_CHANNELS_LAST, 16, 16)):
            assert f(layout | T, jp, J) == -4, (hex(layout), jp, J)
    for other in (_lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16_IN, _lib.OUT_ZSPECTRUM, _lib.HM_ONE_ZSPECTRUM):
        assert train(NHWC | T | other, 16, 15) == -4 and train(NHWC | T | W | other, 32, 21) == -4, hex(other)
        assert one_train(PLANAR | T | other, 15, 1) == -4 and one_train(NHWC | T | other, 16, 4) == -4, hex(other)
    assert train(PLANAR | T, 15, 15) == -4 and train(NHWC | T, 32, 17) == -4 and train(NHWC | T | W, 16, 15) == -4
    for jp in (4, 8, 12):
        assert train(NHWC | T, jp, jp) == -4
    assert train(NHWC | T | _lib.HM_ONE_CHANNEL, 16, 1) == -4 and train(PLANAR | T | _lib.HM_ONE_CHANNEL, 15, 1) == -4
    assert train(NHWC | T | W | _lib.OUT_CHANNELS_LAST, 32, 20) == -4 and train(NHWC | T | _lib.OUT_CHANNELS_LAST, 16, 15) == -4
    for hw in ((8, 1), (1, 8)):
        assert train(NHWC | T, 16, 15, hw) == -4 and train(NHWC | T | W, 32, 21, hw) == -4 and one_train(PLANAR | T, 15, 1, hw) == -4
    assert one_train(PLANAR | T, 15, 2) == -4 and one_train(PLANAR | T | _lib.OUT_CHANNELS_LAST, 15, 1) == -4
    assert train(NHWC | _lib.HM_BF16_IN, 16, 15) == -4 and one_train(PLANAR | _lib.HM_BF16_IN, 15, 1) == -4      # as pinned before
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(res).all()) and bool((mask == SENTINEL).all()), "a refused call wrote to a result"
    # ... and each supported form runs with the bit
    assert train(NHWC | T, 16, 15) == 0 and train(NHWC | T | W, 32, 21) == 0 and train(NHWC | T | _lib.OUT_CHANNELS_LAST, 16, 16) == 0
    assert one_train(PLANAR | T, 15, 1) == 0 and one_train(NHWC | T | _lib.OUT_CHANNELS_LAST, 16, 4) == 0
    torch.cuda.synchronize(dev)
