"""Training through bf16 heat-maps (SP3D_HM_BF16_TRAIN, ``ProjectLayer.bf16_train``, ``use_bf16_training()``) without a GPU: the
flag, the launches resolve_fwd plans for it on the two training entries (sp3d_unproject_fwd_plan) - the bf16-tap kernels with the
geometry of the fp32 training plan -, every refusal the header lists - through the plan, and through the C entries with pointers
that are never dereferenced -, and the routes of the layer on CPU tensors.  tests/test_gpu_bf16_train.py holds the values."""
import ctypes as C
import os
import re

import pytest
import torch

from selfpose3d_amd import _lib, build as sbuild
from selfpose3d_amd.config import load_config
from selfpose3d_amd.project_layer import ProjectLayer, Route, nhwc_heatmap_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NHWC, PLANAR = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
EUNSUPPORTED = -4
BF, F32 = torch.bfloat16, torch.float32
# what a launch's geometry is made of: everything of a plan record but the kernel, its LDS and the two byte offsets
GEOMETRY = [f for f in _lib.PLAN_FIELDS if f not in ("lds", "view_off", "out_off")]


def test_flag_abi_version_and_entry_list():
    """fails on a library and binding without the flag with an AttributeError, before anything is launched"""
    T16 = _lib.HM_BF16_TRAIN
    from tests.test_glue_sweep_reference import LEDGER, _header_signatures
    with open(os.path.join(ROOT, "include", "sp3d.h")) as fh:
        hdr = fh.read()
    assert int(re.search(r"\bSP3D_HM_BF16_TRAIN\s*=\s*(0x[0-9a-fA-F]+)", hdr).group(1), 0) == 0x10000 == T16
    assert "SP3D_ABI_VERSION 3" in hdr and _lib.ABI_VERSION == 3
    # a flag bit, not a symbol: the header declares what the ledger lists, no more
    assert sorted(_header_signatures(os.path.join(ROOT, "include", "sp3d.h"))) == sorted(LEDGER)
    assert len(_lib.SIGNATURES) == 57
    # the bit collides with no other bit of the layout word
    flags = dict((k, int(v, 0)) for k, v in re.findall(r"\b(SP3D_(?:HM|OUT)_[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+)", hdr))
    assert all(v & T16 == 0 for k, v in flags.items() if k != "SP3D_HM_BF16_TRAIN") and T16 & 0xff == 0


@pytest.fixture(scope="module")
def lib():
    assert hasattr(_lib, "HM_BF16_TRAIN")
    sbuild.build()
    return _lib.load()


def T16():
    return _lib.HM_BF16_TRAIN


def plan(flags, layout=NHWC, jp=16, J=15, entry="train", B=2, V=3, h=18, w=24, cube=(8, 12, 20), strides=None):
    return _lib.unproject_fwd_plan(entry, layout | flags, jp, B, V, J, h, w, cube, 0, strides)


# ---- the packed training forward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 4])
def test_train_plan_at_jp16(lib, B):
    forms = (((8, 12, 20), 0, "unproject_pipe_kernel<16, true, 1, false, bf16_t, float, 16>", "unproject_pipe_kernel<16, true, 1, false, float, float, 16>"),
             ((5, 7, 3), 0, "unproject_pipe_kernel<16, true, 1, false, bf16_t, float, 16>", "unproject_pipe_kernel<16, true, 1, false, float, float, 16>"),
             ((8, 8, 32), 0, "unproject_brick_h_kernel<false, float, 16>", "unproject_brick_kernel<16, false, float, float, false, 16>"),
             ((8, 12, 20), _lib.OUT_CHANNELS_LAST, "unproject_brick_h_kernel<true, float, 16>", "unproject_brick_kernel<16, true, float, float, false, 16>"))
    for cube, cl, name, ref_name in forms:
        for J in ((16,) if cl else (13, 15, 16)):
            rc, launches, tuning = plan(T16() | cl, jp=16, J=J, B=B, cube=cube)
            assert rc == 0 and len(launches) == 1, (rc, cube, cl, J)
            l = launches[0]
            assert l["name"] == name
            assert (l["view_off"], l["out_off"], l["grids"], l["J"]) == (0, 0, 1, J)
            rc, ref, ref_tuning = plan(cl, jp=16, J=J, B=B, cube=cube)
            assert rc == 0 and ref[0]["name"] == ref_name
            assert [l[f] for f in GEOMETRY] == [ref[0][f] for f in GEOMETRY]
            assert l["lds"] == ref[0]["lds"] and tuning == ref_tuning


@pytest.mark.parametrize("cube,name", [((8, 12, 20), "unproject_pipe_kernel<16, true, 1, false, bf16_t, float, 32>"),
                                       ((5, 7, 3), "unproject_pipe_kernel<16, true, 1, false, bf16_t, float, 32>"),
                                       ((8, 8, 32), "unproject_brick_h_kernel<false, float, 32>")])
@pytest.mark.parametrize("B", [1, 3, 4])
def test_train_plan_with_the_wide_mask(lib, cube, name, B):
    W = _lib.HM_WIDE_MASK
    X, Y, Z = cube
    for J in (17, 21, 32):
        rc, launches, _ = plan(T16() | W, jp=32, J=J, B=B, cube=cube)
        assert rc == 0 and [l["name"] for l in launches] == [name, name], (rc, J)
        rc, ref, _ = plan(W, jp=32, J=J, B=B, cube=cube)
        assert rc == 0 and len(ref) == 2
        # group 1 starts 16 bf16 channels = 32 bytes into the pixel, and 16 fp32 channel planes into the cubes
        assert [l["view_off"] for l in launches] == [0, 32] and [l["view_off"] for l in ref] == [0, 64]
        assert [l["out_off"] for l in launches] == [r["out_off"] for r in ref] == [0, 16 * X * Y * Z * 4]
        assert [l["J"] for l in launches] == [16, J - 16] and [l["grids"] for l in launches] == [1, 0]
        for l, r in zip(launches, ref):
            assert [l[f] for f in GEOMETRY] == [r[f] for f in GEOMETRY]
    for J in (1, 16):                                                              # no second group
        rc, launches, _ = plan(T16() | W, jp=32, J=J, B=B, cube=cube)
        assert rc == 0 and [(l["name"], l["view_off"], l["out_off"], l["J"]) for l in launches] == [(name, 0, 0, J)]
        ref = plan(W, jp=32, J=J, B=B, cube=cube)[1]
        assert [launches[0][f] for f in GEOMETRY] == [ref[0][f] for f in GEOMETRY]


# ---- the one-channel training forward -----------------------------------------------------------------------------------
LADDER = {3: (3, 4), 5: (5, 4), 7: (8, 4), 16: (16, 8)}


@pytest.mark.parametrize("V", [3, 5, 7, 16])
@pytest.mark.parametrize("layout,jp", [(PLANAR, 1), (PLANAR, 15), (NHWC, 16), (NHWC, 32)])
def test_one_channel_train_plans(lib, V, layout, jp):
    vt, cs = LADDER[V]
    h, w = 18, 24
    want = (h * w * jp, w * jp, jp) if layout == NHWC else (jp * h * w, w, 1)           # sample, row, pixel stride in ELEMENTS
    for J, cl, clname in ((1, 0, "false"), (4, 0, "false"), (4, _lib.OUT_CHANNELS_LAST, "true")):
        for B in (1, 3):
            rc, launches, _ = plan(T16() | cl, layout, jp, J, "one_train", B=B, V=V, cube=(5, 7, 3))
            assert rc == 0 and len(launches) == 1, (rc, J, cl)
            l = launches[0]
            assert l["name"] == "unproject_one_kernel<%d, %d, %s, true, bf16_t>" % (vt, cs, clname)
            assert (l["block"], l["lds"], l["view_off"], l["out_off"], l["J"]) == (64, 0, 0, 0, J)
            assert (l["nscalars"], l["s0"], l["s1"], l["s2"]) == (3,) + want
            rc, ref, _ = plan(cl, layout, jp, J, "one_train", B=B, V=V, cube=(5, 7, 3))
            assert rc == 0 and ref[0]["name"] == "unproject_one_kernel<%d, %d, %s, true>" % (vt, cs, clname)
            assert [l[f] for f in _lib.PLAN_FIELDS] == [ref[0][f] for f in _lib.PLAN_FIELDS]
            # SP3D_HM_ONE_CHANNEL is accepted and implied
            assert plan(T16() | cl | _lib.HM_ONE_CHANNEL, layout, jp, J, "one_train", B=B, V=V, cube=(5, 7, 3))[1] == launches


def test_one_channel_byte_limit_counts_two_byte_elements(lib):
    kw = dict(layout=NHWC, J=1, h=4096, w=4096, entry="one_train")
    assert plan(0, jp=31, **kw)[0] == 0 and plan(0, jp=33, **kw)[0] == EUNSUPPORTED                # fp32: 2^31 bytes at 32
    assert plan(T16(), jp=33, **kw)[0] == 0 and plan(T16(), jp=63, **kw)[0] == 0                   # bf16: at 64
    assert plan(T16(), jp=65, **kw)[0] == EUNSUPPORTED
    assert plan(T16(), layout=NHWC, jp=1 << 20, J=1, entry="one_train")[0] == EUNSUPPORTED         # a row of 2^24 elements
    for h, w in ((18, 1), (1, 24), (4097, 4096)):
        assert plan(T16(), layout=PLANAR, jp=15, J=1, h=h, w=w, entry="one_train")[0] == EUNSUPPORTED


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_plan_refusals(lib):
    t, W = T16(), _lib.HM_WIDE_MASK
    z, one, ozd, h16 = _lib.OUT_ZSPECTRUM, _lib.HM_ONE_CHANNEL, _lib.HM_ONE_ZSPECTRUM, _lib.HM_BF16_IN
    ok = (dict(flags=t, jp=16, J=15), dict(flags=t | W, jp=32, J=21), dict(flags=t, layout=PLANAR, jp=15, J=1, entry="one_train"),
          dict(flags=t, jp=16, J=4, entry="one_train"))
    for kw in ok:
        assert plan(**kw)[0] == 0, kw
    # every entry but the two training forwards
    sj = 8 * 12 * 20
    for entry in ("indexed", "strided", "zdft", "variant"):
        for kw in ok:
            assert plan(**dict(kw, entry=entry))[0] == EUNSUPPORTED, (entry, kw)
        assert plan(t | one, layout=PLANAR, jp=15, J=1, entry=entry)[0] == EUNSUPPORTED
    assert plan(t, jp=16, J=15, entry="strided", strides=(16 * sj, sj, 12 * 20, 20))[0] == EUNSUPPORTED
    assert plan(0, jp=16, J=15, entry="variant")[0] == 0 and plan(0, jp=16, J=15, entry="zdft")[0] == 0
    # next to the storage pair, the inference flag and either spectrum
    for other in (_lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16 | _lib.OUT_BF16, h16, z, ozd):
        for kw in ok:
            assert plan(**dict(kw, flags=kw["flags"] | other))[0] == EUNSUPPORTED, (hex(other), kw)
    # the packed training forward: planar maps, narrower pixels, 32-element pixels without the two-plane mask, one channel
    assert plan(t, layout=PLANAR, jp=15, J=15)[0] == EUNSUPPORTED and plan(t, layout=PLANAR, jp=1, J=1)[0] == EUNSUPPORTED
    for jp in (4, 8, 12):
        assert plan(t, jp=jp, J=jp)[0] == EUNSUPPORTED and plan(0, jp=jp, J=jp)[0] == 0
        assert plan(t | _lib.OUT_CHANNELS_LAST, jp=jp, J=jp)[0] == EUNSUPPORTED
    assert plan(t, jp=32, J=17)[0] == EUNSUPPORTED and plan(t, jp=32, J=16)[0] == EUNSUPPORTED
    assert plan(t | W, jp=16, J=15)[0] == EUNSUPPORTED and plan(t | W, jp=32, J=33)[0] == EUNSUPPORTED
    assert plan(t | W | _lib.OUT_CHANNELS_LAST, jp=32, J=20)[0] == EUNSUPPORTED
    assert plan(t | one, layout=PLANAR, jp=15, J=1)[0] == EUNSUPPORTED and plan(t | one, jp=16, J=1)[0] == EUNSUPPORTED
    assert plan(t | W, jp=32, J=1, entry="one_train")[0] == EUNSUPPORTED
    assert plan(t, jp=16, J=17)[0] == EUNSUPPORTED and plan(t | _lib.OUT_CHANNELS_LAST, jp=16, J=15)[0] == EUNSUPPORTED
    # heat-maps below 2x2 or above 2^24 pixels
    for h, w in ((18, 1), (1, 24), (4097, 4096)):
        assert plan(t, jp=16, J=15, h=h, w=w)[0] == EUNSUPPORTED and plan(t | W, jp=32, J=21, h=h, w=w)[0] == EUNSUPPORTED
        assert plan(t, jp=16, J=15, h=h, w=w, cube=(8, 8, 32))[0] == EUNSUPPORTED
    # the one-channel forward keeps resolve_one's limits
    for J in (2, 3, 15):
        assert plan(t, layout=PLANAR, jp=15, J=J, entry="one_train")[0] == EUNSUPPORTED
    assert plan(t | _lib.OUT_CHANNELS_LAST, layout=PLANAR, jp=15, J=1, entry="one_train")[0] == EUNSUPPORTED
    # SP3D_HM_BF16_IN on both training entries is what it was
    for entry in ("train", "one_train"):
        assert plan(h16, entry=entry, jp=16, J=15)[0] == EUNSUPPORTED
        assert plan(h16, entry=entry, layout=PLANAR, jp=15, J=1)[0] == EUNSUPPORTED
        assert plan(h16 | one, entry=entry, layout=PLANAR, jp=15, J=1)[0] == EUNSUPPORTED
    # an unknown layout byte or a pixel stride below 1 keeps its own code: where the entry has one - sp3d_unproject_fwd_train
    # takes SP3D_LAYOUT_NHWC and answers every other layout byte alike (tests/test_fwd_request_census.py: the plan answers what
    # the entry answers)
    assert plan(t, layout=7, jp=16, J=15)[0] == plan(0, layout=7, jp=16, J=15)[0] == plan(0, layout=PLANAR, jp=16, J=15)[0] == EUNSUPPORTED
    assert plan(t, layout=7, jp=16, J=1, entry="one_train")[0] == plan(0, layout=7, jp=16, J=1, entry="one_train")[0] == -1
    assert plan(t, layout=PLANAR, jp=0, J=1, entry="one_train")[0] == plan(0, layout=PLANAR, jp=0, J=1, entry="one_train")[0] == -1


def test_cabi_refusals_before_any_launch(lib):
    """SP3D_EUNSUPPORTED (-4) with pointers that are never dereferenced.  A library without the flag ignores the bit and LAUNCHES
    on these dummy pointers, so this runs only where no GPU is visible (tests/test_gpu_bf16_train.py repeats the refusals with
    real tensors)."""
    if torch.cuda.is_available():
        pytest.skip("dummy-pointer refusals are checked only where no GPU is visible")
    t, W = T16(), _lib.HM_WIDE_MASK
    gs = (C.c_float * 3)(8000, 8000, 2000)
    views = (C.c_void_p * 2)(0x1000, 0x1000)
    d, res = C.c_void_p(0x1000), C.c_void_p(0x10000)
    tail = lambda J, hw=(8, 8): (1, 2, J, hw[0], hw[1], 8, 8, 20, gs, 96, 72, None)
    st = (C.c_int64 * 4)(32 * 1280, 1280, 160, 20)
    fwd = lambda layout, jp, J: lib.sp3d_unproject_fwd(views, layout, jp, d, d, d, res, None, *tail(J))
    indexed = lambda layout, jp, J: lib.sp3d_unproject_fwd_indexed(views, layout, jp, d, d, d, d, res, None, *tail(J))
    strided = lambda layout, jp, J: lib.sp3d_unproject_fwd_strided(views, layout, jp, d, None, d, d, res, st, *tail(J))
    train = lambda layout, jp, J, hw=(8, 8): lib.sp3d_unproject_fwd_train(views, layout, jp, d, None, d, d, res, None, d, *tail(J, hw))
    one_train = lambda layout, jp, J, hw=(8, 8): lib.sp3d_unproject_one_fwd_train(views, layout, jp, d, None, d, d, res, None, d, *tail(J, hw))
    for f in (fwd, indexed, strided):
        for layout, jp, J in ((NHWC, 16, 15), (NHWC | W, 32, 21), (NHWC, 4, 4), (PLANAR, 15, 15), (PLANAR | _lib.HM_ONE_CHANNEL, 15, 1),
                              (NHWC | _lib.HM_ONE_CHANNEL, 16, 4), (NHWC | _lib.OUT_CHANNELS_LAST, 16, 16)):
            assert f(layout | t, jp, J) == -4, (hex(layout), jp, J)
    for other in (_lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16_IN, _lib.OUT_ZSPECTRUM, _lib.HM_ONE_ZSPECTRUM):
        assert train(NHWC | t | other, 16, 15) == -4 and train(NHWC | t | W | other, 32, 21) == -4, hex(other)
        assert one_train(PLANAR | t | other, 15, 1) == -4 and one_train(NHWC | t | other, 16, 4) == -4, hex(other)
    assert train(PLANAR | t, 15, 15) == -4 and train(NHWC | t, 32, 17) == -4 and train(NHWC | t | W, 16, 15) == -4
    for jp in (4, 8, 12):
        assert train(NHWC | t, jp, jp) == -4
    assert train(NHWC | t | _lib.HM_ONE_CHANNEL, 16, 1) == -4 and train(PLANAR | t | _lib.HM_ONE_CHANNEL, 15, 1) == -4
    assert train(NHWC | t | W | _lib.OUT_CHANNELS_LAST, 32, 20) == -4 and train(NHWC | t | _lib.OUT_CHANNELS_LAST, 16, 15) == -4
    for hw in ((8, 1), (1, 8), (4097, 4096)):
        assert train(NHWC | t, 16, 15, hw) == -4 and train(NHWC | t | W, 32, 21, hw) == -4 and one_train(PLANAR | t, 15, 1, hw) == -4
    assert one_train(PLANAR | t, 15, 2) == -4 and one_train(PLANAR | t | _lib.OUT_CHANNELS_LAST, 15, 1) == -4
    # SP3D_HM_BF16_IN on both training entries is still refused
    assert train(NHWC | _lib.HM_BF16_IN, 16, 15) == -4 and one_train(PLANAR | _lib.HM_BF16_IN, 15, 1) == -4
    assert one_train(NHWC | _lib.HM_BF16_IN, 16, 4) == -4


# ---- Python: the routes and the switches, on CPU tensors -----------------------------------------------------------------
def _layer(**switches):
    cfg = load_config(None)
    layer = ProjectLayer(cfg)
    for k, v in switches.items():
        setattr(layer, k, v)
    return layer, [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]


def _maps(J, w, h, dtype=BF, V=3, B=2, grad=True):
    return [torch.zeros(B, J, h, w, dtype=dtype).requires_grad_(grad) for _ in range(V)]


def test_switch(monkeypatch):
    cfg = load_config(None)
    for value, want in ((None, False), ("", False), ("0", False), ("1", True), ("yes", True)):
        if value is None:
            monkeypatch.delenv("SP3D_BF16_TRAIN", raising=False)
        else:
            monkeypatch.setenv("SP3D_BF16_TRAIN", value)
        assert ProjectLayer(cfg).bf16_train is want, value
    monkeypatch.delenv("SP3D_BF16_TRAIN", raising=False)
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
    from selfpose3d_amd.multi_person_posenet import MultiPersonPoseNet
    from selfpose3d_amd.multi_person_posenet_ssv import MultiPersonPoseNetSSV
    from selfpose3d_amd.pose_regression_net import PoseRegressionNet
    from selfpose3d_amd.pose_resnet import PoseResNet
    for cls in (CuboidProposalNet, CuboidProposalNetSoft, PoseRegressionNet):
        net = cls(cfg)
        assert net.project_layer.bf16_train is False
        assert net.use_bf16_training() is net and net.project_layer.bf16_train is True and net.project_layer.bf16_maps is False
        assert net.use_bf16_training(False).project_layer.bf16_train is False
    for cls in (MultiPersonPoseNet, MultiPersonPoseNetSSV):
        backbone = PoseResNet(cfg)
        model = cls(backbone, cfg)
        assert model.use_bf16_training() is model
        assert model.root_net.project_layer.bf16_train and model.pose_net.project_layer.bf16_train
        assert backbone.bf16_heatmaps is False                          # the backbone is not touched
        model.use_bf16_training(False)
        assert not (model.root_net.project_layer.bf16_train or model.pose_net.project_layer.bf16_train)


def test_routes_of_the_table():
    layer, (w, h) = _layer(bf16_train=True, wide_grad=True, one_channel_grad=True)
    with torch.enable_grad():
        for J in (13, 15, 16):
            for pad, cl in ((False, False), (True, True), (True, False)):
                want = Route("packed", NHWC, 16, BF, "cubes", 16 if pad else J, cl, backward="mask16", autograd=True)
                assert layer.route(_maps(J, w, h), pad_channels=pad, channels_last=cl) == want, (J, pad, cl)
            assert layer.route(_maps(J, w, h), want_grids=False) == Route("packed", NHWC, 16, BF, "cubes", J, backward="mask16", autograd=True)
        assert layer.route(_maps(16, w, h), channels_last=True).channels_last is True          # J % 4 == 0 without padding
        for J in (17, 21, 32):
            want = Route("packed", NHWC, 32, BF, "cubes", J, False, backward="mask2x16", autograd=True)
            assert layer.route(_maps(J, w, h)) == want and layer.route(_maps(J, w, h), pad_channels=True, channels_last=True) == want
        # one channel where it lies: a slice of planar tensors, of a bf16 producer's buffer, a contiguous (B,1,h,w) list
        full = _maps(15, w, h)
        for j in (2, 7):
            hms = [a[:, j:j + 1] for a in full]
            assert layer.route(hms) == Route("one", PLANAR, 15, BF, "cubes", 1, False, backward="one", autograd=True)
            assert layer.route(hms, pad_channels=True, channels_last=True) == Route("one", PLANAR, 15, BF, "cubes", 4, True, backward="one", autograd=True)
            assert layer.route(hms, pad_channels=True) == Route("one", PLANAR, 15, BF, "cubes", 4, False, backward="one", autograd=True)
        for jp, J in ((16, 15), (32, 17)):
            packed = torch.zeros(3, 2, h, w, jp, dtype=BF).requires_grad_(True)
            hms = [v[:, 5:6] for v in nhwc_heatmap_views(packed, J)]
            assert layer.route(hms) == Route("one", NHWC, jp, BF, "cubes", 1, False, backward="one", autograd=True)
        assert layer.route(_maps(1, w, h)) == Route("one", PLANAR, 1, BF, "cubes", 1, False, backward="one", autograd=True)
        # a bf16 producer's (V,B,h,w,16|32) buffer keeps the packed rows (it is read in place: _launch_cubes)
        for jp, J in ((16, 15), (32, 17)):
            hms = nhwc_heatmap_views(torch.zeros(3, 2, h, w, jp, dtype=BF).requires_grad_(True), J)
            assert layer.route(hms)[:4] == ("packed", NHWC, jp, BF)
        with pytest.raises(_lib.Sp3dError, match="out="):
            layer.route(_maps(15, w, h), want_grids=False, out=True)


def test_everything_else_takes_todays_route():
    on, (w, h) = _layer(bf16_train=True)
    off, _ = _layer()
    full = _maps(15, w, h)
    one = [a[:, 7:8] for a in full]
    mixed = _maps(15, w, h)[:2] + _maps(15, w, h, F32)[:1]
    cases = [("4 joints", _maps(4, w, h), {}), ("12 joints", _maps(12, w, h), {}), ("17 joints without wide_grad", _maps(17, w, h), {}),
             ("33 joints", _maps(33, w, h), {}), ("fp32 maps", _maps(15, w, h, F32), {}), ("a mixture", mixed, {}),
             ("one channel without one_channel_grad", one, {}), ("fp32 one channel", [a.float()[:, 7:8] for a in full], dict(one_channel_grad=True)),
             ("the planar path", _maps(15, w, h), dict(mode="planar")), ("17 joints, planar path", _maps(17, w, h), dict(mode="planar", wide_grad=True)),
             ("no gradient", _maps(15, w, h, grad=False), {}), ("no gradient, bf16_maps", _maps(15, w, h, grad=False), dict(bf16_maps=True)),
             ("fp32 maps, every switch", _maps(15, w, h, F32), dict(bf16_maps=True, wide_grad=True, one_channel_grad=True, one_channel=True)),
             ("a 1-pixel-wide map", _maps(15, 1, h), {})]
    with torch.enable_grad():
        for name, hms, sw in cases:
            for k, v in sw.items():
                setattr(on, k, v), setattr(off, k, v)
            for kw in ({}, dict(pad_channels=True, channels_last=True), dict(want_grids=False)):
                a, b = on.route(hms, **kw), off.route(hms, **kw)
                assert a == b, (name, kw, a, b)
                assert a.elem == F32 or name == "no gradient, bf16_maps", (name, kw, a)      # (the inference switch's own bf16 route)
            for k in sw:
                setattr(on, k, getattr(_layer()[0], k)), setattr(off, k, getattr(_layer()[0], k))
    # without grad mode the switch is no inference switch: bf16 maps keep today's route
    with torch.no_grad():
        assert on.route(_maps(15, w, h)) == off.route(_maps(15, w, h))
    # io_dtype = bfloat16 (bf16 maps AND cubes) keeps its route, and its refusal of a one-channel list
    cfg = load_config(None)
    a, b = ProjectLayer(cfg, io_dtype=BF), ProjectLayer(cfg, io_dtype=BF)
    a.bf16_train = True
    with torch.enable_grad():
        assert a.route(_maps(15, w, h)) == b.route(_maps(15, w, h)) and a.route(_maps(15, w, h)).backward == "planar"
        for layer in (a, b):
            with pytest.raises(_lib.Sp3dError, match="bf16 storage needs"):
                layer.route(_maps(17, w, h))
            with pytest.raises(_lib.Sp3dError, match="bf16 storage needs"):
                layer.route(one)
    # bf16_maps keeps its meaning: with a gradient it is ignored, with or without the new switch
    both, _ = _layer(bf16_train=True, bf16_maps=True)
    with torch.enable_grad():
        assert both.route(_maps(15, w, h)) == on.route(_maps(15, w, h))
        assert both.route(_maps(15, w, h, F32)) == off.route(_maps(15, w, h, F32))
