"""bf16 heat-maps through the fused fronts (SP3D_HM_BF16_IN, ``ProjectLayer.bf16_maps``) without a GPU: the flag, the launches
resolve_fwd plans for it next to each of the three flags it belongs to (sp3d_unproject_fwd_plan), every refusal the header
lists - through the plan where a plan entry exists and through the C entries with pointers that are never dereferenced -, and
the Python classifier and switches.  tests/test_gpu_bf16_front.py holds the values."""
import ctypes as C
import os
import re

import pytest
import torch

from selfpose3d_amd import _lib, build as sbuild
from selfpose3d_amd.config import load_config
from selfpose3d_amd.project_layer import ProjectLayer, one_channel_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NHWC, PLANAR = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
EUNSUPPORTED = -4
H16 = 0x8000
ZD_BLOCK, ZD_LDS = 320, 5 * max(16 * 68, 640) * 4       # the fp32 ZD launch: five waves, a (16 x 68)-float tile per wave
ONE_ZD_BLOCK, ONE_ZD_LDS = 320, 16 * 20 * 4
# what a launch's geometry is made of: everything of a plan record but the kernel, its LDS and the two byte offsets
GEOMETRY = [f for f in _lib.PLAN_FIELDS if f not in ("lds", "view_off", "out_off")]


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def plan(flags, layout=NHWC, jp=16, J=15, entry="indexed", B=2, V=3, h=18, w=24, cube=(8, 12, 20), strides=None):
    return _lib.unproject_fwd_plan(entry, layout | flags, jp, B, V, J, h, w, cube, 0, strides)


def test_flag_abi_version_and_entry_list():
    from tests.test_glue_sweep_reference import LEDGER, _header_signatures
    with open(os.path.join(ROOT, "include", "sp3d.h")) as fh:
        hdr = fh.read()
    assert int(re.search(r"\bSP3D_HM_BF16_IN\s*=\s*(0x[0-9a-fA-F]+)", hdr).group(1), 0) == 0x8000 == _lib.HM_BF16_IN == H16
    assert "SP3D_ABI_VERSION 3" in hdr and _lib.ABI_VERSION == 3
    # a flag bit, not a symbol: the header declares what the ledger lists, no more
    assert sorted(_header_signatures(os.path.join(ROOT, "include", "sp3d.h"))) == sorted(LEDGER)
    assert len(_lib.SIGNATURES) == 57


# ---- the brick-h kernel with the z-spectrum result ----------------------------------------------------------------------
@pytest.mark.parametrize("cube", [(8, 12, 20), (80, 80, 20)])
@pytest.mark.parametrize("B", [1, 3, 4])
def test_zspectrum_plan_at_jp16(lib, cube, B):
    for J in (13, 15, 16):
        rc, launches, _ = plan(H16 | _lib.OUT_ZSPECTRUM, jp=16, J=J, B=B, cube=cube)
        assert rc == 0 and len(launches) == 1, (rc, J)
        l = launches[0]
        assert l["name"] == "unproject_brick_h_kernel<false, float, 16, true>"
        assert (l["block"], l["lds"], l["view_off"], l["out_off"], l["grids"], l["J"]) == (ZD_BLOCK, ZD_LDS, 0, 0, 0, J)
        rc, ref, _ = plan(_lib.OUT_ZSPECTRUM, jp=16, J=J, B=B, cube=cube)
        assert rc == 0 and ref[0]["name"] == "unproject_brick_kernel<16, false, float, float, true, 16>"
        assert [l[f] for f in GEOMETRY] == [ref[0][f] for f in GEOMETRY]
        assert l["lds"] == ref[0]["lds"]


@pytest.mark.parametrize("cube", [(8, 12, 20), (80, 80, 20)])
@pytest.mark.parametrize("B", [1, 3, 4])
def test_zspectrum_plan_at_jp32(lib, cube, B):
    name = "unproject_brick_h_kernel<false, float, 32, true>"
    for J in (17, 21, 32):
        rc, launches, _ = plan(H16 | _lib.OUT_ZSPECTRUM, jp=32, J=J, B=B, cube=cube)
        assert rc == 0 and [l["name"] for l in launches] == [name, name], (rc, J)
        rc, ref, _ = plan(_lib.OUT_ZSPECTRUM, jp=32, J=J, B=B, cube=cube)
        assert rc == 0 and len(ref) == 2
        # group 1 starts 16 bf16 channels = 32 bytes into the pixel, and where the fp32 plan's group 1 starts in the spectrum
        assert [l["view_off"] for l in launches] == [0, 32] and [l["view_off"] for l in ref] == [0, 64]
        assert [l["out_off"] for l in launches] == [r["out_off"] for r in ref]
        assert launches[1]["out_off"] == 16 * 15 * (cube[0] // 4) * (cube[1] // 4) * 16 * 8
        assert [l["J"] for l in launches] == [16, J - 16]
        for l, r in zip(launches, ref):
            assert (l["block"], l["lds"], l["grids"]) == (ZD_BLOCK, ZD_LDS, 0)      # both groups have width 16
            assert [l[f] for f in GEOMETRY] == [r[f] for f in GEOMETRY]
    rc, launches, _ = plan(H16 | _lib.OUT_ZSPECTRUM, jp=32, J=16, B=B, cube=cube)           # no second group
    assert rc == 0 and [(l["name"], l["view_off"], l["out_off"], l["J"]) for l in launches] == [(name, 0, 0, 16)]
    ref = plan(_lib.OUT_ZSPECTRUM, jp=32, J=16, B=B, cube=cube)[1]
    assert [launches[0][f] for f in GEOMETRY] == [ref[0][f] for f in GEOMETRY]


# ---- the one-channel kernels ---------------------------------------------------------------------------------------------
LADDER = {3: (3, 4), 5: (5, 4), 7: (8, 4), 16: (16, 8)}


@pytest.mark.parametrize("V", [3, 5, 7, 16])
@pytest.mark.parametrize("layout,jp", [(PLANAR, 1), (PLANAR, 15), (NHWC, 16), (NHWC, 32)])
def test_one_channel_plans(lib, V, layout, jp):
    vt, cs = LADDER[V]
    h, w = 18, 24
    want = (h * w * jp, w * jp, jp) if layout == NHWC else (jp * h * w, w, 1)           # sample, row, pixel stride in ELEMENTS
    sy, sx = 3 + 1, 7 * (3 + 1) + 2                     # a (5,7,3) cube inside a larger buffer: padded rows, planes and channels
    sj = 5 * sx + 11
    forms = [("indexed", 1, 0, None, "false"), ("indexed", 4, 0, None, "false"), ("indexed", 4, _lib.OUT_CHANNELS_LAST, None, "true"),
             ("strided", 1, 0, (4 * sj, sj, sx, sy), "false"), ("strided", 4, 0, (4 * sj, sj, sx, sy), "false")]
    for entry, J, cl, strides, clname in forms:
        for B in (1, 3):
            rc, launches, _ = plan(H16 | _lib.HM_ONE_CHANNEL | cl, layout, jp, J, entry, B=B, V=V, cube=(5, 7, 3), strides=strides)
            assert rc == 0 and len(launches) == 1, (rc, entry, J, cl)
            l = launches[0]
            assert l["name"] == "unproject_one_kernel<%d, %d, %s, false, bf16_t>" % (vt, cs, clname)
            assert (l["block"], l["lds"], l["view_off"], l["out_off"], l["J"]) == (64, 0, 0, 0, J)
            assert (l["nscalars"], l["s0"], l["s1"], l["s2"]) == (3,) + want
            rc, ref, _ = plan(_lib.HM_ONE_CHANNEL | cl, layout, jp, J, entry, B=B, V=V, cube=(5, 7, 3), strides=strides)
            assert rc == 0 and ref[0]["name"] == "unproject_one_kernel<%d, %d, %s>" % (vt, cs, clname)
            assert [l[f] for f in _lib.PLAN_FIELDS] == [ref[0][f] for f in _lib.PLAN_FIELDS]
    for B in (1, 3, 4):
        rc, launches, _ = plan(H16 | _lib.HM_ONE_ZSPECTRUM, layout, jp, 1, B=B, V=V)
        assert rc == 0 and len(launches) == 1
        l = launches[0]
        assert l["name"] == "unproject_one_zd_kernel<%d, %d, bf16_t>" % (vt, cs)
        assert (l["block"], l["lds"], l["view_off"], l["out_off"], l["J"], l["grids"]) == (ONE_ZD_BLOCK, ONE_ZD_LDS, 0, 0, 1, 0)
        assert (l["nscalars"], l["s0"], l["s1"], l["s2"]) == (3,) + want
        rc, ref, _ = plan(_lib.HM_ONE_ZSPECTRUM, layout, jp, 1, B=B, V=V)
        assert rc == 0 and ref[0]["name"] == "unproject_one_zd_kernel<%d, %d>" % (vt, cs)
        assert [l[f] for f in _lib.PLAN_FIELDS] == [ref[0][f] for f in _lib.PLAN_FIELDS]


def test_one_channel_byte_limit_counts_two_byte_elements(lib):
    for flag in (_lib.HM_ONE_CHANNEL, _lib.HM_ONE_ZSPECTRUM):
        kw = dict(layout=NHWC, J=1, h=4096, w=4096)
        assert plan(flag, jp=31, **kw)[0] == 0 and plan(flag, jp=33, **kw)[0] == EUNSUPPORTED          # fp32: 2^31 bytes at 32
        assert plan(H16 | flag, jp=33, **kw)[0] == 0 and plan(H16 | flag, jp=63, **kw)[0] == 0            # bf16: at 64
        assert plan(H16 | flag, jp=65, **kw)[0] == EUNSUPPORTED
        assert plan(H16 | flag, layout=NHWC, jp=1 << 20, J=1)[0] == EUNSUPPORTED                         # a row of 2^24 elements
        for h, w in ((18, 1), (1, 24), (4097, 4096)):
            assert plan(H16 | flag, layout=PLANAR, jp=15, J=1, h=h, w=w)[0] == EUNSUPPORTED


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_plan_refusals(lib):
    z, one, ozd = _lib.OUT_ZSPECTRUM, _lib.HM_ONE_CHANNEL, _lib.HM_ONE_ZSPECTRUM
    ok = {z: dict(jp=16, J=15), one: dict(layout=PLANAR, jp=15, J=1), ozd: dict(layout=PLANAR, jp=15, J=1)}
    for flag, kw in ok.items():
        assert plan(H16 | flag, **kw)[0] == 0
    # on its own: every layout and pixel width the cube-writing kernels take
    for layout, jp, J in ((NHWC, 16, 15), (NHWC, 32, 17), (NHWC, 4, 1), (NHWC, 8, 8), (PLANAR, 15, 15), (PLANAR, 1, 1)):
        assert plan(H16, layout, jp, J)[0] == EUNSUPPORTED, (layout, jp, J)
        assert plan(H16, layout, jp, J, cube=(64, 64, 64))[0] == EUNSUPPORTED
        assert plan(H16 | _lib.OUT_CHANNELS_LAST, layout, jp, J)[0] == EUNSUPPORTED
    # next to the bf16 storage pair or the two-plane mask
    for other in (_lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16 | _lib.OUT_BF16, _lib.HM_WIDE_MASK):
        assert plan(H16 | other, jp=16, J=15)[0] == EUNSUPPORTED and plan(H16 | other, jp=32, J=17)[0] == EUNSUPPORTED
        for flag, kw in ok.items():
            assert plan(H16 | flag | other, **kw)[0] == EUNSUPPORTED, (hex(flag), hex(other))
        assert plan(H16 | other, jp=32, J=17, entry="train")[0] == EUNSUPPORTED
    # channels-last results come from the one-channel kernel alone
    assert plan(H16 | z | _lib.OUT_CHANNELS_LAST, jp=16, J=16)[0] == EUNSUPPORTED
    assert plan(H16 | ozd | _lib.OUT_CHANNELS_LAST, layout=PLANAR, jp=15, J=1)[0] == EUNSUPPORTED
    assert plan(H16 | one | _lib.OUT_CHANNELS_LAST, layout=PLANAR, jp=15, J=4, cube=(5, 7, 3))[0] == 0
    # exactly one of the three
    for pair in (z | one, z | ozd, one | ozd, z | one | ozd):
        for layout, jp, J in ((NHWC, 16, 1), (NHWC, 16, 15), (PLANAR, 15, 1)):
            assert plan(H16 | pair, layout, jp, J)[0] == EUNSUPPORTED, hex(pair)
    # the limits of the flag it stands next to
    assert plan(H16 | z, layout=PLANAR, jp=15, J=15)[0] == EUNSUPPORTED
    for jp, J in ((4, 4), (8, 8), (12, 12), (32, 33), (64, 33)):
        assert plan(H16 | z, jp=jp, J=J)[0] == EUNSUPPORTED, (jp, J)
    for cube in ((8, 12, 16), (8, 12, 24), (10, 12, 20), (8, 10, 20)):
        assert plan(H16 | z, jp=16, J=15, cube=cube)[0] == EUNSUPPORTED and plan(H16 | ozd, PLANAR, 15, 1, cube=cube)[0] == EUNSUPPORTED
    for J in (2, 3, 15):
        assert plan(H16 | one, PLANAR, 15, J)[0] == EUNSUPPORTED and plan(H16 | ozd, PLANAR, 15, J)[0] == EUNSUPPORTED
    assert plan(H16 | ozd, PLANAR, 15, 4)[0] == EUNSUPPORTED
    # the training forwards, the entry without a layout word, and the strided entry next to either spectrum flag
    sj = 8 * 12 * 20
    st = (16 * sj, sj, 12 * 20, 20)
    for flag, kw in ok.items():
        assert plan(H16 | flag, entry="train", **kw)[0] == EUNSUPPORTED
        assert plan(H16 | flag, entry="one_train", **kw)[0] == EUNSUPPORTED
        assert plan(H16 | flag, entry="zdft", **kw)[0] == EUNSUPPORTED
    for entry in ("train", "one_train", "zdft"):
        assert plan(H16, entry=entry, jp=16, J=15)[0] == EUNSUPPORTED
        assert plan(H16, entry=entry, layout=PLANAR, jp=15, J=1)[0] == EUNSUPPORTED
    assert plan(0, entry="zdft", jp=16, J=15)[0] == 0 and plan(0, entry="one_train", layout=PLANAR, jp=15, J=1)[0] == 0
    for flag in (z, ozd):
        assert plan(H16 | flag, entry="strided", strides=st, **ok[flag])[0] == EUNSUPPORTED
        assert plan(H16 | flag, entry="strided", **ok[flag])[0] == EUNSUPPORTED
    assert plan(H16, entry="strided", jp=16, J=15, strides=st)[0] == EUNSUPPORTED


def test_pinned_refusals_of_the_storage_flags_hold(lib):
    """SP3D_HM_BF16 / SP3D_OUT_BF16 stay refused next to the three flags, with or without the new bit"""
    for flag, kw in ((_lib.OUT_ZSPECTRUM, dict(jp=16, J=15)), (_lib.OUT_ZSPECTRUM, dict(jp=32, J=17)),
                     (_lib.HM_ONE_CHANNEL, dict(layout=PLANAR, jp=15, J=1)), (_lib.HM_ONE_CHANNEL, dict(jp=16, J=4)),
                     (_lib.HM_ONE_ZSPECTRUM, dict(layout=PLANAR, jp=15, J=1)), (_lib.HM_ONE_ZSPECTRUM, dict(jp=32, J=1))):
        for other in (_lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16 | _lib.OUT_BF16):
            assert plan(flag | other, **kw)[0] == EUNSUPPORTED, (hex(flag), hex(other))
    # and the storage pair's own kernels are what they were
    rc, launches, _ = plan(_lib.HM_BF16, jp=16, J=15, cube=(64, 64, 64))
    assert rc == 0 and [l["name"] for l in launches] == ["unproject_brick_h_kernel<false, float, 16>"]
    rc, launches, _ = plan(_lib.HM_BF16, jp=32, J=17, cube=(64, 64, 64))
    assert rc == 0 and [(l["name"], l["view_off"]) for l in launches] == [("unproject_brick_h_kernel<false, float, 32>", 0),
                                                                          ("unproject_brick_h_kernel<false, float, 32>", 32)]


def test_cabi_refusals_before_any_launch(lib):
    """SP3D_EUNSUPPORTED (-4) with pointers that are never dereferenced.  A library without the flag masks the bit off and
    LAUNCHES on these dummy pointers, so this runs only where no GPU is visible (tests/test_gpu_bf16_front.py repeats the
    pinned refusals with real tensors)."""
    if torch.cuda.is_available():
        pytest.skip("dummy-pointer refusals are checked only where no GPU is visible")
    gs = (C.c_float * 3)(8000, 8000, 2000)
    views = (C.c_void_p * 2)(0x1000, 0x1000)
    d, spec = C.c_void_p(0x1000), C.c_void_p(0x10000)
    z, one, ozd = _lib.OUT_ZSPECTRUM, _lib.HM_ONE_CHANNEL, _lib.HM_ONE_ZSPECTRUM
    f, fi = lib.sp3d_unproject_fwd, lib.sp3d_unproject_fwd_indexed

    def both(layout, jp, J, cubes=spec, grids=None, cube=(8, 8, 20)):
        tail = (1, 2, J, 8, 8, *cube, gs, 96, 72, None)
        a = f(views, layout, jp, d, d, d, cubes, grids, *tail)
        b = fi(views, layout, jp, d, None, d, d, cubes, grids, *tail)
        c = fi(views, layout, jp, d, d, d, d, cubes, grids, *tail)          # with sample_of
        assert a == b == c, (a, b, c)
        return a

    st = (C.c_int64 * 4)(32 * 1280, 1280, 160, 20)
    tail = lambda J: (1, 2, J, 8, 8, 8, 8, 20, gs, 96, 72, None)
    strided = lambda layout, jp, J: lib.sp3d_unproject_fwd_strided(views, layout, jp, d, None, d, d, spec, st, *tail(J))
    train = lambda layout, jp, J: lib.sp3d_unproject_fwd_train(views, layout, jp, d, None, d, d, spec, None, d, *tail(J))
    one_train = lambda layout, jp, J: lib.sp3d_unproject_one_fwd_train(views, layout, jp, d, None, d, d, spec, None, d, *tail(J))
    # on its own
    for layout, jp, J in ((NHWC, 16, 15), (NHWC, 32, 17), (NHWC, 4, 4), (PLANAR, 15, 15)):
        assert both(layout | H16, jp, J) == -4 and both(layout | H16, jp, J, grids=d) == -4
        assert both(layout | H16 | _lib.OUT_CHANNELS_LAST, jp, J) == -4
        assert strided(layout | H16, jp, J) == -4 and train(layout | H16, jp, J) == -4
    assert one_train(PLANAR | H16, 15, 1) == -4 and one_train(NHWC | H16, 16, 4) == -4
    ok = ((z, NHWC, 16, 15), (one, PLANAR, 15, 1), (ozd, PLANAR, 15, 1))
    for flag, layout, jp, J in ok:
        for other in (_lib.HM_BF16, _lib.OUT_BF16, _lib.HM_WIDE_MASK):
            assert both(layout | H16 | flag | other, jp, J) == -4, (hex(flag), hex(other))
        assert train(layout | H16 | flag, jp, J) == -4 and one_train(layout | H16 | flag, jp, J) == -4
    assert both(NHWC | H16 | z | _lib.OUT_CHANNELS_LAST, 16, 16) == -4
    assert both(PLANAR | H16 | ozd | _lib.OUT_CHANNELS_LAST, 15, 1) == -4
    for pair in (z | one, z | ozd, one | ozd):
        assert both(NHWC | H16 | pair, 16, 1) == -4
    assert strided(NHWC | H16 | z, 16, 15) == -4 and strided(PLANAR | H16 | ozd, 15, 1) == -4
    # what the flags next to it refuse, they refuse with it
    assert both(NHWC | H16 | z, 16, 15, grids=d) == -4 and both(PLANAR | H16 | ozd, 15, 1, grids=d) == -4
    for off in (8, 64):
        assert both(NHWC | H16 | z, 16, 15, cubes=C.c_void_p(0x10000 + off)) == -4
        assert both(PLANAR | H16 | ozd, 15, 1, cubes=C.c_void_p(0x10000 + off)) == -4
    assert both(NHWC | H16 | z, 16, 15, cube=(8, 8, 16)) == -4 and both(PLANAR | H16 | one, 15, 2) == -4


# ---- Python: the classifier and the switches, no GPU -----------------------------------------------------------------------
def test_one_channel_source_with_dtype():
    bf, f32 = torch.bfloat16, torch.float32
    h, w = 6, 5
    full = [torch.zeros(3, 15, h, w, dtype=bf) for _ in range(4)]
    for j in (0, 2, 7, 14):                                              # planar slice, odd and even channel
        hms = [a[:, j:j + 1] for a in full]
        assert one_channel_source(hms, bf) == (PLANAR, 15)
        assert one_channel_source(hms) is None and one_channel_source(hms, f32) is None          # the default call is unchanged
    for jp in (16, 32):                                                  # a slice of the channels-last buffer
        packed = torch.zeros(4, 3, h, w, jp, dtype=bf)
        for j in (0, 3, jp - 1):
            hms = [packed[c].permute(0, 3, 1, 2)[:, j:j + 1] for c in range(4)]
            assert one_channel_source(hms, bf) == (NHWC, jp)
            assert one_channel_source(hms) is None
    contiguous = [torch.zeros(3, 1, h, w, dtype=bf) for _ in range(4)]
    assert one_channel_source(contiguous, bf) == (PLANAR, 1) and one_channel_source(contiguous) is None
    for t in (torch.zeros(1, 15, h, w, dtype=bf), torch.zeros(1, 1, h, w, dtype=bf)):            # B = 1: the sample stride is no evidence
        assert one_channel_source([t[:, 0:1]] * 2, bf) == (PLANAR, 1)
    one = torch.zeros(1, h, w, 16, dtype=bf).permute(0, 3, 1, 2)[:, 5:6]
    assert one_channel_source([one, one], bf) == (NHWC, 16)
    expanded = [torch.zeros(1, 1, h, w, dtype=bf).expand(3, 1, h, w) for _ in range(4)]
    assert one_channel_source(expanded, bf) is None
    mixed = [full[0][:, 2:3], torch.zeros(4, 3, h, w, 16, dtype=bf)[0].permute(0, 3, 1, 2)[:, 2:3]]
    assert one_channel_source(mixed, bf) is None
    assert one_channel_source([full[0][:, 2:3], full[1][:, 2:3].float()], bf) is None            # views of different type
    assert one_channel_source([a[:, 2:4] for a in full], bf) is None                             # J = 2
    # fp32 tensors classify as before, and not as bf16
    f = [torch.zeros(3, 15, h, w) for _ in range(4)]
    assert one_channel_source([a[:, 2:3] for a in f]) == (PLANAR, 15) and one_channel_source([a[:, 2:3] for a in f], bf) is None
    # the byte limit counts 2-byte elements: a (4096 x 4096 x 33)-element sample is below 2^31 bytes as bf16 only
    big = lambda ps, dt: torch.empty_strided((2, 1, 4096, 4096), (4096 * 4096 * ps, 1, 4096 * ps, ps), dtype=dt, device="meta")
    big16, big32 = big(33, bf), big(33, f32)
    assert one_channel_source([big16], bf) == (NHWC, 33) and one_channel_source([big32]) is None
    assert one_channel_source([big(63, bf)], bf) == (NHWC, 63) and one_channel_source([big(65, bf)], bf) is None


def test_switches(monkeypatch):
    cfg = load_config(None)
    for value, want in ((None, False), ("", False), ("0", False), ("1", True), ("yes", True)):
        if value is None:
            monkeypatch.delenv("SP3D_BF16_MAPS", raising=False)
        else:
            monkeypatch.setenv("SP3D_BF16_MAPS", value)
        assert ProjectLayer(cfg).bf16_maps is want, value
    monkeypatch.delenv("SP3D_BF16_MAPS", raising=False)
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
    from selfpose3d_amd.multi_person_posenet import MultiPersonPoseNet
    from selfpose3d_amd.pose_regression_net import PoseRegressionNet
    from selfpose3d_amd.pose_resnet import PoseResNet
    for cls in (CuboidProposalNet, CuboidProposalNetSoft, PoseRegressionNet):
        net = cls(cfg)
        assert net.project_layer.bf16_maps is False
        assert net.use_bf16_heatmaps() is net and net.project_layer.bf16_maps is True
        assert net.use_bf16_heatmaps(False).project_layer.bf16_maps is False
    backbone = PoseResNet(cfg)
    assert backbone.bf16_heatmaps is False
    model = MultiPersonPoseNet(backbone, cfg)
    assert model.use_bf16_heatmaps() is model
    assert backbone.bf16_heatmaps and model.root_net.project_layer.bf16_maps and model.pose_net.project_layer.bf16_maps
    model.use_bf16_heatmaps(False)
    assert not (backbone.bf16_heatmaps or model.root_net.project_layer.bf16_maps or model.pose_net.project_layer.bf16_maps)


class _Cuda:
    """stands where a GPU heat-map would (tests/test_one_front_host.py): the refusals read shapes, strides and flags only"""
    is_cuda, requires_grad = True, False

    def __init__(self, t):
        self.t, self.shape, self.dtype, self.device = t, t.shape, t.dtype, t.device

    def dim(self):
        return self.t.dim()

    def stride(self):
        return self.t.stride()


def test_io_dtype_and_bf16_maps_exclude_each_other():
    cfg = load_config(None)
    w, h = (int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    layer = ProjectLayer(cfg, io_dtype=torch.bfloat16)
    layer.bf16_maps = True
    hms = [_Cuda(torch.zeros(2, 15, h, w)) for _ in range(3)]
    with torch.no_grad(), pytest.raises(_lib.Sp3dError, match="exclude each other"):
        layer.get_voxel_zspectrum(hms, [], [8000.0, 8000.0, 2000.0], [[0.0, 0.0, 0.0]], [80, 80, 20], 28)
    # the spectrum routes keep their switches: 17..32 joints without ``wide_zspectrum``, one channel without ``one_zspectrum``
    layer = ProjectLayer(cfg)
    layer.bf16_maps = True
    for bad in ([_Cuda(torch.zeros(2, 17, h, w, dtype=torch.bfloat16)) for _ in range(3)],
                [_Cuda(torch.zeros(2, 15, h, w, dtype=torch.bfloat16)[:, 2:3]) for _ in range(3)],
                [_Cuda(torch.zeros(2, 12, h, w, dtype=torch.bfloat16)) for _ in range(3)]):
        with torch.no_grad(), pytest.raises(_lib.Sp3dError, match="13..16 joints only"):
            layer.get_voxel_zspectrum(bad, [], [8000.0, 8000.0, 2000.0], [[0.0, 0.0, 0.0]], [80, 80, 20], 28)
