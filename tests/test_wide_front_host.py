"""The z-spectrum result at 17..32 joints (SP3D_OUT_ZSPECTRUM, ``SP3D_WIDE_FRONT``) without a GPU: the flag, the launches
resolve_fwd plans for it (sp3d_unproject_fwd_plan), every refusal the header lists - through the plan where a plan entry
exists and through the C entries with pointers that are never dereferenced -, the pins that must not move, and the Python
predicates with the switch off.  tests/test_gpu_wide_front.py holds the values."""
import ctypes as C
import os
import re

import pytest
import torch

from selfpose3d_amd import _lib, build as sbuild
from selfpose3d_amd.config import load_config
from selfpose3d_amd.project_layer import ProjectLayer
from selfpose3d_amd.v2v_net import V2VNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMPUS = os.path.join(ROOT, "configs", "campus_synthetic_coco17_cam3.yaml")
NHWC, PLANAR = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
EUNSUPPORTED = -4
CUBE = (24, 16, 20)
K = 15                                   # SZ / 2 + 1 at SZ = 28


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def plan(entry="indexed", layout=NHWC, jp=32, B=2, V=3, J=17, h=18, w=24, cube=CUBE, flags=None, strides=None):
    flags = _lib.OUT_ZSPECTRUM if flags is None else flags
    return _lib.unproject_fwd_plan(entry, layout | flags, jp, B, V, J, h, w, cube, 0, strides)


def test_flag_value_matches_the_header():
    with open(os.path.join(ROOT, "include", "sp3d.h")) as fh:
        hdr = fh.read()
    assert int(re.search(r"\bSP3D_OUT_ZSPECTRUM\s*=\s*(0x[0-9a-fA-F]+)", hdr).group(1), 0) == 0x2000 == _lib.OUT_ZSPECTRUM
    assert "SP3D_ABI_VERSION 3" in hdr and _lib.ABI_VERSION == 3
    assert len(_lib.SIGNATURES) == 57                    # the feature is a flag bit, not a symbol


@pytest.mark.parametrize("J,W", [(17, 4), (21, 8), (29, 16), (32, 16)])
def test_plan_at_jp32_is_two_zd_groups(lib, J, W):
    rc, launches, tuning = plan(J=J)
    assert rc == 0 and len(launches) == 2
    assert [l["name"] for l in launches] == ["unproject_brick_kernel<16, false, float, float, true, 32>",
                                             "unproject_brick_kernel<%d, false, float, float, true, 32>" % W]
    plane16 = 16 * K * (CUBE[0] // 4) * (CUBE[1] // 4) * 16 * 8
    assert plane16 == 16 * 15 * 6 * 4 * 16 * 8
    assert [(l["J"], l["view_off"], l["out_off"], l["grids"]) for l in launches] == [(16, 0, 0, 0), (J - 16, 64, plane16, 0)]
    assert [l["block"] for l in launches] == [320, 320]
    # per wave max(JP * WOSTR, WREC) floats (sp3d_unproject_host.h), five waves: what the kernel of that width indexes
    assert [l["lds"] for l in launches] == [5 * max(16 * 68, 640) * 4, 5 * max(W * 68, 640) * 4]
    # the same grid and brick geometry in both groups, and the brick stacks' tuning
    geom = [k for k in _lib.PLAN_FIELDS if k not in ("lds", "J", "view_off", "out_off")]
    assert {k: launches[0][k] for k in geom} == {k: launches[1][k] for k in geom}
    assert tuning == plan("zdft", jp=16, J=15, flags=0)[2]


def test_plan_at_jp32_up_to_16_joints_is_one_launch(lib):
    rc, launches, _ = plan(J=16)
    assert rc == 0 and len(launches) == 1
    assert launches[0]["name"] == "unproject_brick_kernel<16, false, float, float, true, 32>"
    assert (launches[0]["J"], launches[0]["view_off"], launches[0]["out_off"], launches[0]["grids"]) == (16, 0, 0, 0)


@pytest.mark.parametrize("cube,B", [(CUBE, 2), ((80, 80, 20), 1), ((80, 80, 20), 4), ((12, 20, 20), 3)])
def test_plan_at_jp16_is_the_zdft_entry(lib, cube, B):
    """field for field, name and tuning included: the same kernel on the same grid"""
    for J in (13, 15, 16):
        assert plan(jp=16, J=J, cube=cube, B=B) == plan("zdft", jp=16, J=J, cube=cube, B=B, flags=0)
        assert plan(jp=16, J=J, cube=cube, B=B)[0] == 0
    assert plan(jp=16, J=15)[1][0]["name"] == "unproject_brick_kernel<16, false, float, float, true, 16>"


def test_plan_refusals(lib):
    z = _lib.OUT_ZSPECTRUM
    assert plan()[0] == 0
    for other in (_lib.OUT_CHANNELS_LAST, _lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16 | _lib.OUT_BF16, _lib.HM_ONE_CHANNEL,
                  _lib.HM_WIDE_MASK):
        for jp, J in ((32, 20), (16, 16), (16, 4), (32, 4), (32, 1)):
            assert plan(jp=jp, J=J, flags=z | other)[0] == EUNSUPPORTED, (hex(other), jp, J)
    assert plan(layout=PLANAR, jp=17, J=17)[0] == EUNSUPPORTED                         # the planar layout
    assert plan(layout=PLANAR, jp=16, J=16)[0] == EUNSUPPORTED
    for jp, J in ((4, 4), (8, 8), (12, 12), (20, 17), (36, 17), (64, 17)):           # any other Jp
        assert plan(jp=jp, J=J)[0] == EUNSUPPORTED, jp
    assert plan(jp=32, J=33)[0] == EUNSUPPORTED and plan(jp=16, J=17)[0] == EUNSUPPORTED
    for cube in ((24, 16, 16), (24, 16, 24), (24, 16, 32), (24, 16, 40)):            # any other Z
        assert plan(cube=cube)[0] == EUNSUPPORTED and plan(jp=16, J=15, cube=cube)[0] == EUNSUPPORTED, cube
    for cube in ((22, 16, 20), (24, 18, 20), (23, 15, 20)):                          # X, Y multiples of 4
        assert plan(cube=cube)[0] == EUNSUPPORTED and plan(jp=16, J=15, cube=cube)[0] == EUNSUPPORTED, cube
    for h, w in ((18, 1), (1, 24), (4097, 4096)):                                    # 2 x 2 .. 2^24 pixels
        assert plan(h=h, w=w)[0] == EUNSUPPORTED and plan(jp=16, J=15, h=h, w=w)[0] == EUNSUPPORTED
    assert plan(h=2, w=2)[0] == 0 and plan(h=4096, w=4096)[0] == 0
    # the flag on the other entries
    sj = CUBE[0] * CUBE[1] * CUBE[2]
    for jp, J in ((32, 17), (16, 15)):
        assert plan("strided", jp=jp, J=J, strides=(J * sj, sj, CUBE[1] * CUBE[2], CUBE[2]))[0] == EUNSUPPORTED
        assert plan("train", jp=jp, J=J)[0] == EUNSUPPORTED
        assert plan("train", jp=jp, J=J, flags=z | _lib.HM_WIDE_MASK)[0] == EUNSUPPORTED
    assert plan("one_train", layout=PLANAR, jp=5, J=1)[0] == EUNSUPPORTED
    assert plan("one_train", layout=NHWC, jp=32, J=1)[0] == EUNSUPPORTED


def test_cabi_refusals_before_any_launch(lib):
    """SP3D_EUNSUPPORTED (-4) with pointers that are never dereferenced.  A library without the flag masks the bit off and
    LAUNCHES on these dummy pointers, so this runs only where no GPU is visible (tests/test_gpu_wide_front.py repeats the
    refusals with real tensors)."""
    if torch.cuda.is_available():
        pytest.skip("dummy-pointer refusals are checked only where no GPU is visible")
    gs = (C.c_float * 3)(8000, 8000, 2000)
    views = (C.c_void_p * 2)(0x1000, 0x1000)
    d, spec = C.c_void_p(0x1000), C.c_void_p(0x10000)
    z = _lib.OUT_ZSPECTRUM
    f, fi = lib.sp3d_unproject_fwd, lib.sp3d_unproject_fwd_indexed
    shape = (1, 2, 17, 8, 8, 8, 8, 20, gs, 96, 72, None)             # B, V, J, h, w, X, Y, Z, ...

    def both(layout, jp, cubes, grids, *tail):
        a = f(views, layout, jp, d, d, d, cubes, grids, *tail)
        b = fi(views, layout, jp, d, None, d, d, cubes, grids, *tail)
        c = fi(views, layout, jp, d, d, d, d, cubes, grids, *tail)          # with sample_of
        assert a == b == c, (a, b, c)
        return a

    for other in (_lib.OUT_CHANNELS_LAST, _lib.HM_BF16, _lib.OUT_BF16, _lib.HM_ONE_CHANNEL, _lib.HM_WIDE_MASK):
        assert both(NHWC | z | other, 32, spec, None, *shape) == -4, hex(other)
        assert both(NHWC | z | other, 16, spec, None, 1, 2, 16, 8, 8, 8, 8, 20, gs, 96, 72, None) == -4, hex(other)
    assert both(PLANAR | z, 17, spec, None, *shape) == -4                                        # the planar layout
    for jp in (4, 8, 12, 20, 36):                                                                # any other Jp
        assert both(NHWC | z, jp, spec, None, 1, 2, min(jp, 17), 8, 8, 8, 8, 20, gs, 96, 72, None) == -4, jp
    assert both(NHWC | z, 32, spec, None, 1, 2, 33, 8, 8, 8, 8, 20, gs, 96, 72, None) == -4       # J > Jp
    assert both(NHWC | z, 16, spec, None, 1, 2, 17, 8, 8, 8, 8, 20, gs, 96, 72, None) == -4
    for Z in (16, 24, 32):                                                                       # any other Z
        assert both(NHWC | z, 32, spec, None, 1, 2, 17, 8, 8, 8, 8, Z, gs, 96, 72, None) == -4, Z
    for X, Y in ((6, 8), (8, 10), (7, 7)):                                                       # X, Y multiples of 4
        assert both(NHWC | z, 32, spec, None, 1, 2, 17, 8, 8, X, Y, 20, gs, 96, 72, None) == -4, (X, Y)
    for h, w in ((1, 8), (8, 1), (4097, 4096)):                                                  # 2 x 2 .. 2^24 pixels
        assert both(NHWC | z, 32, spec, None, 1, 2, 17, h, w, 8, 8, 20, gs, 96, 72, None) == -4, (h, w)
    for jp, J in ((32, 17), (16, 15)):
        tail = (1, 2, J, 8, 8, 8, 8, 20, gs, 96, 72, None)
        assert both(NHWC | z, jp, spec, d, *tail) == -4                                          # a non-NULL grids
        for off in (4, 8, 16, 64):                                                               # a misaligned spectrum
            assert both(NHWC | z, jp, C.c_void_p(0x10000 + off), None, *tail) == -4, off
        # the flag on the other forward entries
        st = (C.c_int64 * 4)(J * 1280, 1280, 160, 20)
        assert lib.sp3d_unproject_fwd_strided(views, NHWC | z, jp, d, None, d, d, spec, st, *tail) == -4
        assert lib.sp3d_unproject_fwd_train(views, NHWC | z, jp, d, None, d, d, spec, None, d, *tail) == -4
        assert lib.sp3d_unproject_fwd_train(views, NHWC | z | _lib.HM_WIDE_MASK, jp, d, None, d, d, spec, None, d, *tail) == -4
    for layout, jp in ((PLANAR, 5), (NHWC, 32)):
        assert lib.sp3d_unproject_one_fwd_train(views, layout | z, jp, d, None, d, d, spec, None, d, 1, 2, 1, 8, 8, 8, 8, 20,
                                                gs, 96, 72, None) == -4
    # sp3d_unproject_fwd_zdft itself accepts what it accepted: Jp = 16 only
    assert lib.sp3d_unproject_fwd_zdft(views, 32, d, d, d, spec, 1, 2, 17, 8, 8, 8, 8, 20, gs, 96, 72, 28, None) == -4


def test_pins_that_must_not_move(lib):
    assert plan("zdft", jp=32, J=17, B=1, cube=(80, 80, 20), flags=0)[0] == EUNSUPPORTED
    assert plan("zdft", jp=32, J=16, flags=0)[0] == EUNSUPPORTED
    for cube, family in ((CUBE, "unproject_pipe_kernel"), ((24, 16, 32), "unproject_brick_kernel")):
        rc, launches, _ = plan(jp=32, J=21, cube=cube, flags=0)
        assert rc == 0 and [l["name"].split("<")[0] for l in launches] == [family] * 2
        assert [(l["J"], l["view_off"], l["out_off"], l["grids"]) for l in launches] == \
            [(16, 0, 0, 1), (5, 64, 16 * 24 * 16 * cube[2] * 4, 0)]
        assert launches[1]["name"].startswith(family + "<8, ") and launches[1]["name"].endswith(", 32>")
    rc, launches, _ = plan(jp=32, J=21, cube=(24, 16, 32), flags=0)
    assert [l["name"] for l in launches] == ["unproject_brick_kernel<16, false, float, float, false, 32>",
                                             "unproject_brick_kernel<8, false, float, float, false, 32>"]
    assert plan(jp=32, J=20, flags=_lib.OUT_CHANNELS_LAST)[0] == EUNSUPPORTED
    assert plan("train", jp=32, J=17, flags=0)[0] == EUNSUPPORTED


# ---- Python predicates, no GPU ------------------------------------------------------------------------------------------
def test_env_switch_is_read_as_the_others_are(monkeypatch):
    cfg = load_config(CAMPUS)
    for value, want in ((None, False), ("", False), ("0", False), ("1", True), ("yes", True)):
        if value is None:
            monkeypatch.delenv("SP3D_WIDE_FRONT", raising=False)
        else:
            monkeypatch.setenv("SP3D_WIDE_FRONT", value)
        assert ProjectLayer(cfg).wide_zspectrum is want, value
        assert V2VNet(17, 1).wide_front is want, value
        assert _lib.env_switch("SP3D_WIDE_FRONT", False) is want


def test_predicates_with_the_switch_off(monkeypatch):
    monkeypatch.delenv("SP3D_WIDE_FRONT", raising=False)
    net = V2VNet(17, 1).eval()
    assert net.wide_front is False
    with torch.no_grad():
        assert net.wants_zspectrum(80, 80, 20, 17) is None
        assert not net.wants_channels_last_cubes(80, 80, 20)
        net.wide_front = True                       # CPU weights: the fused front needs the GPU plan, switch or not
        assert net.wants_zspectrum(80, 80, 20, 17) is None
    assert (20, 28, 16) in _lib.ZDFT_SHAPES and len(_lib.ZDFT_SHAPES) == 1


class _Cuda:
    """stands where a GPU heat-map would: get_voxel_zspectrum refuses from shape and device flags, before any device access"""
    is_cuda, requires_grad, device = True, False, torch.device("cpu")

    def __init__(self, shape):
        self.shape = shape


def test_get_voxel_zspectrum_raises_at_17_joints_with_the_switch_off(monkeypatch):
    monkeypatch.delenv("SP3D_WIDE_FRONT", raising=False)
    cfg = load_config(CAMPUS)
    layer = ProjectLayer(cfg)
    assert layer.wide_zspectrum is False
    w, h = (int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    hms = [_Cuda((2, 17, h, w)) for _ in range(3)]
    with torch.no_grad(), pytest.raises(_lib.Sp3dError, match="13..16 joints only"):
        layer.get_voxel_zspectrum(hms, [], [8000.0, 8000.0, 2000.0], [[0.0, 0.0, 0.0]], [80, 80, 20], 28)
    for J in (33, 40):                              # ... and beyond 32 joints with it on
        layer.wide_zspectrum = True
        with torch.no_grad(), pytest.raises(_lib.Sp3dError, match="13..16 joints only"):
            layer.get_voxel_zspectrum([_Cuda((2, J, h, w))] * 3, [], [8000.0, 8000.0, 2000.0], [[0.0, 0.0, 0.0]], [80, 80, 20], 28)
