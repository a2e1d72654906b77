"""The one-channel z-spectrum front (SP3D_HM_ONE_ZSPECTRUM, ``SP3D_ONE_FRONT``) without a GPU: the flag, the launch
resolve_fwd plans for it (sp3d_unproject_fwd_plan), every refusal the header lists - through the plan where a plan entry
exists and through the C entries with pointers that are never dereferenced -, the pins that must not move, and the Python
switches and predicates.  tests/test_gpu_one_front.py holds the values."""
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
NHWC, PLANAR = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
EINVAL, EUNSUPPORTED = -1, -4
CUBE = (12, 20, 20)
BLOCK, LDS = 320, 16 * 20 * 4                  # five waves, a slab of 16 columns x 20 floats


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def plan(entry="indexed", layout=PLANAR, jp=15, B=2, V=3, J=1, h=18, w=24, cube=CUBE, flags=None, strides=None):
    flags = _lib.HM_ONE_ZSPECTRUM if flags is None else flags
    return _lib.unproject_fwd_plan(entry, layout | flags, jp, B, V, J, h, w, cube, 0, strides)


def test_flag_abi_version_and_entry_list():
    from tests.test_glue_sweep_reference import LEDGER, _header_signatures
    with open(os.path.join(ROOT, "include", "sp3d.h")) as fh:
        hdr = fh.read()
    assert int(re.search(r"\bSP3D_HM_ONE_ZSPECTRUM\s*=\s*(0x[0-9a-fA-F]+)", hdr).group(1), 0) == 0x4000 == _lib.HM_ONE_ZSPECTRUM
    assert "SP3D_ABI_VERSION 3" in hdr and _lib.ABI_VERSION == 3
    # the feature is a flag bit, not a symbol: the header declares what the ledger lists, no more
    assert sorted(_header_signatures(os.path.join(ROOT, "include", "sp3d.h"))) == sorted(LEDGER)
    assert len(_lib.SIGNATURES) == 57


@pytest.mark.parametrize("cube", [(12, 20, 20), (80, 80, 20)])
@pytest.mark.parametrize("V,name", [(3, "unproject_one_zd_kernel<3, 4>"), (5, "unproject_one_zd_kernel<5, 4>"),
                                    (7, "unproject_one_zd_kernel<8, 4>"), (16, "unproject_one_zd_kernel<16, 8>")])
def test_plan_is_one_launch_of_the_new_kernel(lib, cube, V, name):
    X, Y, _ = cube
    h, w = 18, 24
    for entry in ("indexed",):                 # sp3d_unproject_fwd is the indexed entry with sample_of = NULL (one plan entry)
        for B in (1, 3, 4):
            for layout in (PLANAR, NHWC):
                for jp in (1, 15, 16, 32):
                    rc, launches, _ = plan(entry, layout, jp, B=B, V=V, cube=cube, h=h, w=w)
                    assert rc == 0 and len(launches) == 1, (rc, layout, jp, B)
                    l = launches[0]
                    assert l["name"] == name
                    assert l["workgroups"] == B * (X // 4) * (Y // 4)
                    assert (l["block"], l["lds"]) == (BLOCK, LDS)
                    assert (l["J"], l["grids"], l["view_off"], l["out_off"]) == (1, 0, 0, 0)
                    # sample, row and pixel stride in elements: the addressing of SP3D_HM_ONE_CHANNEL
                    want = (h * w * jp, w * jp, jp) if layout == NHWC else (jp * h * w, w, 1)
                    assert (l["nscalars"], l["s0"], l["s1"], l["s2"]) == (3,) + want
                    # ... which the one-channel flag's own plan carries for the same request
                    one = plan(entry, layout, jp, B=B, V=V, cube=cube, h=h, w=w, flags=_lib.HM_ONE_CHANNEL)[1][0]
                    assert (one["s0"], one["s1"], one["s2"]) == want
                    assert (l["bk_nxy"], l["bk_nby"], l["xm_tiles"]) == ((X // 4) * (Y // 4), Y // 4, (X // 4) * (Y // 4))


def test_plan_refusals(lib):
    z = _lib.HM_ONE_ZSPECTRUM
    assert plan()[0] == 0
    for other in (_lib.OUT_CHANNELS_LAST, _lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16 | _lib.OUT_BF16, _lib.HM_ONE_CHANNEL,
                  _lib.HM_WIDE_MASK, _lib.OUT_ZSPECTRUM):
        for layout, jp in ((PLANAR, 15), (NHWC, 16), (NHWC, 32)):
            assert plan(layout=layout, jp=jp, flags=z | other)[0] == EUNSUPPORTED, (hex(other), layout, jp)
    for J in (2, 4, 15, 16, 17):                                                         # J != 1
        assert plan(J=J)[0] == EUNSUPPORTED and plan(layout=NHWC, jp=16, J=J)[0] == EUNSUPPORTED, J
    for cube in ((12, 20, 16), (12, 20, 24), (12, 20, 32), (12, 20, 40)):               # any other Z
        assert plan(cube=cube)[0] == EUNSUPPORTED, cube
    for cube in ((10, 20, 20), (12, 18, 20), (11, 19, 20)):                             # X, Y multiples of 4
        assert plan(cube=cube)[0] == EUNSUPPORTED, cube
    for h, w in ((18, 1), (1, 24), (4097, 4096)):                                       # 2 x 2 .. 2^24 pixels
        assert plan(h=h, w=w)[0] == EUNSUPPORTED and plan(layout=NHWC, jp=16, h=h, w=w)[0] == EUNSUPPORTED
    assert plan(h=2, w=2)[0] == 0 and plan(h=4096, w=4096)[0] == 0
    assert plan(layout=NHWC, jp=31, h=4096, w=4096)[0] == 0                              # a sample below 2^31 bytes fits ...
    assert plan(layout=NHWC, jp=33, h=4096, w=4096)[0] == EUNSUPPORTED                  # ... one of more than 2^31 bytes does not
    assert plan(layout=NHWC, jp=1 << 20, h=18, w=24)[0] == EUNSUPPORTED                 # a row of 2^24 elements or more
    # SP3D_EINVAL as the one-channel flag answers
    for jp in (0, -1):
        assert plan(jp=jp)[0] == EINVAL and plan(layout=NHWC, jp=jp)[0] == EINVAL
        assert plan(jp=jp, flags=_lib.HM_ONE_CHANNEL)[0] == EINVAL
    for layout in (2, 3, 0xff):
        assert plan(layout=layout)[0] == EINVAL and plan(layout=layout, flags=_lib.HM_ONE_CHANNEL)[0] == EINVAL
    # the flag on the other entries
    sj = CUBE[0] * CUBE[1] * CUBE[2]
    for layout, jp in ((PLANAR, 15), (NHWC, 16)):
        assert plan("strided", layout, jp, strides=(sj, sj, CUBE[1] * CUBE[2], CUBE[2]))[0] == EUNSUPPORTED
        assert plan("strided", layout, jp)[0] == EUNSUPPORTED
        assert plan("train", layout, jp)[0] == EUNSUPPORTED
        assert plan("zdft", layout, jp)[0] == EUNSUPPORTED and plan("zdft", NHWC, 16, J=15)[0] == EUNSUPPORTED
        assert plan("one_train", layout, jp)[0] == EUNSUPPORTED


def test_cabi_refusals_before_any_launch(lib):
    """SP3D_EUNSUPPORTED (-4) / SP3D_EINVAL (-1) with pointers that are never dereferenced.  A library without the flag masks
    the bit off and LAUNCHES on these dummy pointers, so this runs only where no GPU is visible
    (tests/test_gpu_one_front.py repeats the refusals with real tensors)."""
    if torch.cuda.is_available():
        pytest.skip("dummy-pointer refusals are checked only where no GPU is visible")
    gs = (C.c_float * 3)(8000, 8000, 2000)
    views = (C.c_void_p * 2)(0x1000, 0x1000)
    d, spec = C.c_void_p(0x1000), C.c_void_p(0x10000)
    z = _lib.HM_ONE_ZSPECTRUM
    f, fi = lib.sp3d_unproject_fwd, lib.sp3d_unproject_fwd_indexed

    def both(layout, jp, cubes, grids, J=1, hw=(8, 8), cube=(8, 8, 20)):
        tail = (1, 2, J, hw[0], hw[1], *cube, gs, 96, 72, None)
        a = f(views, layout, jp, d, d, d, cubes, grids, *tail)
        b = fi(views, layout, jp, d, None, d, d, cubes, grids, *tail)
        c = fi(views, layout, jp, d, d, d, d, cubes, grids, *tail)          # with sample_of
        assert a == b == c, (a, b, c)
        return a

    for layout, jp in ((PLANAR, 15), (NHWC, 16)):
        for other in (_lib.OUT_CHANNELS_LAST, _lib.HM_BF16, _lib.OUT_BF16, _lib.HM_ONE_CHANNEL, _lib.HM_WIDE_MASK,
                      _lib.OUT_ZSPECTRUM):
            assert both(layout | z | other, jp, spec, None) == -4, hex(other)
        for J in (2, 4, 16):
            assert both(layout | z, jp, spec, None, J=J) == -4, J
        for Z in (16, 24, 32):
            assert both(layout | z, jp, spec, None, cube=(8, 8, Z)) == -4, Z
        for X, Y in ((6, 8), (8, 10), (7, 7)):
            assert both(layout | z, jp, spec, None, cube=(X, Y, 20)) == -4, (X, Y)
        for hw in ((1, 8), (8, 1), (4097, 4096)):
            assert both(layout | z, jp, spec, None, hw=hw) == -4, hw
        assert both(layout | z, jp, spec, d) == -4                                               # a non-NULL grids
        for off in (4, 8, 16, 64):                                                               # a misaligned spectrum
            assert both(layout | z, jp, C.c_void_p(0x10000 + off), None) == -4, off
        assert both(layout | z, 0, spec, None) == -1                                             # Jp < 1
        # the flag on the other forward entries
        tail = (1, 2, 1, 8, 8, 8, 8, 20, gs, 96, 72, None)
        st = (C.c_int64 * 4)(1280, 1280, 160, 20)
        assert lib.sp3d_unproject_fwd_strided(views, layout | z, jp, d, None, d, d, spec, st, *tail) == -4
        assert lib.sp3d_unproject_fwd_train(views, layout | z, jp, d, None, d, d, spec, None, d, *tail) == -4
        assert lib.sp3d_unproject_one_fwd_train(views, layout | z, jp, d, None, d, d, spec, None, d, *tail) == -4
    assert both(NHWC | z, 33, spec, None, hw=(4096, 4096)) == -4                                 # a sample of more than 2^31 bytes
    assert both(2 | z, 15, spec, None) == -1 and both(0xff | z, 15, spec, None) == -1            # neither PLANAR nor NHWC


def test_pins_that_must_not_move(lib):
    """the older pair, the one-channel kernel's plan and the 13..16-joint z-spectrum plan are what they were"""
    pair = _lib.HM_ONE_CHANNEL | _lib.OUT_ZSPECTRUM
    for layout, jp, J in ((NHWC, 16, 1), (NHWC, 32, 1), (PLANAR, 15, 1), (NHWC, 16, 4)):
        assert plan(layout=layout, jp=jp, J=J, flags=pair)[0] == EUNSUPPORTED
    rc, launches, _ = plan(flags=_lib.HM_ONE_CHANNEL, V=5, cube=(80, 80, 20), B=4)
    assert rc == 0 and [(l["name"], l["block"], l["lds"]) for l in launches] == [("unproject_one_kernel<5, 4, false>", 64, 0)]
    rc, launches, _ = plan(layout=NHWC, jp=16, J=15, flags=_lib.OUT_ZSPECTRUM, cube=(80, 80, 20))
    assert rc == 0 and [l["name"] for l in launches] == ["unproject_brick_kernel<16, false, float, float, true, 16>"]
    assert (20, 28, 16) in _lib.ZDFT_SHAPES and len(_lib.ZDFT_SHAPES) == 1


# ---- Python switches and predicates, no GPU -----------------------------------------------------------------------------
def test_env_switch_is_read_as_the_others_are(monkeypatch):
    cfg = load_config(None)
    for value, want in ((None, False), ("", False), ("0", False), ("1", True), ("yes", True)):
        if value is None:
            monkeypatch.delenv("SP3D_ONE_FRONT", raising=False)
        else:
            monkeypatch.setenv("SP3D_ONE_FRONT", value)
        assert ProjectLayer(cfg).one_zspectrum is want, value
        assert V2VNet(1, 1).one_front is want, value
        assert _lib.env_switch("SP3D_ONE_FRONT", False) is want


def test_predicate_without_a_gpu_plan(monkeypatch):
    monkeypatch.delenv("SP3D_ONE_FRONT", raising=False)
    net = V2VNet(1, 1).eval().to(memory_format=torch.channels_last_3d)
    assert net.one_front is False
    with torch.no_grad():
        assert net.wants_zspectrum(80, 80, 20, 1) is None
        net.one_front = True                        # CPU weights: the fused front needs the GPU plan, switch or not
        assert net.wants_zspectrum(80, 80, 20, 1) is None
    assert net.wants_zspectrum(80, 80, 20, 1) is None       # ... nor with grad enabled


class _Cuda:
    """stands where a GPU heat-map would: get_voxel_zspectrum refuses from shapes, strides and device flags, before any
    device access; everything the refusals read is answered by a CPU tensor"""
    is_cuda, requires_grad = True, False

    def __init__(self, t):
        self.t, self.shape, self.dtype, self.device = t, t.shape, t.dtype, t.device

    def dim(self):
        return self.t.dim()

    def stride(self):
        return self.t.stride()


ARGS = ([], [8000.0, 8000.0, 2000.0], [[0.0, 0.0, 0.0]], [80, 80, 20], 28)


def test_get_voxel_zspectrum_raises_as_before(monkeypatch):
    monkeypatch.delenv("SP3D_ONE_FRONT", raising=False)
    cfg = load_config(None)
    layer = ProjectLayer(cfg)
    assert layer.one_zspectrum is False
    w, h = (int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    full = [torch.zeros(2, 15, h, w) for _ in range(3)]
    one = [_Cuda(a[:, 2:3]) for a in full]
    with torch.no_grad(), pytest.raises(_lib.Sp3dError, match="13..16 joints only"):        # the switch off: today's error
        layer.get_voxel_zspectrum(one, *ARGS)
    layer.one_zspectrum = True
    expanded = [_Cuda(torch.zeros(1, 1, h, w).expand(2, 1, h, w)) for _ in range(3)]           # stride 0: does not classify
    two = [_Cuda(a[:, 2:4]) for a in full]                                                     # J = 2
    other_dtype = [_Cuda(a[:, 2:3].double()) for a in full]
    for bad in (expanded, two, other_dtype):
        with torch.no_grad(), pytest.raises(_lib.Sp3dError, match="13..16 joints only"):
            layer.get_voxel_zspectrum(bad, *ARGS)
    layer.mode = "planar"
    with torch.no_grad(), pytest.raises(_lib.Sp3dError, match="13..16 joints only"):
        layer.get_voxel_zspectrum(one, *ARGS)
