"""Host side of the 17..32-joint training pair (SP3D_HM_WIDE_MASK on sp3d_unproject_fwd_train, SP3D_SCATTER_WIDE on the two
packed scatters, ProjectLayer.wide_grad): the cases of tests/wide_grad_cases.py hold what tests/test_gpu_wide_grad.py relies
on, the flag values, the forward plan, the refusal order of the backward entries and the path decision.  No GPU: every C
call below is answered before a launch (the plan entry never launches; the backward calls all break a rule)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from selfpose3d_amd import _lib, build as sbuild
from selfpose3d_amd.project_layer import unproject_path
from tests import bwd_sweep_cases as sweep
from tests import wide_grad_cases as wide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "sp3d.h")) as fh:
        return fh.read()


# ---- the cases themselves -------------------------------------------------------------------------------------------
def test_case_table_is_the_documented_one():
    assert wide.CASES == list(range(100, 108))
    assert [wide.WIDE[i][3] for i in wide.CASES] == [17, 17, 20, 32, 21, 25, 29, 17]
    for idx in wide.CASES:
        c = wide.get(idx)
        assert c.idx == idx and (c.P, c.B, c.V, c.J, (c.w, c.h), c.cube, c.kind) == tuple(wide.WIDE[idx])
        assert 16 < c.J <= 32
    # the sweep's own table is untouched by building these
    assert len(sweep.cases()) == len(sweep.FIXED) + sweep.NUM_RANDOM + len(sweep.EXTRA)


@pytest.mark.parametrize("idx", wide.CASES, ids=wide.case_id)
def test_case_exercises_what_it_is_there_for(idx):
    c = wide.get(idx)
    planes = c.expected_mask_planes
    assert planes.shape == (2, c.P, c.N) and planes.dtype == np.uint16
    # the planes are expected_pass, bit for bit, and nothing else
    ep = c.expected_pass.reshape(c.P, c.J, c.N)
    for j in range(c.J):
        assert np.array_equal((planes[j // 16] >> (j % 16)) & 1, ep[:, j].astype(np.uint16))
    assert not (planes[1] >> (c.J - 16)).any()                       # bits at or above J - 16 in plane 1
    assert not planes[:, c.valid == 0].any()                         # both planes of an invalid cube
    seen = c.seen.reshape(c.P, c.N) & (c.valid[:, None] > 0)
    if idx in (101, 102, 103, 104, 106, 107):
        for grp, lo, hi in ((0, 0, 16), (1, 16, c.J)):
            sel = ep[:, lo:hi][np.broadcast_to(seen[:, None], ep[:, lo:hi].shape)]
            assert sel.any() and not sel.all(), (idx, grp)             # passing AND blocked voxels that some view sees
    assert np.abs(c.ref[:, :, 16:]).max() > 0                        # the second group has a gradient to scatter
    assert sweep.auto_takes_merge(c.cube, c.grid_size) == (idx in (103, 104, 106))
    if idx in (104, 106):
        assert (c.valid == 0).any()
    if idx == 106:
        assert not c.owns_valid[1] and c.owns_valid[0]
        assert not c.ref[:, 1].any()


# ---- the flag bits --------------------------------------------------------------------------------------------------
def test_flag_values_match_the_header():
    hdr = _header()
    val = lambda name: int(re.search(r"\b%s\s*=\s*(0x[0-9a-fA-F]+|\d+)" % name, hdr).group(1), 0)
    assert val("SP3D_HM_WIDE_MASK") == 0x1000 == _lib.HM_WIDE_MASK
    assert val("SP3D_SCATTER_WIDE") == 0x100 == _lib.SCATTER_WIDE
    # the layout-word scan of tests/test_one_channel_host.py sees the first and not the second
    scanned = dict(re.findall(r"\b(SP3D_(?:HM|OUT|LAYOUT)_[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", hdr))
    assert "SP3D_HM_WIDE_MASK" in scanned and "SP3D_SCATTER_WIDE" not in scanned
    assert _lib.SCATTER_WIDE & 0xff == 0
    for s in (_lib.SCATTER_AUTO, _lib.SCATTER_PER_TAP, _lib.SCATTER_MERGE):
        assert 0 <= s < 0x100


# ---- the forward plan -----------------------------------------------------------------------------------------------
WIDE_NHWC = _lib.LAYOUT_NHWC | _lib.HM_WIDE_MASK


def _plan(entry, layout, jp, J, cube, h=18, w=24, B=2, V=3):
    return _lib.unproject_fwd_plan(entry, layout, jp, B, V, J, h, w, cube)


def test_training_plan_with_the_wide_mask(lib):
    rc, launches, _ = _plan("train", WIDE_NHWC, 32, 21, (24, 16, 20))
    assert rc == 0 and len(launches) == 2
    assert all(l["name"].startswith("unproject_pipe_kernel<") for l in launches), [l["name"] for l in launches]
    assert [l["J"] for l in launches] == [16, 5]
    assert [l["view_off"] for l in launches] == [0, 64]
    assert [l["out_off"] for l in launches] == [0, 16 * 24 * 16 * 20 * 4]
    assert [l["grids"] for l in launches] == [1, 0]
    # the inference forward plans the same two launches (the mask is a runtime branch of the same kernels)
    rc_i, inf, _ = _plan("indexed", _lib.LAYOUT_NHWC, 32, 21, (24, 16, 20))
    assert rc_i == 0 and inf == launches
    rc, launches, _ = _plan("train", WIDE_NHWC, 32, 21, (24, 16, 32))
    assert rc == 0 and len(launches) == 2
    assert all(l["name"].startswith("unproject_brick_kernel<") for l in launches), [l["name"] for l in launches]
    assert [l["J"] for l in launches] == [16, 5]
    rc, launches, _ = _plan("train", WIDE_NHWC, 32, 16, (24, 16, 20))
    assert rc == 0 and len(launches) == 1 and launches[0]["J"] == 16
    rc, launches, _ = _plan("train", WIDE_NHWC, 32, 1, (24, 16, 20))
    assert rc == 0 and len(launches) == 1 and launches[0]["J"] == 1


def test_training_plan_refusals(lib):
    cube = (24, 16, 20)
    assert _plan("train", _lib.LAYOUT_NHWC, 32, 21, cube)[0] == -4                   # without the flag: as before
    assert _plan("train", _lib.LAYOUT_NHWC | _lib.HM_WIDE_MASK, 16, 15, cube)[0] == -4
    assert _plan("train", _lib.LAYOUT_NHWC | _lib.HM_WIDE_MASK, 16, 16, cube)[0] == -4
    assert _plan("train", WIDE_NHWC | _lib.OUT_CHANNELS_LAST, 32, 20, cube)[0] == -4
    assert _plan("train", WIDE_NHWC | _lib.HM_BF16, 32, 21, cube)[0] == -4
    assert _plan("train", WIDE_NHWC | _lib.OUT_BF16, 32, 21, cube)[0] == -4
    assert _plan("train", WIDE_NHWC | _lib.HM_ONE_CHANNEL, 32, 1, cube)[0] == -4
    assert _plan("train", WIDE_NHWC, 32, 21, cube, h=18, w=1)[0] == -4
    assert _plan("train", WIDE_NHWC, 32, 33, cube)[0] == -4
    assert _plan("train", _lib.LAYOUT_PLANAR | _lib.HM_WIDE_MASK, 32, 21, cube)[0] == -4
    for entry in ("indexed", "strided", "zdft", "one_train"):
        assert _plan(entry, WIDE_NHWC, 32, 21, cube)[0] == -4, entry
    assert _plan("one_train", WIDE_NHWC, 32, 1, cube)[0] == -4
    # the same requests without the flag keep their answers: the inference entries plan, the 16-channel training forward plans
    assert _plan("indexed", _lib.LAYOUT_NHWC, 32, 21, cube)[0] == 0
    assert _plan("strided", _lib.LAYOUT_NHWC, 32, 21, cube)[0] == 0
    assert _plan("train", _lib.LAYOUT_NHWC, 16, 15, cube)[0] == 0
    assert _plan("one_train", _lib.LAYOUT_NHWC, 32, 1, cube)[0] == 0


# ---- the backward entries -------------------------------------------------------------------------------------------
def test_wide_scatter_refusal_order(lib):
    """Every call is at Jp = 32, carries the flag bit or breaks an earlier rule, so a library that does not know the flag
    refuses each of them too (it reads 0x100 as an unknown scatter): nothing here can launch, whichever library answers."""
    hdr = _header()
    EINVAL, ENULL, ERANGE, EUNSUPPORTED = (int(re.search(name + r"\s*=\s*(-?\d+)", hdr).group(1))
                                           for name in ("SP3D_EINVAL", "SP3D_ENULL", "SP3D_ERANGE", "SP3D_EUNSUPPORTED"))
    gs = (C.c_float * 3)(2000, 2000, 2000)
    d = C.c_void_p(0x1000)
    W = _lib.SCATTER_WIDE

    def packed(det):
        f = lib.sp3d_unproject_bwd_packed_det if det else lib.sp3d_unproject_bwd_packed

        def call(cam=d, mask=d, scale=d, B=1, V=2, J=17, Jp=32, w=8, X=4, scatter=W):
            return f(cam, None, d, d, d, mask, d, *((scale,) if det else ()), B, 1, V, J, Jp, 8, w, X, 4, 4, gs, 96, 72, scatter, None)
        return call

    for f in (packed(False), packed(True)):
        # the low byte keeps its meaning, nothing lives above the flag
        assert f(scatter=W | 1) == EINVAL and f(scatter=W | 4) == EINVAL and f(scatter=0x200) == EINVAL
        assert f(scatter=W | 0x200) == EINVAL and f(scatter=W | 0x10000) == EINVAL and f(scatter=-1) == EINVAL
        # without the flag Jp = 32 is refused as before, whatever the choice
        for s in (_lib.SCATTER_AUTO, _lib.SCATTER_PER_TAP, _lib.SCATTER_MERGE):
            assert f(scatter=s) == EUNSUPPORTED
        # with it: Jp must be 32 (Jp = 16 at J = 15 is a call the plain entry would launch), J <= 32, the map at least 2x2
        assert f(Jp=16, J=15) == EUNSUPPORTED and f(Jp=16, J=15, cam=None) == ENULL
        for s in (0, _lib.SCATTER_PER_TAP, _lib.SCATTER_MERGE):
            assert f(Jp=16, J=15, scatter=W | s, w=1) == EUNSUPPORTED
        assert f(w=1) == EUNSUPPORTED
        assert f(Jp=36, J=33) == EUNSUPPORTED and f(Jp=32, J=33, w=1) == EUNSUPPORTED
        # the order: geometry, B, scatter, pointers, unsupported
        assert f(cam=None) == ENULL and f(mask=None) == ENULL
        assert f(cam=None, w=1) == ENULL and f(mask=None, Jp=36, J=33) == ENULL            # a NULL pointer before the unsupported refusals
        assert f(scatter=W | 1, cam=None, w=1) == EINVAL                                # scatter before the pointers
        assert f(B=0, scatter=W | 1, cam=None) == EINVAL and f(B=0, cam=None, w=1) == EINVAL
        assert f(V=17, B=0, cam=None, w=1) == EINVAL and f(X=0, scatter=0x200) == EINVAL
    det = packed(True)
    assert det(scale=None) == ENULL and det(scale=None, V=0) == ENULL and det(scale=None, scatter=W | 1) == ENULL
    assert det(scale=None, B=0, w=1) == ENULL


# ---- the path decision ----------------------------------------------------------------------------------------------
def test_path_decision_switch_off_is_todays():
    for J in (1, 15, 16):
        for grad in (False, True):
            assert unproject_path(J, grad, 72, 96, "auto", False) == "nhwc"
            assert unproject_path(J, grad, 72, 96, "nhwc", False) == "nhwc"
            assert unproject_path(J, grad, 1, 96, "auto", False) == "planar"
    for J in (17, 20, 32):
        assert unproject_path(J, False, 72, 96, "auto", False) == "nhwc"
        assert unproject_path(J, True, 72, 96, "auto", False) == "planar"
        assert unproject_path(J, False, 72, 96, "nhwc", False) == "nhwc"
        with pytest.raises(_lib.Sp3dError, match="16 joints"):
            unproject_path(J, True, 72, 96, "nhwc", False)
        assert unproject_path(J, True, 72, 96, "planar", False) == "planar"
    assert unproject_path(33, False, 72, 96, "auto", False) == "planar"
    assert unproject_path(33, True, 72, 96, "auto", False) == "planar"
    with pytest.raises(_lib.Sp3dError, match="16 joints"):
        unproject_path(33, True, 72, 96, "nhwc", False)


def test_path_decision_switch_on():
    for J in (17, 20, 32):
        assert unproject_path(J, True, 72, 96, "auto", True) == "nhwc"
        assert unproject_path(J, True, 72, 96, "nhwc", True) == "nhwc"
        assert unproject_path(J, False, 72, 96, "auto", True) == "nhwc"
        assert unproject_path(J, True, 72, 96, "planar", True) == "planar"
        assert unproject_path(J, True, 1, 96, "auto", True) == "planar"             # below 2x2: no NHWC kernels at all
        with pytest.raises(_lib.Sp3dError, match="16 joints"):
            unproject_path(J, True, 72, 1, "nhwc", True)
    # at most 16 joints and above 32 the switch changes nothing
    for J in (1, 16):
        assert unproject_path(J, True, 72, 96, "auto", True) == "nhwc"
    assert unproject_path(33, True, 72, 96, "auto", True) == "planar"
    assert unproject_path(33, False, 72, 96, "auto", True) == "planar"
    with pytest.raises(_lib.Sp3dError, match="16 joints"):
        unproject_path(33, True, 72, 96, "nhwc", True)


def test_layer_switch_is_off_by_default_and_settable(monkeypatch):
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer
    cfg = load_config(os.path.join(ROOT, "configs", "campus_synthetic_coco17_cam3.yaml"))
    monkeypatch.delenv("SP3D_WIDE_GRAD", raising=False)
    layer = ProjectLayer(cfg)
    assert layer.wide_grad is False
    layer.wide_grad = True
    assert layer.wide_grad is True
    monkeypatch.setenv("SP3D_WIDE_GRAD", "1")
    assert ProjectLayer(cfg).wide_grad is True
    monkeypatch.setenv("SP3D_WIDE_GRAD", "0")
    assert ProjectLayer(cfg).wide_grad is False
