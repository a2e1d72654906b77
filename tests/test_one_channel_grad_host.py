"""The one-channel training pair without a GPU: the cases of tests/one_channel_grad_cases.py are sound (the oracle on the
J = 1 slice is channel rid of the J-channel oracle), the three new entries of the C ABI are declared once and refuse before
any launch, the launch plan answers for the new forward entry, and the switch of ProjectLayer is off by default."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from selfpose3d_amd import _lib, build as sbuild
from tests import bwd_sweep_cases as sweep
from tests import one_channel_grad_cases as cases
from tests.test_host_cabi import _table_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NHWC, PLANAR = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
EINVAL, ENULL, ERANGE, EUNSUPPORTED = -1, -2, -3, -4
NEW = ("sp3d_unproject_one_fwd_train", "sp3d_unproject_one_bwd", "sp3d_unproject_one_bwd_det")


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


# ---- the cases ------------------------------------------------------------------------------------------------------------
def test_case_list_wraps_the_whole_sweep_and_adds_twelve_views():
    idx = cases.indices()
    assert idx[:-1] == list(range(len(sweep.cases()))) and idx[-1] == cases.OWN_IDX
    assert cases.OWN[2] == 12 and not any(c[2] == 12 for c in sweep.cases())
    assert {17, 20} <= {c[3] for c in sweep.cases()}                   # the J > 16 cases are wrapped too
    assert len({cases.case_id(i) for i in idx}) == len(idx)


@pytest.mark.parametrize("idx", [0, 3, 12])
def test_own_case_recipe_is_the_sweeps(idx):
    """the helper's copy of the recipe, given a sweep specification, builds the sweep's case"""
    mine, theirs = cases._OwnCase(idx, sweep.cases()[idx]), sweep.get(idx)
    for k in ("cam", "sample_of", "centers", "valid", "grad", "cam_p", "owns_valid"):
        assert np.array_equal(getattr(mine, k), getattr(theirs, k)), k
    assert all(np.array_equal(a, b) for a, b in zip(mine.hms, theirs.hms))
    assert (mine.grid_size, mine.T, mine.det_step, mine.img) == (theirs.grid_size, theirs.T, theirs.det_step, theirs.img)


@pytest.mark.parametrize("idx", [0, 1, 3, 7, 9, cases.OWN_IDX])
def test_slicing_is_sound_on_the_oracle(idx):
    """channels are independent: the oracle on the contiguous J = 1 slice gives channel rid of the J-channel oracle, forward bit
    for bit and backward exactly (the same float64 additions in the same order)"""
    c = cases.get(idx)
    b = c.base
    assert c.rid == idx % b.J and c.grad.shape == (c.P, 1) + tuple(c.cube)
    hms_p = [x[c.sample_of] for x in c.hms_one]
    fwd = b.oracle_fwd(hms_p)
    assert fwd.shape == c.fwd.shape and np.array_equal(fwd, c.fwd)
    rows = b.to_samples(b.oracle_bwd_rows(hms_p, c.grad))
    assert rows.shape == c.ref.shape and np.array_equal(rows, c.ref)
    assert np.array_equal(b.to_samples(b.oracle_bwd_rows(hms_p, np.abs(c.grad))), c.S)
    # the mask: bit 0 only, zero rows for invalid cubes, and it is the clamp's pass set of the sliced forward
    m = c.expected_mask
    assert m.dtype == np.uint16 and m.shape == (c.P, c.N) and int(m.max()) <= 1 and not m[c.valid == 0].any()
    q, neg = b.oracle_fwd([0.25 * x for x in hms_p]), b.oracle_fwd([-0.25 * x for x in hms_p])
    want = (c.valid[:, None] > 0) & ~(4.0 * q[:, 0].reshape(c.P, c.N) > 1.0) & ~(neg[:, 0].reshape(c.P, c.N) > 0.0)
    assert np.array_equal(m.astype(bool), want)
    assert c.det_step == 2.0 ** (np.ceil(np.log2(np.abs(b.grad[:, c.rid]).max())) - 40) and c.det_step <= b.det_step
    assert c.T == b.T


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_once_and_match_their_header():
    """the three entries are lines of the binding's one table (tests/test_host_cabi.py holds it against include/sp3d.h, both
    ways); the ABI version is unchanged, and the launch plan knows the new forward entry"""
    assert set(NEW) <= set(_lib.SIGNATURES) and not set(NEW) & set(_lib.TUNING_SIGNATURES)
    with open(os.path.join(ROOT, "include", "sp3d.h")) as fh:
        text = fh.read()
    assert "#define SP3D_ABI_VERSION 3" in text
    assert _lib.PLAN_ENTRIES[:5] == ("indexed", "strided", "train", "zdft", "variant") and _lib.PLAN_ENTRIES[5] == "one_train"
    with open(os.path.join(ROOT, "selfpose3d_amd", "csrc", "sp3d_tuning.h")) as fh:
        tuning = fh.read()
    assert "SP3D_PLAN_ZDFT, SP3D_PLAN_TUNING, SP3D_PLAN_ONE_TRAIN }" in tuning


def test_both_flavours_export_and_declare_the_new_entries(lib):
    nopk = C.CDLL(_lib.NOPK_LIB_PATH)
    for name, (restype, argtypes) in _table_signatures({n: _lib.SIGNATURES[n] for n in NEW}).items():
        assert hasattr(nopk, name), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.sp3d_abi_version() == 3


def test_refusals_before_any_launch(lib):
    """every call below must come back with its status and pointers that are never dereferenced: run only where no GPU is
    visible, as tests/test_one_channel_host.py does (tests/test_gpu_one_channel_grad.py repeats them with real tensors)"""
    if torch.cuda.is_available():
        pytest.skip("dummy-pointer refusals are checked only where no GPU is visible")
    one = _lib.HM_ONE_CHANNEL
    gs = (C.c_float * 3)(8000, 8000, 2000)
    views = (C.c_void_p * 2)(0x1000, 0x1000)
    d = C.c_void_p(0x1000)
    ft, fb, fd = lib.sp3d_unproject_one_fwd_train, lib.sp3d_unproject_one_bwd, lib.sp3d_unproject_one_bwd_det

    def fwd(layout=NHWC, flags=0, jp=16, J=1, V=2, h=8, w=8, cam=d, cubes=d, mask=d, hm=views):
        return ft(hm, layout | flags, jp, cam, None, d, d, cubes, None, mask, 1, V, J, h, w, 4, 4, 4, gs, 96, 72, None)
    for layout, jp in ((PLANAR, 15), (NHWC, 16), (NHWC, 17)):
        for flag in (0, one):                                                            # the flag is accepted and implied
            for J in (2, 3, 5, 16):                                                      # J is 1 or 4
                assert fwd(layout, flag, jp, J) == EUNSUPPORTED, (layout, J)
            assert fwd(layout, flag | _lib.OUT_CHANNELS_LAST, jp, 1) == EUNSUPPORTED     # a channels-last result has 4 channels
            for J in (1, 4):
                assert fwd(layout, flag | _lib.OUT_BF16, jp, J) == EUNSUPPORTED          # fp32 storage only
                assert fwd(layout, flag | _lib.HM_BF16, jp, J) == EUNSUPPORTED
                assert fwd(layout, flag, jp, J, h=8, w=1) == EUNSUPPORTED                # heat-maps of at least 2x2 pixels
                assert fwd(layout, flag, jp, J, h=1, w=8) == EUNSUPPORTED
                assert fwd(layout, flag, jp, J, V=17) == EINVAL                          # at most SP3D_MAX_VIEWS views
                assert fwd(layout, flag, jp, J, mask=None) == ENULL                      # the mask is what the entry is for
                assert fwd(layout, flag, jp, J, cubes=None) == ENULL
                assert fwd(layout, flag, jp, J, cam=None) == ENULL
                assert fwd(layout, flag, jp, J, hm=None) == ENULL
        assert fwd(layout, 0, 0, 1) == EINVAL                                            # no channel to read
    assert fwd(PLANAR, 0, 1, 1, h=4097, w=4096) == EUNSUPPORTED                          # ... of at most 2^24 pixels
    assert fwd(NHWC, 0, 64, 1, h=4096, w=2048) == EUNSUPPORTED                           # a sample beyond 32-bit byte offsets
    assert fwd(7, 0, 16, 1) == EINVAL                                                    # unknown layout

    N = 64

    def bwd(det, stride=N, V=2, h=8, w=8, B=1, cam=d, grad=d, mask=d, acc=d, scale=d, cube=(4, 4, 4)):
        if det:
            return fd(cam, None, d, d, grad, stride, mask, acc, scale, B, 1, V, h, w, *cube, gs, 96, 72, None)
        return fb(cam, None, d, d, grad, stride, mask, acc, B, 1, V, h, w, *cube, gs, 96, 72, None)
    for det in (False, True):
        assert bwd(det, h=8, w=1) == EUNSUPPORTED and bwd(det, h=1, w=8) == EUNSUPPORTED
        assert bwd(det, h=4097, w=4096) == EUNSUPPORTED
        assert bwd(det, V=17) == EINVAL and bwd(det, V=0) == EINVAL and bwd(det, B=0) == EINVAL
        assert bwd(det, stride=N - 1) == EINVAL                                          # channel 0 of two cubes would overlap
        assert bwd(det, cube=(2048, 2048, 2048), stride=1 << 40) == ERANGE               # beyond 32-bit voxel indexing
        for kw in (dict(cam=None), dict(grad=None), dict(mask=None), dict(acc=None)):
            assert bwd(det, **kw) == ENULL, kw
    assert bwd(True, scale=None) == ENULL
    # the packed training forward keeps refusing the flag
    t = lib.sp3d_unproject_fwd_train
    assert t(views, NHWC | one, 16, d, None, d, d, d, None, d, 1, 2, 1, 8, 8, 4, 4, 4, gs, 96, 72, None) == EUNSUPPORTED


# ---- the launch plan ------------------------------------------------------------------------------------------------------
def _plan(entry, layout, jp=5, B=2, V=3, J=1, h=18, w=24, cube=(24, 16, 20), flags=0):
    return _lib.unproject_fwd_plan(entry, layout | flags, jp, B, V, J, h, w, cube, 0, None)


@pytest.mark.parametrize("V", [1, 5, 7, 9, 12, 16])
@pytest.mark.parametrize("layout", [PLANAR, NHWC])
def test_plan_of_the_training_forward(lib, V, layout):
    """the kernel with MASK = true on the grid (and every Geom field) of the inference forward's launch for the same request:
    the `one_*` rows of tests/golden/fwd_launch_census.json, which tests/test_fwd_launch_plan.py holds the "indexed" plan to"""
    vt = V if V <= 6 else (8 if V <= 8 else (10 if V <= 10 else (12 if V <= 12 else 16)))
    for cl in (False, True):
        kw = dict(V=V, J=4 if cl else 1, flags=_lib.OUT_CHANNELS_LAST if cl else 0)
        rc, train, _ = _plan("one_train", layout, **kw)
        rc0, infer, _ = _plan("indexed", layout, **{**kw, "flags": kw["flags"] | _lib.HM_ONE_CHANNEL})
        assert rc == 0 and rc0 == 0 and len(train) == len(infer) == 1
        t, i = train[0], infer[0]
        assert i["name"] == "unproject_one_kernel<%d, %d, %s>" % (vt, 8 if vt > 8 else 4, "true" if cl else "false")
        assert t["name"] == i["name"][:-1] + ", true>"
        assert {k: v for k, v in t.items() if k != "name"} == {k: v for k, v in i.items() if k != "name"}
        assert (t["workgroups"], t["block"], t["lds"]) == (i["workgroups"], 64, 0) and t["workgroups"] >= 2 * (24 * 16 * 20 // 64)
        # the flag is implied, and accepted
        assert _plan("one_train", layout, **{**kw, "flags": kw["flags"] | _lib.HM_ONE_CHANNEL})[1] == train


def test_plan_refusals_and_old_answers(lib):
    one = _lib.HM_ONE_CHANNEL
    for layout in (PLANAR, NHWC):
        assert _plan("train", layout, flags=one)[0] == EUNSUPPORTED                      # the old entry keeps refusing
        assert _plan("train", layout, J=4, flags=one)[0] == EUNSUPPORTED
        for J in (2, 3, 5, 16):
            assert _plan("one_train", layout, J=J)[0] == EUNSUPPORTED
        assert _plan("one_train", layout, J=1, flags=_lib.OUT_CHANNELS_LAST)[0] == EUNSUPPORTED
        for bf in (_lib.HM_BF16, _lib.OUT_BF16):
            assert _plan("one_train", layout, flags=bf)[0] == EUNSUPPORTED
        for h, w in ((18, 1), (1, 24), (4097, 4096)):
            assert _plan("one_train", layout, h=h, w=w)[0] == EUNSUPPORTED
        assert _plan("one_train", layout, jp=0)[0] == EINVAL
        assert _plan("one_train", layout, V=17)[0] == EINVAL
        # an inference plan never names the mask kernel
        assert _plan("indexed", layout, flags=one)[1][0]["name"].count(",") == 2
    assert _plan("one_train", 7)[0] == EINVAL
    # the packed training entry still plans its own kernels
    rc, launches, _ = _lib.unproject_fwd_plan("train", NHWC, 16, 2, 3, 15, 18, 24, (24, 16, 20), 0, None)
    assert rc == 0 and launches[0]["name"].startswith("unproject_pipe_kernel<16,")


# ---- the switch -----------------------------------------------------------------------------------------------------------
def test_switch_default_and_environment(monkeypatch):
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer
    cfg = load_config(None)
    monkeypatch.delenv("SP3D_ONE_CHANNEL_GRAD", raising=False)
    monkeypatch.delenv("SP3D_ONE_CHANNEL", raising=False)
    assert ProjectLayer(cfg).one_channel_grad is False           # opt-in: no timing rule met
    monkeypatch.setenv("SP3D_ONE_CHANNEL_GRAD", "0")
    assert ProjectLayer(cfg).one_channel_grad is False
    monkeypatch.setenv("SP3D_ONE_CHANNEL_GRAD", "1")
    layer = ProjectLayer(cfg)
    assert layer.one_channel_grad is True and layer.one_channel is False         # independent of the inference switch
    monkeypatch.delenv("SP3D_ONE_CHANNEL_GRAD")
    monkeypatch.setenv("SP3D_ONE_CHANNEL", "1")
    layer = ProjectLayer(cfg)
    assert layer.one_channel is True and layer.one_channel_grad is False


def test_wrappers_keep_their_signatures():
    import inspect
    names = list(inspect.signature(_lib.unproject_one_bwd).parameters)
    assert names == ["cam", "centers", "valid", "grad_cubes", "pass_mask", "batch", "num_views", "h", "w", "cube_size", "grid_size",
                     "img_size", "sample_of", "deterministic"]
    assert inspect.signature(_lib.unproject_one_bwd).parameters["deterministic"].default is False
