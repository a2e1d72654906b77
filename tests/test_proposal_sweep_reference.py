"""The reference side of the randomised sweep of the proposal stage (tests/proposal_sweep_cases.py), pinned on the CPU so
that tests/test_gpu_proposal_sweep.py compares the device against something that was itself checked:
  * NMS: the reference's literal torch expression, an independent numpy selection by the documented total order and
    oracle.nms_topk agree on every case (values bit for bit, indices equal); torch.topk agrees wherever its own order is
    defined; the oracle applies "a NaN voxel is never a candidate" wherever the NaN lies;
  * the case list is the fixed one and reaches what it is there for: -0.0 and negative winners, ties at zero and at other
    values that span tiles, winners on all six faces of a tile, NaN in the volume, unfilled slots, a threshold equal to a
    returned score, the merge kernel's pass boundaries;
  * soft-argmax: the float64 reference gives the fp32 voxel centre in the one-hot rows, the midpoint of two equal peaks and the
    grid mean of a constant row; the error scales S and T are finite and positive; oracle.soft_argmax lies within 2 S; the
    analytic backward is the autograd of the torch graph;
  * the error codes of the proposal entry points that return before any launch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import proposal_sweep_cases as sweep

NMS = list(range(len(sweep.nms_cases())))
SA = list(range(len(sweep.sa_cases())))

# oracle.soft_argmax rounds the fp32 product beta x (relative u), the fp32 subtraction of the maximum (u) and its fp32 result
# (u |out| <= u sum p |g|) and does everything else in double: at first order that is below S; 2 covers the second order.
C_ORACLE = 2.0
# The device constants must stay below what an fp32 accumulation could cost at worst: numerator and denominator of the
# quotient each pass accumulation_depth(N) additions, so 2 depth u sum p |g|.  At the pose net's own 64^3 that is 2 * 278.
C_DEVICE_CEILING = 2 * sweep.accumulation_depth(64 ** 3)


def test_case_lists_are_the_fixed_ones():
    cs = sweep.nms_cases()
    assert len(cs) == len(sweep.NMS_FIXED) + sweep.NMS_NUM_RANDOM == 56 and list(cs[:40]) == sweep.NMS_FIXED
    assert cs == sweep.nms_cases.__wrapped__()                                  # generated from a fixed seed
    fams = [sweep.split_family(c[3]) for c in cs]
    assert {f for f, _ in fams} == set(sweep.NMS_FAMILIES)
    assert {(f, v) for f, v in fams if v} == {(f, v) for f, vs in sweep.NMS_VARIANTS.items() for v in vs}       # every variant
    assert all((v is not None) == (f in sweep.NMS_VARIANTS) for f, v in fams)
    assert {c[2] for c in cs} == set(sweep.KS) | {5} and {c[0] for c in cs} == {1, 3, 260}
    shapes = {c[1] for c in cs}
    assert {(1, 1, 1), (4, 8, 32), (3, 7, 31), (5, 9, 33), (13, 9, 70), (80, 80, 20), (160, 160, 40)} <= shapes
    for axis in range(3):
        assert any(s[axis] == 1 and max(s) > 1 for s in shapes)
    # candidates of the merge kernel: at one pass of <8>, one chunk above, at one pass of <16>, one chunk above
    ncand = {(sweep.num_tiles(c[1]), c[2]) for c in cs}
    assert {(64, 32), (65, 32), (128, 32), (129, 32), (204, 10), (205, 10), (409, 10), (410, 10)} <= ncand
    assert 64 * 32 == 2048 and 128 * 32 == 4096 and 204 * 10 <= 2048 < 205 * 10 and 409 * 10 <= 4096 < 410 * 10
    x0, x1 = sweep.NmsCase(5).x, sweep.NmsCase(5).x
    assert np.array_equal(sweep.bits(x0), sweep.bits(x1))
    sa = sweep.sa_cases()
    assert len(sa) == 30 and {c[4] for c in sa} == set(sweep.SA_FAMILIES) and {c[3] for c in sa} == {1.0, 100.0, 1000.0}
    assert {(64, 64, 64), (16, 12, 10), (7, 1, 33), (1, 5, 4), (5, 3, 1), (1, 1, 1), (5, 3, 2), (1, 1, 1025), (3, 11, 31),
            (96, 96, 96)} <= {c[2] for c in sa}
    assert np.array_equal(sweep.SaCase(5).x, sweep.SaCase(5).x)
    assert 96 ** 3 > 256 * 256 * 8                                              # beyond the backward's cap of 256 workgroups


# ---------------------------------------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------------------------------------
def _best_are_distinct(nv, kk):
    """(B,) bool: the best kk + 1 values of a sample are pairwise distinct, so torch.topk's indices are defined"""
    best = np.sort(nv, 1)[:, ::-1][:, :kk + 1]
    return (np.diff(best, axis=1) != 0).all(1)


@pytest.mark.parametrize("idx", NMS, ids=sweep.nms_case_id)
def test_nms_reference_layers_agree(idx):
    c = sweep.nms_get(idx)
    vals, flat = c.selected
    ov, oi = c.oracle
    assert vals.shape == ov.shape == (c.B, c.k) and oi.shape == c.idx3.shape == (c.B, c.k, 3)
    assert np.array_equal(sweep.bits(vals), sweep.bits(ov)), "values: numpy selection vs oracle"
    assert np.array_equal(c.idx3, oi), "indices: numpy selection vs oracle"
    assert not np.isnan(vals).any()
    nv = c.nms_volume.reshape(c.B, c.N)
    # a filled slot returns the volume's own bits at its index; an empty one is +0.0 at (0, 0, 0)
    filled = flat >= 0
    for b in range(c.B):
        assert np.array_equal(sweep.bits(vals[b][filled[b]]), sweep.bits(nv[b][flat[b][filled[b]]]))
    assert not sweep.bits(vals[~filled]).any() and not c.idx3[~filled].any()
    assert np.array_equal(filled.sum(1), np.minimum(c.k, (~np.isnan(nv)).sum(1)))
    if c.has_nan or np.isnan(nv).any():
        return
    # torch.topk on the same volume: the same multiset of values; the same indices where the best k + 1 are distinct
    kk = min(c.k, c.N)
    tv, ti = torch.topk(torch.from_numpy(nv), kk, dim=1)
    assert np.array_equal(np.sort(tv.numpy(), 1), np.sort(vals[:, :kk], 1))
    distinct = _best_are_distinct(nv, kk)
    assert np.array_equal(ti.numpy()[distinct], flat[:, :kk][distinct])


@pytest.mark.parametrize("idx", NMS, ids=sweep.nms_case_id)
def test_nms_locs_rows_and_thresholds(idx):
    c = sweep.nms_get(idx)
    thr = c.thresholds
    assert len(thr) == 5 and np.float32(thr[0]) == c.vals[0, c.k // 2] and thr[2] == 0.0 and thr[3] < 0 and thr[4] == np.inf
    if np.isfinite(thr[0]):
        assert thr[1] < thr[0] and np.float32(thr[1]) == np.float32(thr[1]).astype(np.float64) == thr[1]
    one_bin = np.array(c.shape) == 1
    assert np.isnan(c.locs[..., one_bin]).all() and np.isfinite(c.locs[..., ~one_bin]).all()
    lo = np.array(c.grid_center) - np.array(c.grid_size) / 2
    inside = (c.locs >= lo - 1.0) & (c.locs <= lo + np.array(c.grid_size) + 1.0)
    assert inside[..., ~one_bin].all()
    for t in thr:
        r = c.rows(t)
        assert r.shape == (c.B, c.k, 5) and r.dtype == np.float32
        assert np.array_equal(r[..., 3], np.where(c.vals > t, 0.0, -1.0)) and sweep.rows_equal(r, r.copy())
    # strict >: the slot whose score is the threshold is rejected, and accepted one fp32 step below
    assert c.rows(thr[0])[0, c.k // 2, 3] == -1.0
    if np.isfinite(thr[0]):
        assert c.rows(thr[1])[0, c.k // 2, 3] == 0.0
    assert not (c.rows(thr[4])[..., 3] == 0.0).any()


def test_oracle_never_returns_a_nan_voxel():
    """the three inputs on which the oracle used to contradict its own rule"""
    from oracle import oracle
    x = np.random.default_rng(0).random((1, 8, 8, 8), dtype=np.float32)
    ref_v, ref_i = oracle.nms_topk(x, 10)
    a = x.copy(); a[0, 0, 0, 0] = np.nan
    va, ia = oracle.nms_topk(a, 10)
    assert not np.isnan(va).any() and not (ia == 0).all(-1).any()               # NaN at flat index 0 does not win
    b = x.copy(); b[0, 4, 4, 4] = np.nan
    vb, ib = oracle.nms_topk(b, 10)
    assert not np.isnan(vb).any() and not (ib == 4).all(-1).any()
    for v, i in ((va, ia), (vb, ib)):                                            # peaks away from the NaN are the old ones
        far = (np.abs(i - (0 if v is va else 4)).max(-1) > 1)[0]
        assert far.any() and all(any((i[0, s] == ref_i[0, t]).all() and v[0, s] == ref_v[0, t] for t in range(10))
                                 for s in np.flatnonzero(far) if v[0, s] > 0.9)
    c = np.full((1, 8, 8, 8), -np.inf, np.float32); c[0, 3, 5, 2] = -3.0
    vc, ic = oracle.nms_topk(c, 5)
    assert vc[0, 0] == -3.0 and ic[0, 0].tolist() == [3, 5, 2] and (vc[0, 1:] == -np.inf).all()
    near = np.abs(ic[0, 1:] - np.array([3, 5, 2])).max(-1) <= 1
    assert not near.any()                                                        # the 0 * -inf = NaN neighbours are no candidates
    flat = (ic[0, 1:, 0] * 8 + ic[0, 1:, 1]) * 8 + ic[0, 1:, 2]
    assert flat.tolist() == [0, 1, 2, 3]


def test_nms_sweep_is_not_vacuous():
    minus_zero = negative = zero_tiles = equal_tiles = nan_absent = unfilled = thr_hit = nan_free = topk_cases = topk_samples = 0
    faces = np.zeros(6, int)
    T = np.array(sweep.TILE)
    for idx in NMS:
        c = sweep.nms_get(idx)
        vals, flat = c.selected
        filled = flat >= 0
        b = sweep.bits(vals)
        minus_zero += bool(((b == 0x80000000) & filled).any())
        negative += bool((vals < 0).any())
        tiles = sweep.tile_of(c.idx3)
        for s in range(min(c.B, 3)):
            z = filled[s] & (vals[s] == 0)
            zero_tiles += len(set(tiles[s][z])) >= 2
            nz = filled[s] & (vals[s] != 0)
            equal_tiles += any(len(set(tiles[s][nz & (vals[s] == v)])) >= 2 for v in set(vals[s][nz]))
        w = c.idx3[filled & (vals > 0)] if c.family == "faces" else np.zeros((0, 3), int)
        for a in range(3):
            faces[2 * a] += bool((w[:, a] % T[a] == 0).any())
            faces[2 * a + 1] += bool((w[:, a] % T[a] == T[a] - 1).any() and c.shape[a] > T[a])
        nan_absent += bool(np.isnan(c.x).any())
        nv = c.nms_volume.reshape(c.B, c.N)
        if not np.isnan(nv).any():
            nan_free += 1
            d = _best_are_distinct(nv, min(c.k, c.N))
            topk_cases += bool(d.any())
            topk_samples += int(d.sum())
        unfilled += bool((~filled).any())
        thr_hit += bool((c.vals == np.float32(c.thresholds[0])).any())
    print("minus_zero", minus_zero, "negative", negative, "zero_tiles", zero_tiles, "equal_tiles", equal_tiles, "faces", faces,
          "nan", nan_absent, "unfilled", unfilled, "thr", thr_hit, "nan_free", nan_free, "topk index cases", topk_cases,
          "samples", topk_samples)
    assert minus_zero >= 12, minus_zero
    assert negative >= 8, negative
    assert zero_tiles >= 8, zero_tiles
    assert equal_tiles >= 8, equal_tiles
    assert (faces >= 2).all(), faces
    assert nan_absent >= 6, nan_absent
    assert unfilled >= 4, unfilled
    assert thr_hit == len(NMS)
    # the comparison of indices with torch.topk is not vacuous: samples whose best k + 1 values are distinct
    assert nan_free >= 40 and topk_cases >= 10 and topk_samples >= 100, (nan_free, topk_cases, topk_samples)


def test_few_peaks_mix_both_zeros_among_the_winners():
    """the zero merge of the kernel's key: +0.0 candidates lie at higher flat indices than -0.0 ones and still come later"""
    seen = 0
    for idx in NMS:
        c = sweep.nms_get(idx)
        if c.family != "few_peaks":
            continue
        vals, flat = c.selected
        for s in range(min(c.B, 3)):
            b = sweep.bits(vals[s])
            z = (vals[s] == 0) & (flat[s] >= 0)
            if (b[z] == 0).any() and (b[z] == 0x80000000).any():
                assert np.all(np.diff(flat[s][z]) > 0)                           # by flat index alone, whatever the sign
                first_plus = np.flatnonzero(z & (b == 0))[0]
                seen += bool((z & (b == 0x80000000))[:first_plus].any())
    assert seen >= 4, seen


# ---------------------------------------------------------------------------------------------------------------------------
# soft-argmax
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", SA, ids=sweep.sa_case_id)
def test_soft_argmax_reference(idx):
    from oracle import oracle
    c = sweep.sa_get(idx)
    out, S = c.out, c.S
    assert out.shape == S.shape == (c.P, c.J, 3) and out.dtype == np.float64
    g = c.grids
    assert g.dtype == np.float32 and g.shape == (c.P, c.N, 3)
    assert np.isfinite(out).all() and np.isfinite(S).all() and (S >= 0).all()
    if c.family == "one_hot":
        want = g[np.arange(c.P)[:, None], c.hot]                                # (P, J, 3) fp32 voxel centres
        assert np.array_equal(out, want.astype(np.float64))
        assert ((S > 0) | (want == 0)).all()                                    # S = 0 only where the one centre is exactly 0
    else:
        assert (S > 0).all()
    if c.family == "two_peaks":
        mid = (g[:, 0].astype(np.float64) + g[:, -1].astype(np.float64)) / 2
        assert np.array_equal(out, np.broadcast_to(mid[:, None], out.shape))
    if c.family == "constant":
        mean = g.astype(np.float64).mean(1)
        assert np.abs(out - mean[:, None]).max() <= 1e-12 * np.abs(g).max()
    # the weights sum to one and the result lies inside the grid
    assert np.abs(c.p.sum(axis=(2, 3, 4)) - 1).max() <= 1e-12
    lo, hi = g.min(1).astype(np.float64)[:, None], g.max(1).astype(np.float64)[:, None]
    assert (out >= lo - 1e-9).all() and (out <= hi + 1e-9).all()
    ref = oracle.soft_argmax(c.x, g, c.beta).astype(np.float64)
    assert (np.abs(ref - out) <= C_ORACLE * S).all(), float((np.abs(ref - out) / np.maximum(S, 1e-300)).max())
    # backward: analytic form == autograd of the torch graph; T finite and positive
    dx = c.dx
    assert dx.shape == c.x.shape and dx.dtype == np.float64
    assert np.abs(dx - c.dx_analytic).max() <= 1e-11 * max(1e-300, np.abs(dx).max())
    T = c.T(64.0)
    assert T.shape == dx.shape and np.isfinite(T).all() and (T > 0).all()
    assert (c.T(128.0) >= T).all()
    se, scale = c.sumexp
    assert (scale > 0).all() and (se >= 1.0 - scale).all() and (se <= c.N * (1.0 + 1e-5)).all()


def test_soft_argmax_sweep_is_not_vacuous():
    kinds = set()
    odd_middle_at_origin = underflow = 0
    for idx in SA:
        c = sweep.sa_get(idx)
        if c.family == "one_hot":
            kinds |= set(c.hot_kind)
            for r, kd in enumerate(c.hot_kind):
                # the row that tells the two forms of linspace apart: middle bin of an odd axis, cube 0 (centre at the origin),
                # and the two forms do differ there in fp32
                if kd == "middle" and r == 0:
                    for d in range(3):
                        n, L = c.cube[d], np.float32(c.grid_size[d])
                        if n % 2 == 1 and n > 1:
                            step = (L / np.float32(2) - (-(L / np.float32(2)))) / np.float32(n - 1)
                            a = np.float32(np.float64(step) * (n // 2) - np.float64(L / np.float32(2)))
                            b = np.float32(np.float64(-step) * (n - 1 - n // 2) + np.float64(L / np.float32(2)))
                            odd_middle_at_origin += bool(a != b) and c.axes[d][0, n // 2] == b
        underflow += bool((c.p == 0).any())
    assert kinds == set(sweep.HOT_KINDS), kinds
    assert odd_middle_at_origin >= 2, odd_middle_at_origin
    assert underflow >= 8, underflow
    assert C_ORACLE < C_DEVICE_CEILING == 556


# ---------------------------------------------------------------------------------------------------------------------------
# error codes that need no device (every one returns before a launch; tests/test_host_cabi.py has k = 33 and a null cube)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from selfpose3d_amd import _lib, build as sbuild
    sbuild.build()
    return _lib.load()


def test_proposal_entry_points_refuse_bad_arguments(lib):
    buf = C.create_string_buffer(4096)
    d = C.cast(buf, C.c_void_p).value
    f3 = (C.c_float * 3)(1000.0, 1000.0, 1000.0)
    EINVAL, ENULL, ERANGE = -1, -2, -3
    assert lib.sp3d_error_string(EINVAL) and lib.sp3d_error_string(ERANGE)
    top = lambda cube, B, k, vals=d, idx=d, ws=d, gs=None, gc=None, locs=None: lib.sp3d_nms_topk(
        cube, B, 4, 4, 4, k, gs, gc, vals, idx, locs, ws, None)
    assert top(d, 1, 0) == EINVAL and top(d, 1, -3) == EINVAL and top(d, 1, 33) == EINVAL and top(d, 0, 10) == EINVAL
    assert top(d, 1, 10, vals=None) == ENULL and top(d, 1, 10, idx=None) == ENULL and top(d, 1, 10, ws=None) == ENULL
    assert top(d, 1, 10, locs=d) == ENULL and top(d, 1, 10, locs=d, gs=f3) == ENULL        # locs without size / centre
    assert top(d, 65536, 10) == ERANGE
    prop = lambda B, k, locs, out: lib.sp3d_nms_proposals(d, B, 4, 4, 4, k, f3, f3, C.c_float(0.3), d, d, locs, out, d, None)
    assert prop(1, 0, d, d) == EINVAL and prop(1, 33, d, d) == EINVAL
    assert prop(1, 10, None, d) == ENULL                                        # rows need locs
    assert prop(65536, 10, d, d) == ERANGE
    assert lib.sp3d_nms_topk_workspace_bytes(1, 4, 4, 4, 0) == 0 and lib.sp3d_nms_topk_workspace_bytes(0, 4, 4, 4, 10) == 0
    assert lib.sp3d_nms_topk_workspace_bytes(3, 5, 9, 33, 32) == 3 * 8 * 32 * 8
    b100 = C.c_float(100.0)
    assert lib.sp3d_soft_argmax(d, d, d, 1, 0, 64, b100, None) == EINVAL and lib.sp3d_soft_argmax(d, d, d, 1, 1, 0, b100, None) == EINVAL
    assert lib.sp3d_soft_argmax(None, d, d, 1, 1, 64, b100, None) == ENULL and lib.sp3d_soft_argmax(d, None, d, 1, 1, 64, b100, None) == ENULL
    assert lib.sp3d_soft_argmax(d, d, None, 1, 1, 64, b100, None) == ENULL
    grid = lambda x, cen, gs, out, Bv=1, J=1, X=4: lib.sp3d_soft_argmax_grid(x, cen, gs, X, 4, 4, out, Bv, J, b100, None)
    assert grid(d, d, f3, d, Bv=0) == EINVAL and grid(d, d, f3, d, J=0) == EINVAL and grid(d, d, f3, d, X=0) == EINVAL
    assert grid(d, d, f3, d, Bv=65536) == EINVAL
    assert grid(None, d, f3, d) == ENULL and grid(d, None, f3, d) == ENULL and grid(d, d, None, d) == ENULL and grid(d, d, f3, None) == ENULL
    assert lib.sp3d_soft_argmax_grid(d, d, f3, 2048, 2048, 1024, d, 1, 1, b100, None) == ERANGE
    bwd = lambda x=d, out=d, stats=d, g=d, dx=d, J=1: lib.sp3d_soft_argmax_grid_bwd(x, d, f3, 4, 4, 4, out, stats, g, dx, 1, J, b100, None)
    assert bwd(J=0) == EINVAL and bwd(J=65536) == EINVAL
    assert bwd(x=None) == ENULL and bwd(out=None) == ENULL and bwd(stats=None) == ENULL and bwd(g=None) == ENULL and bwd(dx=None) == ENULL
