"""The CPU side of the sweep of joint rendering and the memory-bound helper kernels (tests/glue_sweep_cases.py), so that
tests/test_gpu_glue_sweep.py compares the device with something that was itself checked:
  * every class the tables are there for is entered by at least one case (the classes are read off shapes and inputs);
  * each referee agrees with an independent restatement by plain loops on the small cases;
  * the error scales of the rendering and of the up-conv head are finite, and positive wherever a result can be non-zero;
  * in every rendering case at most 0.1 % of the pixels are undecided about the clip;
  * the documented refusals of the entries come back from the library before any launch;
  * the ledger: every sp3d_* function of include/sp3d.h names the test modules that sweep it.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import glue_sweep_cases as gs
from tests.test_host_cabi import _header_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# A. joint rendering
# ---------------------------------------------------------------------------------------------------------------------------
def test_render_table_enters_every_class():
    seen = set()
    for i, case in enumerate(gs.RENDER_CASES):
        seen |= gs.render_classes(case, gs.render_problem(i)[1])
    want = set(gs.RENDER_PIXEL_CLASSES) | set(gs.RENDER_COUNT_CLASSES) | set(gs.RENDER_PLACEMENTS)
    want |= {"P=1", "P=2", "P=15", "P=16", "J=1", "J=15", "J=17", "N=1", "N=6", "sigma=0.5", "sigma=3", "sigma=20",
             "count differs per n"}
    assert want <= seen, sorted(want - seen)
    # the geometry behind the pixel classes, on the numbers the issue names
    assert gs.render_geometry(5, 7)["fwd_blocks"] == 1 and gs.render_geometry(16, 16)["bwd_serial"] == 1
    assert gs.render_geometry(257, 1)["fwd_blocks"] == 2 and gs.render_geometry(1, 257)["bwd_serial"] == 2
    g = gs.render_geometry(65, 127)
    assert g["hw"] > 32 * 256 and g["fwd_blocks"] == 32 and g["fwd_trips"] == 2 and g["bwd_depth"] == 33 + 8
    # no infinite key-point in a backward case; rows p >= count hold NaN in every case
    for i, case in enumerate(gs.RENDER_CASES):
        kps = gs.render_problem(i)[1]
        for n, c in enumerate(gs.render_effective_count(case)):
            assert torch.isnan(kps[n, c:]).all() and not torch.isnan(kps[n, :c]).any()
            assert case.get("backward", True) <= bool(torch.isfinite(kps[n, :c]).all())


def test_render_placements_do_what_they_are_named_for():
    by_name = {c["name"]: i for i, c in enumerate(gs.RENDER_CASES)}
    # on a pixel centre: the sum is exactly 1 in float64, and in fp32 (one exp(0), every other term zero or absent)
    case, kps, count, gout, ref = gs.render_problem(by_name["5x7 one person on a centre"])
    assert float(ref["s"][0, 0, 5 // 3, 7 // 2]) == 1.0 and float(ref["out"].max()) == 1.0
    case, kps, count, gout, ref = gs.render_problem(by_name["19x30 infinite co-ordinates"])
    assert float(ref["s"][0, 7, 19 // 3, 30 // 2]) == 1.0                 # the infinite neighbour contributes exp(-inf) = 0
    assert float(ref["s"][0, 0].max()) < 1.0 and torch.isfinite(ref["s"]).all() and torch.isfinite(ref["T_fwd"]).all()
    # coincident: the clip is active over a disc; one sigma apart: a mask boundary (both sides present)
    case, kps, count, gout, ref = gs.render_problem(by_name["16x16 coincident pair"])
    assert 10 < int((ref["s"][0, 0] > 1).sum()) < 128 and float(ref["s"].max()) > 1.9
    case, kps, count, gout, ref = gs.render_problem(by_name["65x127 grid-stride, pairs"])
    assert 0 < int((ref["s"][3, 7] > 1).sum()) < 65 * 127
    # 1e4 pixels outside: the contribution is 0 in both formats, map and gradient
    j = 2
    assert float(ref["s"][5, j].max()) < 1.0 and float(ref["grad"][5, 0, j].abs().max()) == 0.0
    assert float(np.exp(np.float32(-(1e4 / 3.0) ** 2 / 2))) == 0.0
    # count = 0: zero map, zero gradient; gradient rows p >= count are exactly zero
    assert float(ref["out"][1].abs().max()) == 0.0 and float(ref["grad"][1].abs().max()) == 0.0
    assert float(ref["grad"][2, 1:].abs().max()) == 0.0 and float(ref["grad"][2, 0].abs().max()) > 0.0


@pytest.mark.parametrize("index", range(len(gs.RENDER_CASES)))
def test_render_scales_and_undecided_pixels(index):
    case, kps, count, gout, ref = gs.render_problem(index)
    T = ref["T_fwd"]
    assert torch.isfinite(T).all() and (T >= 0).all()
    for n, c in enumerate(ref["np"]):
        assert (T[n] > 0).all() if c else (T[n] == 0).all()
    und = gs.render_undecided(ref)
    print(case["name"], "undecided", int(und.sum()), "of", und.numel())
    assert int(und.sum()) <= gs.UNDECIDED_CAP * und.numel()
    if case.get("backward", True):
        Tb, A = gs.render_bwd_scales(case, kps, gout, ref)
        assert torch.isfinite(Tb).all() and torch.isfinite(A).all() and (A >= 0).all()
        for n, c in enumerate(ref["np"]):
            assert (Tb[n, :c] > 0).all() and (Tb[n, c:] == 0).all() and (A[n, c:] == 0).all()
        assert (ref["grad"].abs() <= 1e3 * Tb / gs.U24 + 1e-300).all()              # the scale is the gradient's own size


@pytest.mark.parametrize("index", [i for i, c in enumerate(gs.RENDER_CASES) if c["N"] * c["P"] * c["J"] * c["h"] * c["w"] <= 20000])
def test_render_referee_against_loops(index):
    case, kps, count, gout, ref = gs.render_problem(index)
    k = torch.nan_to_num(kps, nan=0.0) if case["count"] is not None else kps    # the loops never read rows p >= count either
    out, grad = gs.render_naive(k, count, case["h"], case["w"], case["sigma"], gout if case.get("backward", True) else None)
    assert np.abs(out - ref["out"].numpy()).max() <= 1e-14
    if case.get("backward", True):
        assert np.abs(grad - ref["grad"].numpy()).max() <= 1e-12 * max(1.0, float(ref["grad"].abs().max()))


def test_render_cases_small_enough_for_loops_exist():
    small = [c for c in gs.RENDER_CASES if c["N"] * c["P"] * c["J"] * c["h"] * c["w"] <= 20000]
    assert len(small) >= 4 and any(c["count"] is not None for c in small) and any(not c.get("backward", True) for c in small)


# ---------------------------------------------------------------------------------------------------------------------------
# B. heat-map packing
# ---------------------------------------------------------------------------------------------------------------------------
def test_pack_table_enters_every_class():
    assert len(gs.PACK_ROWS) == 11 and len(set(gs.PACK_ROWS)) == 11
    assert {gs.pack_geometry(h, w)["hw"] for h, w in gs.PACK_IMAGES} == {1, 255, 256, 257, 768, 33 * 65}
    for row in gs.PACK_ROWS:
        cases = gs.pack_cases(row)
        Jp = row[0]
        assert {c["J"] for c in cases} >= {1, Jp - 1, Jp} | ({17} if Jp == 32 else set()), row
        assert {(c["h"], c["w"]) for c in cases} >= set(gs.PACK_IMAGES)
        assert {c["B"] for c in cases} == {1, 3} and {c["V"] for c in cases} == {1, 16}
        assert sum(c["offset"] for c in cases) == 1
        if row[1] or row[2]:                                        # every special value reaches the kernel in this row
            seen = set()
            for c in cases:
                for x in gs.pack_inputs(c):
                    seen |= set(np.unique(x.float().numpy().view(np.uint32)).tolist())
            want = set(gs.PACK_SPECIALS)
            if row[1]:                                              # bf16 inputs hold the specials as torch converts them
                want = set((gs.bits_of(torch.tensor(gs.PACK_SPECIALS, dtype=torch.int64).to(torch.int32).view(torch.float32)
                                       .to(torch.bfloat16)).to(torch.int64) & 0xFFFF).mul(65536).tolist())
            assert want <= seen, (row, sorted(want - seen))


def test_pack_referee_is_torchs_conversion_on_the_specials():
    x = torch.tensor(gs.PACK_SPECIALS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    b = (gs.bits_of(x.to(torch.bfloat16)).to(torch.int64) & 0xFFFF).tolist()
    assert b[:9] == [0x0000, 0x8000, 0x0000, 0x8040, 0x7F80, 0xFF80, 0x3F80, 0x3F82, 0x7F80]      # ties to even, 0x7f7fffff -> inf
    assert all((v & 0x7FFF) > 0x7F80 for v in b[9:])                 # a NaN stays a NaN
    # what integer rounding alone does to them: the three defects the sweep is there to catch
    u = np.asarray(gs.PACK_NANS, np.uint64)
    wrong = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).tolist()
    assert wrong == [0x7FC0, 0x7F80, 0x7F81, 0x8000, 0x0000]


@pytest.mark.parametrize("row", gs.PACK_ROWS, ids=gs.pack_row_name)
def test_pack_referee_against_loops(row):
    for case in gs.pack_cases(row):
        if case["B"] * case["V"] * case["J"] * case["h"] * case["w"] > 6000:
            continue
        views = gs.pack_inputs(case)
        ref = gs.pack_referee(views, case["Jp"], case["out_bf16"])
        naive = gs.pack_naive(views, case["Jp"], case["out_bf16"])
        got = torch.from_numpy(naive.view(np.int16 if case["out_bf16"] else np.int32)).view(ref.dtype)
        assert gs.same_bits_nan_free(got, ref), case
        assert ref[..., case["J"]:].abs().sum() == 0 and not torch.signbit(ref[..., case["J"]:]).any()


# ---------------------------------------------------------------------------------------------------------------------------
# C. channel shift + activation
# ---------------------------------------------------------------------------------------------------------------------------
def test_csa_table_enters_every_class():
    seen = set()
    for s in gs.CSA_SHAPES:
        assert gs.csa_refusal(s[1], s[2], s[3]) == 0
        seen |= gs.csa_classes(s)
    want = {"planar", "channels-last", "planar inner=4", "planar C=1", "channels-last C=4", "channels-last C=12",
            "channels-last C=64", "n4<256", "ragged last workgroup"}
    assert want <= seen, sorted(want - seen)
    assert "second trip" not in seen and "second trip, partial" not in seen
    b, c, inner = gs.CSA_LARGE
    g = gs.csa_geometry(b, c, inner)
    assert g["n"] == 8519680 > gs.CSA_CAP * 256 * 4 == 8388608 and g["blocks"] == gs.CSA_CAP and g["trips"] == 2
    assert 0 < g["last_trip"] < g["blocks"] * 256
    for cl in (0, 1):
        assert gs.csa_refusal(c, inner, cl) == 0 and "second trip, partial" in gs.csa_classes((b, c, inner, cl))
    assert sorted(gs.CSA_LARGE_MODES) == [0, 1]


@pytest.mark.parametrize("mode", range(4))
def test_csa_referee_against_loops(mode):
    for i, shape in enumerate(gs.CSA_SHAPES):
        if shape[0] * shape[1] * shape[2] > 2100:
            continue
        for nan in (False, True):
            y, shift, res = gs.csa_inputs(shape, i, nan)
            ref = gs.csa_referee(y, shift, res, mode, shape[3])
            assert gs.same_bits_nan_free(gs.csa_naive(y, shift, res, mode, shape[3]), ref), (shape, mode, nan)
            # the pinned NaN rule: fmaxf - NaN becomes 0 (+ residual in mode 3) in modes 1-3, stays NaN in mode 0
            was = torch.isnan(y)
            assert bool(torch.isnan(ref)[was].all()) == (mode == 0) or not nan
            if nan and mode in (1, 2):
                assert (ref[was] == 0).all()
            if nan and mode == 3:
                assert torch.equal(ref[was], res[was])


# ---------------------------------------------------------------------------------------------------------------------------
# D. max-pool
# ---------------------------------------------------------------------------------------------------------------------------
def test_pool_table_enters_every_class():
    assert gs.POOL_SHAPES[0] == (1, 2, 2, 2, 4)
    assert {s[4] for s in gs.POOL_SHAPES} == {4, 12, 32, 128} and {s[0] for s in gs.POOL_SHAPES} == {1, 3}
    for axis in (1, 2, 3):
        assert {s[axis] for s in gs.POOL_SHAPES} == {2, 6, 10}
    assert all(gs.pool_refusal(*s) == 0 and not gs.pool_geometry(*s)["capped"] for s in gs.POOL_SHAPES)
    assert gs.pool_geometry(3, 10, 10, 10, 32)["blocks"] == 12          # more than one workgroup, the last one ragged
    # the cap needs more lanes than an input of 34 GB has: not reachable, not tested
    assert gs.POOL_CAP_LANES * 8 * 4 * 4 > 34e9
    assert gs.POOL_FAMILIES == ["random", "ties", "neg_inf"] + ["nan_at_%d" % t for t in range(8)] + ["all_nan"]
    shape = (3, 6, 10, 2, 12)
    win = lambda x: x.view(3, 3, 2, 5, 2, 1, 2, 12).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(-1, 8)
    assert (win(gs.pool_inputs(shape, "ties")).sort(1).values.diff(dim=1) == 0).any(1).all()      # a tie in every window
    assert (win(gs.pool_inputs(shape, "neg_inf")) == float("-inf")).all(1).any()
    assert torch.isnan(win(gs.pool_inputs(shape, "all_nan"))).all(1).any()
    for t in range(8):
        w = torch.isnan(win(gs.pool_inputs(shape, "nan_at_%d" % t)))
        assert w[:, t].any() and not w[:, [u for u in range(8) if u != t]].any()


@pytest.mark.parametrize("family", gs.POOL_FAMILIES)
def test_pool_referee_against_loops(family):
    for shape in gs.POOL_SHAPES[:3] + gs.POOL_SHAPES[4:5]:
        x = gs.pool_inputs(shape, family)
        ref = gs.pool_referee(x)
        assert gs.same_bits_nan_free(gs.pool_naive(x), ref), (shape, family)
        assert tuple(ref.shape) == (shape[0], shape[1] // 2, shape[2] // 2, shape[3] // 2, shape[4])


# ---------------------------------------------------------------------------------------------------------------------------
# E. fixed point -> float
# ---------------------------------------------------------------------------------------------------------------------------
def test_fix_table_and_referee():
    assert gs.FIX_NS == [1, 255, 256, 257, 100003] and gs.FIX_SCALES == [2.0 ** -10, 1.0, 2.0 ** 40]
    assert [gs.fix_geometry(n)["blocks"] for n in gs.FIX_NS] == [1, 1, 1, 2, 391]
    first = set()
    for seed, n in enumerate(gs.FIX_NS * 3):
        acc = gs.fix_inputs(n, seed)
        assert acc.dtype == np.int64 and len(acc) == n
        first.add(int(acc[0]))
        if n >= 255:
            assert set(gs.FIX_SPECIALS) <= set(acc.tolist())
    assert len(first) >= 10                                              # n = 1 meets a different value in every case
    # the halfway integers are halfway: both neighbours of the quotient are equally far
    h = gs.fix_halfway(24, 3)[:24]
    for scale in gs.FIX_SCALES:
        q = h.astype(np.float64) / scale
        f = q.astype(np.float32).astype(np.float64)
        other = np.where(f > q, np.nextafter(f.astype(np.float32), np.float32(-np.inf)), np.nextafter(f.astype(np.float32), np.float32(np.inf)))
        assert (np.abs(f - q) == np.abs(other.astype(np.float64) - q)).all() and (f != q).all()
        assert (f.astype(np.float32).view(np.uint32) & 1 == 0).all()     # ties went to even
    for seed, scale in enumerate(gs.FIX_SCALES):
        acc = gs.fix_inputs(257, seed)
        assert np.array_equal(gs.fix_referee(acc, scale).view(np.uint32), gs.fix_naive(acc, scale).view(np.uint32))
    assert gs.fix_referee(np.asarray([gs.INT64_MAX, gs.INT64_MIN]), 1.0).tolist() == [2.0 ** 63, -2.0 ** 63]


# ---------------------------------------------------------------------------------------------------------------------------
# F. fetch ring
# ---------------------------------------------------------------------------------------------------------------------------
def test_ring_table_enters_every_class():
    seen = set()
    for case in gs.RING_CASES:
        seen |= gs.ring_classes(case)
    assert {"vector", "scalar", "R=1", "R=3", "fewer than 256 vectors", "one full trip", "second trip, almost idle", "n=1",
            "n%4!=0", "dst misaligned"} <= seen and "other" not in seen
    assert gs.ring_geometry(4096, 0)["trips"] == 1 and gs.ring_geometry(4100, 0)["trips"] == 2
    assert gs.ring_expected(3, 0, 5) == [(0, 1), (1, 2), (2, 3), (0, 4), (1, 5)]
    assert gs.ring_expected(3, gs.RING_WRAP, 2) == [((2 ** 32 - 1) % 3, 0), (0, 1)]
    assert gs.ring_expected(1, gs.RING_WRAP, 1) == [(0, 0)]
    d = gs.ring_data(1283, 3, 0)
    assert d.shape == (3, 1283) and len({d[r].tobytes() for r in range(3)}) == 3


# ---------------------------------------------------------------------------------------------------------------------------
# G. up-conv scatter
# ---------------------------------------------------------------------------------------------------------------------------
def test_up_table_enters_every_class():
    seen = [gs.up_classes(c) for c in gs.UP_CASES]
    assert "second trip" in seen[4] and "scatter O=64" in seen[4] and "second trip" in seen[5] and "head J=15" in seen[5]
    assert all("one trip" in s for s in seen[:4]) and "ragged" in seen[0]
    assert {"head J=1", "head J=9"} <= set().union(*seen) and "second head group" in seen[3] and "second head group" in seen[5]
    g = gs.up_geometry(*gs.UP_CASES[4])
    assert g["n_in"] == 32769 and g["total"] > gs.UP_CAP * 256 and g["second_trip_lanes"] == 128
    assert g["n_in"] * 8 * 64 * 4 == 67110912                           # the 67 MB result
    g = gs.up_geometry(*gs.UP_CASES[5])
    assert g["n_in"] == 65537 and g["second_trip_lanes"] == 64 and gs.UP_CASES[5][2:] == (32, 15)


@pytest.mark.parametrize("index", range(4))
def test_up_referees_against_loops(index):
    case = gs.UP_CASES[index]
    batch, size, O, J = case
    G, shift, skip, w, b = gs.up_inputs(case, index)
    naive = gs.up_naive(G, shift, skip, w, b, batch, size, O, J)
    if not J:
        ref = gs.up_scatter_referee(G, shift, skip, batch, size, O)
        assert np.array_equal(naive.view(np.int32), ref.numpy().view(np.int32))
    else:
        head, scale = gs.up_head_referee(G, shift, skip, w, b, batch, size, O)
        assert np.abs(naive - head.numpy()).max() <= 1e-13
        assert torch.isfinite(scale).all() and (scale > 0).all() and tuple(scale.shape) == tuple(head.shape)
        assert (head.abs() <= scale / (33 * gs.U24)).all()


def test_constants_are_powers_of_two():
    for c in (gs.C_FWD, gs.C_BWD, gs.C_HEAD):
        assert c > 0 and gs.power_of_two_at_or_above(c) == c
    assert gs.power_of_two_at_or_above(4 * 1.3) == 8.0 and gs.power_of_two_at_or_above(4.0) == 4.0


# ---------------------------------------------------------------------------------------------------------------------------
# refusals that need no device: every one comes back before a launch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from selfpose3d_amd import _lib, build as sbuild
    sbuild.build()
    return _lib.load()


def test_entries_refuse_bad_arguments(lib):
    buf = C.create_string_buffer(4096)
    d = C.cast(buf, C.c_void_p).value
    EINVAL, ENULL, ERANGE, EUNSUPPORTED = gs.EINVAL, gs.ENULL, gs.ERANGE, gs.EUNSUPPORTED
    for code in (EINVAL, ENULL, ERANGE, EUNSUPPORTED):
        assert lib.sp3d_error_string(code)
    # joint rendering
    fwd = lambda kps=d, out=d, N=1, P=1, J=1, h=4, w=4, sigma=3.0: lib.sp3d_render_joints_fwd(kps, None, N, P, J, h, w, sigma, out, None)
    bwd = lambda kps=d, go=d, gk=d, N=1, P=1, J=1, h=4, w=4, sigma=3.0: lib.sp3d_render_joints_bwd(kps, None, go, N, P, J, h, w, sigma, gk, None)
    for f in (fwd, bwd):
        assert f(N=0) == EINVAL and f(P=0) == EINVAL and f(P=17) == EINVAL and f(J=0) == EINVAL and f(h=0) == EINVAL and f(w=0) == EINVAL
        assert f(sigma=0.0) == EINVAL and f(sigma=-1.0) == EINVAL and f(sigma=float("nan")) == EINVAL
        assert f(kps=None) == ENULL and f(N=65536) == ERANGE
    assert fwd(out=None) == ENULL and fwd(J=65536) == ERANGE and bwd(go=None) == ENULL and bwd(gk=None) == ENULL
    # heat-map packing
    views = (C.c_void_p * 17)(*([d] * 17))
    holes = (C.c_void_p * 2)(d, None)
    pack = lambda v=views, out=d, ib=0, ob=0, B=1, V=1, J=4, Jp=4, h=4, w=4: lib.sp3d_pack_heatmaps_ex(v, out, ib, ob, B, V, J, Jp, h, w, None)
    assert pack(B=0) == EINVAL and pack(V=0) == EINVAL and pack(V=17) == EINVAL and pack(J=0) == EINVAL and pack(h=0) == EINVAL
    assert pack(out=None) == ENULL and pack(v=None) == ENULL and pack(v=holes, V=2) == ENULL
    assert pack(J=5, Jp=4) == EUNSUPPORTED and pack(J=5, Jp=6) == EUNSUPPORTED and pack(Jp=20) == EUNSUPPORTED
    for ib, ob in ((1, 0), (0, 1), (1, 1)):                          # bf16 needs Jp == 16 or 32
        assert all(pack(ib=ib, ob=ob, Jp=jp) == EUNSUPPORTED for jp in (4, 8, 12))
    assert lib.sp3d_pack_heatmaps(views, None, 1, 1, 4, 4, 4, 4, None) == ENULL
    # channel shift + activation
    csa = lambda y=d, s=d, r=d, mode=0, batch=1, Cc=4, inner=4, cl=0: lib.sp3d_channel_shift_act(y, s, r, mode, batch, Cc, inner, cl, None)
    assert csa(batch=0) == EINVAL and csa(Cc=0) == EINVAL and csa(inner=0) == EINVAL and csa(mode=-1) == EINVAL and csa(mode=4) == EINVAL
    assert csa(y=None) == ENULL and csa(s=None) == ENULL and csa(r=None, mode=2) == ENULL and csa(r=None, mode=3) == ENULL
    assert csa(inner=6) == EUNSUPPORTED and csa(Cc=6, cl=1) == EUNSUPPORTED
    assert gs.csa_refusal(4, 6, 0) == EUNSUPPORTED and gs.csa_refusal(6, 4, 1) == EUNSUPPORTED
    # max-pool
    pool = lambda x=d, y=d, B=1, X=2, Y=2, Z=2, Cc=4: lib.sp3d_maxpool2x_cl(x, y, B, X, Y, Z, Cc, None)
    assert pool(B=0) == EINVAL and pool(X=1) == EINVAL and pool(Y=0) == EINVAL and pool(Z=1) == EINVAL and pool(Cc=0) == EINVAL
    assert pool(x=None) == ENULL and pool(y=None) == ENULL
    assert pool(Cc=6) == EUNSUPPORTED and pool(X=3) == EUNSUPPORTED and pool(Y=5) == EUNSUPPORTED and pool(Z=7) == EUNSUPPORTED
    assert gs.pool_refusal(1, 3, 2, 2, 4) == EUNSUPPORTED and gs.pool_refusal(1, 1, 2, 2, 4) == EINVAL
    # fixed point -> float
    fix = lambda acc=d, out=d, scale=d, n=1: lib.sp3d_fixed_to_float(acc, out, scale, n, None)
    assert fix(n=0) == EINVAL and fix(n=-5) == EINVAL and fix(acc=None) == ENULL and fix(out=None) == ENULL and fix(scale=None) == ENULL
    assert fix(n=2 ** 39 + 1) == ERANGE
    # fetch ring
    ring = lambda r=d, dst=d, cnt=d, R=1, n=4: lib.sp3d_fetch_ring(r, dst, cnt, R, n, None)
    assert ring(R=0) == EINVAL and ring(n=0) == EINVAL and ring(r=None) == ENULL and ring(dst=None) == ENULL and ring(cnt=None) == ENULL
    # up-conv scatter
    sc = lambda G=d, out=d, s=d, k=d, batch=1, X=1, Y=1, Z=1, O=4: lib.sp3d_upsample2x_scatter(G, out, s, k, batch, X, Y, Z, O, None)
    assert sc(batch=0) == EINVAL and sc(X=0) == EINVAL and sc(Y=0) == EINVAL and sc(Z=0) == EINVAL and sc(O=0) == EINVAL
    assert sc(G=None) == ENULL and sc(out=None) == ENULL and sc(s=None) == ENULL and sc(k=None) == ENULL and sc(O=6) == EUNSUPPORTED
    hd = lambda G=d, out=d, s=d, k=d, w=d, b=d, batch=1, O=32, J=1: lib.sp3d_upsample2x_scatter_head(G, out, s, k, w, b, batch, 1, 1, 1, O, J, None)
    assert hd(batch=0) == EINVAL and hd(J=0) == EINVAL and hd(O=0) == EINVAL
    assert hd(G=None) == ENULL and hd(out=None) == ENULL and hd(w=None) == ENULL and hd(b=None) == ENULL
    assert hd(O=64) == EUNSUPPORTED and hd(O=16) == EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
# H. the ledger: which test modules sweep which C-ABI entry
# ---------------------------------------------------------------------------------------------------------------------------
HOST_ONLY, LIBRARY = "host only", "library transform (hipFFT)"
_UNPROJECT_FWD = ("test_gpu_fwd_option_sweep", "test_gpu_random_sweep")
_PROPOSAL, _CONV, _FRONT, _GLUE, _TRAIN = ("test_gpu_proposal_sweep",), ("test_gpu_conv_sweep",), ("test_gpu_front_sweep",), \
    ("test_gpu_glue_sweep",), ("test_gpu_train_sweep",)
LEDGER = {
    "sp3d_abi_version": HOST_ONLY, "sp3d_camera_finish": HOST_ONLY, "sp3d_error_string": HOST_ONLY,
    "sp3d_gbn_workspace_bytes": HOST_ONLY, "sp3d_nms_topk_workspace_bytes": HOST_ONLY,
    "sp3d_rfft3d": LIBRARY, "sp3d_irfft3d": LIBRARY, "sp3d_cfft2d": LIBRARY,
    "sp3d_pack_heatmaps": _GLUE, "sp3d_pack_heatmaps_ex": _GLUE,
    "sp3d_unproject_fwd": _GLUE, "sp3d_unproject_fwd_indexed": _UNPROJECT_FWD,
    "sp3d_unproject_fwd_strided": _UNPROJECT_FWD, "sp3d_unproject_fwd_train": ("test_gpu_bwd_random_sweep",),
    "sp3d_unproject_fwd_zdft": _FRONT,
    "sp3d_unproject_bwd": _GLUE, "sp3d_unproject_bwd_indexed": ("test_gpu_bwd_random_sweep",),
    "sp3d_unproject_bwd_packed": ("test_gpu_bwd_random_sweep", "test_gpu_wide_grad"),
    "sp3d_unproject_bwd_packed_det": ("test_gpu_bwd_random_sweep", "test_gpu_wide_grad"),
    "sp3d_fixed_to_float": _GLUE,
    "sp3d_unproject_one_fwd_train": ("test_gpu_one_channel_grad",), "sp3d_unproject_one_bwd": ("test_gpu_one_channel_grad",),
    "sp3d_unproject_one_bwd_det": ("test_gpu_one_channel_grad",),
    "sp3d_nms_topk": _PROPOSAL, "sp3d_nms_proposals": _PROPOSAL, "sp3d_soft_argmax": _PROPOSAL, "sp3d_soft_argmax_grid": _PROPOSAL,
    "sp3d_soft_argmax_grid_train": _PROPOSAL, "sp3d_soft_argmax_grid_bwd": _PROPOSAL,
    "sp3d_channel_shift_act": _GLUE, "sp3d_fetch_ring": _GLUE, "sp3d_maxpool2x_cl": _GLUE,
    "sp3d_crop_shift_act_cl": _FRONT, "sp3d_zdft_fwd_cl": _FRONT, "sp3d_zdft_inv_cl": _FRONT, "sp3d_cfft2d_ex": _FRONT,
    "sp3d_cfft2d_88_tiled": _FRONT, "sp3d_freq_contract": _FRONT, "sp3d_freq_contract_ex": _FRONT, "sp3d_freq_contract_ty": _FRONT,
    "sp3d_gbn_forward": _TRAIN, "sp3d_gbn_backward": _TRAIN, "sp3d_gaussian_target_3d": _TRAIN,
    "sp3d_render_root_heatmaps": _TRAIN, "sp3d_render_joints_fwd": _GLUE, "sp3d_render_joints_bwd": _GLUE,
    "sp3d_wino_input": _CONV, "sp3d_wino_output": _CONV, "sp3d_wino_fused": _CONV, "sp3d_wino_fused_split": _CONV,
    "sp3d_wino_fused_split64": _CONV, "sp3d_wino_fused_split64_skip": _CONV, "sp3d_conv3_split": _CONV,
    "sp3d_conv3_split_skip": _CONV, "sp3d_upconv2x_fused": _CONV,
    "sp3d_upsample2x_scatter": _CONV + _GLUE, "sp3d_upsample2x_scatter_head": _CONV + _GLUE,
}
# the _lib function a module calls where it does not name the C entry itself.  sp3d_unproject_fwd and sp3d_unproject_bwd are the
# one-line forms of their _indexed entries with sample_of = NULL: the glue sweep shows that they hand their arguments on
WRAPPERS = {
    "sp3d_unproject_fwd_indexed": "unproject_fwd", "sp3d_unproject_fwd_strided": "unproject_fwd", "sp3d_unproject_fwd_train": "unproject_fwd",
    "sp3d_unproject_fwd_zdft": "unproject_fwd_zdft", "sp3d_unproject_bwd_indexed": "unproject_bwd",
    "sp3d_unproject_bwd_packed": "unproject_bwd_packed", "sp3d_unproject_bwd_packed_det": "unproject_bwd_packed",
    "sp3d_unproject_one_bwd_det": "unproject_one_bwd", "sp3d_soft_argmax_grid_bwd": "soft_argmax_grid_autograd",
    "sp3d_soft_argmax_grid_train": "soft_argmax_grid_autograd", "sp3d_cfft2d_ex": "cfft2d_",
    "sp3d_wino_input": "wino_conv3d_", "sp3d_wino_output": "wino_conv3d_", "sp3d_wino_fused": "wino_fused_conv3d_",
    "sp3d_wino_fused_split": "wino_fused_conv3d_", "sp3d_wino_fused_split64": "wino_fused_conv3d_",
    "sp3d_wino_fused_split64_skip": "wino_fused_conv3d_", "sp3d_conv3_split": "conv3_split_", "sp3d_conv3_split_skip": "conv3_split_",
    "sp3d_upconv2x_fused": "upsample2x_", "sp3d_upsample2x_scatter": "upsample2x_", "sp3d_upsample2x_scatter_head": "upsample2x_head_",
    "sp3d_nms_topk": "nms_topk", "sp3d_nms_proposals": "nms_proposals", "sp3d_soft_argmax": "soft_argmax",
    "sp3d_soft_argmax_grid": "soft_argmax_grid", "sp3d_crop_shift_act_cl": "crop_shift_act_cl", "sp3d_zdft_fwd_cl": "zdft_fwd_cl",
    "sp3d_zdft_inv_cl": "zdft_inv_cl", "sp3d_cfft2d_88_tiled": "cfft2d_88_tiled", "sp3d_freq_contract": "freq_contract",
    "sp3d_freq_contract_ex": "freq_contract_ex", "sp3d_freq_contract_ty": "freq_contract_ty",
    "sp3d_gaussian_target_3d": "gaussian_target_3d", "sp3d_render_root_heatmaps": "render_root_heatmaps",
    "sp3d_unproject_one_fwd_train": "unproject_one_fwd_train", "sp3d_unproject_one_bwd": "unproject_one_bwd",
}


def test_every_c_abi_entry_names_its_sweep():
    from selfpose3d_amd import _lib
    declared = sorted(_header_signatures(os.path.join(ROOT, "include", "sp3d.h")))
    assert sorted(LEDGER) == declared, sorted(set(LEDGER) ^ set(declared))               # no entry without a line, no stale line
    for entry, where in LEDGER.items():
        if isinstance(where, str):
            assert where in (HOST_ONLY, LIBRARY), entry
            continue
        for module in where:
            path = os.path.join(ROOT, "tests", module + ".py")
            assert os.path.exists(path), (entry, module)                                 # the module exists
            src = open(path).read()
            wrapper = WRAPPERS.get(entry)
            assert wrapper is None or hasattr(_lib, wrapper), (entry, wrapper)
            # and it names what it sweeps, as a whole word: sp3d_freq_contract_ex does not stand for sp3d_freq_contract
            named = re.search(r"\b%s\b" % entry, src) or (wrapper and re.search(r"\b_lib\.%s\(" % wrapper, src))
            assert named, (entry, module)
