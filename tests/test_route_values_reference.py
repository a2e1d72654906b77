"""The CPU side of the route value census (tests/route_value_cases.py): which cases run, that the module's written-out rules
agree with ``ProjectLayer.route`` and with the census file, that every case carries signal, that the referees agree with
independent restatements, and that ``compare_case`` rejects planted errors - all without a GPU, from the oracle alone."""
import numpy as np
import pytest
import torch

from tests import route_cases as rc
from tests import route_value_cases as rv
from tests.front_sweep_cases import PARITY_CAP, untile44

CASES = rv.cases()
RUN = [cid for cid, c in CASES.items() if not rv.raises(c)]


def _layer(c):
    layer = rc.build_layer(c)
    layer.bf16_train = "bf16_train" in c["sw"]
    return layer


def _calls(c):
    return range(rv.repeats(c))


# ---- which cases run ----------------------------------------------------------------------------------------------------------
def test_no_silent_skip():
    """left out of the value run are exactly the layer-level census cases whose outcome (``intended`` applied) is a raise, and
    no case of the module's own"""
    census = rv.census()
    layer_ids = [rc.case_id(c) for c in rc.layer_cases()]
    raising = sorted(cid for cid in layer_ids if isinstance(census[cid], list))
    left_out = sorted(cid for cid, c in CASES.items() if rv.raises(c))
    print("%d cases, %d run, %d left out:" % (len(CASES), len(RUN), len(left_out)))
    for cid in left_out:
        print("  left out (%s): %s" % (census[cid][1][:60], cid))
    assert left_out == raising and len(left_out) == len(raising) == len(CASES) - len(RUN)
    assert not any(c.get("own") for c in CASES.values() if rv.raises(c))
    own = [c for c in CASES.values() if c.get("own")]
    assert len(own) == 20 and len(CASES) == len(layer_ids) + 20
    assert {(c["J"], c["hand"]) for c in own} == {(15, "nhwc_bf16"), (17, "nhwc_bf16"), (32, "nhwc_bf16"), (1, "slice_nhwc_bf16"),
                                                   (1, "planar_bf16")}


def test_inputs_follow_the_index():
    """flip on every second case; of the non-``sample_of`` cases every third has centres per sample, every other one of those
    an invalid sample 1; the second call of a repeated case has new values of the same shapes"""
    per = [c for c in CASES.values() if c["centres"] in ("per_sample", "invalid1")]
    assert all(c["idx"] % 3 == 0 and c["call"] != "sample_of" for c in per)
    assert [c["centres"] for c in per] == ["per_sample", "invalid1"] * (len(per) // 2) + ["per_sample"] * (len(per) % 2)
    assert all(c["flip"] == (c["idx"] % 2 == 1) for c in CASES.values())
    assert all((c["centres"] == "sample_of") == (c["call"] == "sample_of") for c in CASES.values())
    ran = [CASES[cid] for cid in RUN]
    for kind in ("shared", "per_sample", "invalid1", "sample_of"):
        for flip in (False, True):
            assert any(c["centres"] == kind and c["flip"] == flip for c in ran), (kind, flip)
    for c in ran:
        if rv.repeats(c) == 2:
            a, b = rv.leaf_arrays(c, 0), rv.leaf_arrays(c, 1)
            assert all(x.shape == y.shape and not np.array_equal(x, y) for x, y in zip(a, b))
        for a in rv.leaf_arrays(c):
            assert a.min() >= -0.3 - 2 ** -9 and a.max() <= 1.3 + 2 ** -8 and (a < 0).any() and (a > 1).any()
        if "nhwc" in c["hand"]:
            Jn = rv.SLICE_OF if c["hand"].startswith("slice") else c["J"]
            assert not rv.leaf_arrays(c)[0][..., Jn:].any()


# ---- the rules against the record and the census file ------------------------------------------------------------------------------
def _route(c):
    layer = _layer(c)
    leaves = rv.make_leaves(c, rv.leaf_arrays(c), "cpu")
    hms = rv.views_of(c, leaves)
    with rc.grad_context(c):
        if c["call"] == "zspectrum":
            return layer.route(hms, rc.SZ), hms
        _, kw = rc.call_kwargs(c, "cpu")
        return layer.route(hms, None, kw["want_grids"], kw["pad_channels"], kw["channels_last"], "out" in kw), hms


def test_rules_agree_with_the_record():
    """two independently written tables: ``sees_rounded`` / ``masked`` / ``result_form`` here, ``Route`` there"""
    counts = dict(rounded=0, masked=0, one=0, cl=0)
    for cid in RUN:
        c = CASES[cid]
        route, hms = _route(c)
        rounded = hms[0].dtype == torch.bfloat16 or route.elem == torch.bfloat16
        assert rv.sees_rounded(c) == rounded, cid
        assert rv.masked(c) == (route.backward in ("mask16", "mask2x16", "one")), cid
        assert rv.wants_grad(c) == (route.backward != "none"), cid
        assert (route.layout == 1 or route.read == "one") == (rv.nhwc_path(c) or c["call"] == "zspectrum") or route.read == "planar", cid
        assert (route.read == "planar") == (not rv.nhwc_path(c) and c["call"] != "zspectrum"), cid
        _, shape, strides = rv.result_form(c)
        assert route.J == shape[1], cid
        if c["call"] != "zspectrum":
            assert route.channels_last == (strides[1] == 1 and shape[1] > 1), cid
            assert route.out == (c["call"] == "out"), cid
        counts["rounded"] += rounded
        counts["masked"] += rv.masked(c)
        counts["one"] += route.read == "one"
        counts["cl"] += route.channels_last
    print(counts)
    assert min(counts.values()) >= 10, counts


def test_result_form_is_what_the_census_records():
    census = rv.census()
    for cid in RUN:
        c = CASES[cid]
        if c.get("own"):
            continue
        dtype, shape, strides = rv.result_form(c)
        results = census[cid]["result"]
        assert len(results) == rv.repeats(c), cid
        for r in results:
            assert r[0][:2] == [dtype, list(shape)], (cid, r[0], dtype, shape)
            assert rv.same_strides(shape, r[0][2], strides), (cid, r[0], strides)
            if c["call"] != "zspectrum":
                assert (r[1] is not None) == rv.returns_grids(c), cid
                if rv.wants_grad(c):
                    assert r[0][3] and all(g is not None for g in r[-1]), cid      # every leaf got a gradient


def test_own_cases_take_the_routes_they_are_about():
    for cid in RUN:
        c = CASES[cid]
        if not c.get("own"):
            continue
        route, _ = _route(c)
        on = "bf16_train" in c["sw"]
        assert route.elem == (torch.bfloat16 if on else torch.float32), cid
        one = c["J"] == 1 and on          # switch off: bf16 tensors do not classify as an fp32 slice, the packed route widens them
        assert route.backward == ("one" if one else ("mask2x16" if c["J"] > 16 else "mask16")), cid
        assert route.read == ("one" if one else "packed"), cid


# ---- signal ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", RUN)
def test_signal(cid):
    """from the oracle alone: every valid cube is seen, both clamps act and most values are inside, every channel's reference
    gradient is non-zero in every view; where the referee is on rounded maps, the oracle on unrounded maps gives other cubes"""
    c = CASES[cid]
    for call_no in _calls(c):
        e = rv.expected(cid, call_no)
        ok = e.valid > 0
        for p in np.flatnonzero(ok):
            assert e.seen[p].mean() >= 0.30, (call_no, p, e.seen[p].mean())
        vals = e.cubes[ok].transpose(1, 0, 2, 3, 4)[:, e.seen[ok]]
        clamped, inside = float(((vals == 0) | (vals == 1)).mean()), float(((vals > 0) & (vals < 1)).mean())
        assert clamped >= 0.05 and inside >= 0.30, (call_no, clamped, inside)
        assert (vals == 0).any() and (vals == 1).any()
        assert not e.cubes[~ok].any()
        if rv.wants_grad(c):
            nz = np.abs(e.per_view).max(axis=(1, 3, 4))          # (V, J)
            assert nz.shape == (rv.V, c["J"]) and (nz > 0).all(), nz
            if c["centres"] == "invalid1":
                assert not e.per_view[:, 1].any() and e.per_view[:, 0].any()
        raw = rv.logical_maps(c, e.arrays)
        if rv.sees_rounded(c) and c["hand"] not in rv.BF16_HANDS:      # bf16 tensors have no unrounded maps to confuse them with
            other = rv.oracle_cubes(c, raw, want_grids=False)[0]
            mine = rv.oracle_cubes(c, e.maps, want_grids=False)[0]
            nonzero = (mine != 0) | (other != 0)
            assert (mine != other)[nonzero].mean() > 0.5, (mine != other)[nonzero].mean()


def test_flip_reaches_the_values():
    """the unflipped table gives other cubes wherever sample 1 is read, the same ones for sample 0"""
    n = 0
    for cid in RUN[:60]:
        c = CASES[cid]
        if not c["flip"]:
            continue
        e = rv.expected(cid)
        flipped = rv.oracle_cubes(c, e.maps, want_grids=False)[0]
        plain = rv.oracle_cubes(c, e.maps, flip=False, want_grids=False)[0]
        for p, b in enumerate(e.so):
            if b == 0 or not e.valid[p]:
                assert np.array_equal(flipped[p], plain[p]), cid
            else:
                assert (flipped[p] != plain[p])[flipped[p] != 0].mean() > 0.5, cid
                n += 1
    assert n >= 10


# ---- referee against referee -----------------------------------------------------------------------------------------------------
def _restated_grads(c, maps, weights):
    """float64 torch autograd through a plain restatement of the reference's ``get_voxel``: the oracle's grids and its fp32
    pixel projection, then clamp, crop affine, flip, normalisation and clamp to +-1.1 (reference project_layer.py:78-90) written
    out in fp32 numpy, ``F.grid_sample`` (bilinear, zeros, align_corners) on float64 maps, the bounding-weighted mean over the
    views, clamp(0, 1) - and autograd for the gradient of (cubes * W).sum()"""
    from oracle import oracle
    import torch.nn.functional as F
    cam, centres, valid, so = rv.geometry(c)
    w, h = rc.hm_size(c)
    W_in, H_in = rc.IMG
    f = np.float32
    _, grids = rv.oracle_cubes(c, maps)
    leaves = [torch.from_numpy(m.astype(np.float64)).requires_grad_(True) for m in maps]
    fma = lambda a, b, acc: (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(f)
    total = 0.0
    for p in range(len(so)):
        if not valid[p]:
            continue
        acc, cnt = 0.0, np.zeros(rv.N, f)
        for v in range(rv.V):
            cm = cam[p, v]
            px = oracle.project_points(cm, grids[p])
            x, y = px[:, 0], px[:, 1]
            W0, H0 = cm[27], cm[28]
            bound = ((x >= 0) & (y >= 0) & (x < W0) & (y < H0)).astype(f)
            mx = max(W0, H0)
            x, y = np.clip(x, f(-1), mx), np.clip(y, f(-1), mx)
            A = cm[21:27]
            qx = fma(np.full_like(x, A[2]), np.ones_like(x), fma(np.full_like(x, A[1]), y, A[0] * x))
            qy = fma(np.full_like(x, A[5]), np.ones_like(x), fma(np.full_like(x, A[4]), y, A[3] * x))
            if cm[29] != 0:
                qx = f(W_in) - qx
            gx = np.clip(qx * f(w) / f(W_in) / f(w - 1) * f(2) - f(1), f(-1.1), f(1.1))
            gy = np.clip(qy * f(h) / f(H_in) / f(h - 1) * f(2) - f(1), f(-1.1), f(1.1))
            grid = torch.from_numpy(np.stack([gx, gy], 1).astype(np.float64)).reshape(1, 1, rv.N, 2)
            val = F.grid_sample(leaves[v][so[p]:so[p] + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            acc = acc + val[0, :, 0] * torch.from_numpy(bound.astype(np.float64))
            cnt = cnt + bound
        den = torch.from_numpy((cnt + f(1e-6)).astype(np.float64))
        cube = (acc / den).clamp(0.0, 1.0)                        # (J, N)
        total = total + (cube * torch.from_numpy(weights[p, :cube.shape[0]].reshape(-1, 1).astype(np.float64))).sum()
    total.backward()
    return np.stack([x.grad.numpy() for x in leaves])              # (V,B,J,h,w): autograd adds the rows of a sample itself


@pytest.mark.parametrize("want", [dict(J=1, hand="slice_planar"), dict(J=15, hand="planar"), dict(J=17, call="sample_of")],
                         ids=["J1-slice", "J15", "J17-sample_of"])
def test_backward_referee_against_autograd(want):
    """on the geometry, maps and weights of a case (whether or not the layer runs it or it asks for a gradient: the census has
    no 17-joint ``sample_of`` case that does not raise, and the referees do not care)"""
    cid = next(k for k in CASES if CASES[k]["call"] != "zspectrum" and all(CASES[k][a] == b for a, b in want.items()))
    c = CASES[cid]
    e = rv.expected(cid)
    weights = rv.loss_weights(c)
    ref = rv.oracle_grads(c, e.maps, weights)
    got = _restated_grads(c, e.maps, weights)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("%s: max|autograd - oracle| = %.3g, max|ref| = %.3g" % (cid, err, scale))
    assert scale > 0 and err <= 1e-6 * scale


def test_dft_referee_against_a_dft_matrix():
    g = np.random.default_rng(3)
    cubes = g.random((2, 3, rv.X, rv.Y, rv.Z))
    k, n = np.arange(rv.KZ)[:, None], np.arange(rv.Z)[None, :]
    F = np.exp(-2j * np.pi * k * n / rv.SZ)                       # (KZ, Z): bins 0..SZ//2 of the SZ-point DFT of a row of Z values
    want = np.einsum("kz,pjxyz->pjkxy", F, cubes)
    got = rv.z_spectrum(cubes)
    assert got.shape == (2, 3, rv.KZ, rv.X // 4, rv.Y // 4, 16) and got.dtype == np.complex128
    back = untile44(torch.from_numpy(got), rv.X, rv.Y).numpy()    # the untiling helper of the front tests
    assert np.abs(back - want).max() <= 1e-12 * np.abs(want).max()
    assert rv.PARITY_CAP == PARITY_CAP


# ---- compare_case rejects planted errors ----------------------------------------------------------------------------------------
def _oracle_got(e, deterministic=False):
    """the oracle's own outputs in the form the GPU test hands ``compare_case``"""
    got = dict(deterministic=deterministic)
    if e.spectrum is not None:
        got["spectrum"] = e.spectrum.astype(np.complex64)
        return got
    want = e.cube_bits()
    cubes = np.zeros(e.shape, want.dtype)
    cubes[:, :e.J] = want
    got["cubes"], got["grids"] = cubes, e.grid_bits()
    if rv.wants_grad(e.c):
        got["grads"] = [r.copy() for r in e.ref]
        if e.leaf_dtype == "bfloat16":
            got["grads"] = [torch.from_numpy(r).to(torch.bfloat16).double().numpy() for r in e.ref]
        got["grad_dtypes"] = [e.leaf_dtype] * len(e.ref)
        got["again"] = [g.copy() for g in got["grads"]]
    return got


def _names(e, got):
    return sorted({name for name, _ in rv.compare_case(e, got)})


def _pick(**want):
    return next(k for k in RUN if all((CASES[k].get(a) == b) if a not in ("sw_has",) else (b in CASES[k]["sw"]) for a, b in want.items()))


@pytest.mark.parametrize("cid", RUN)
def test_the_oracle_passes_its_own_comparison(cid):
    for call_no in _calls(CASES[cid]):
        e = rv.expected(cid, call_no)
        for det in (False, True):
            assert rv.compare_case(e, _oracle_got(e, det)) == [], cid


def test_planted_errors_are_rejected():
    # two channels swapped
    e = rv.expected(_pick(J=15, call="plain", io="fp32"))
    got = _oracle_got(e)
    got["cubes"][:, [3, 4]] = got["cubes"][:, [4, 3]]
    assert _names(e, got) == ["cubes:bits"]
    # one voxel off by one fp32 ulp
    got = _oracle_got(e)
    p, j, x, y, z = np.argwhere((e.cubes > 0) & (e.cubes < 1))[7]
    got["cubes"][p, j, x, y, z] += 1
    assert _names(e, got) == ["cubes:bits"]
    # grids off by one ulp
    got = _oracle_got(e)
    got["grids"] = got["grids"].copy()
    got["grids"][0, 5, 1] += 1
    assert _names(e, got) == ["grids:bits"]
    # a non-zero pad channel
    e = rv.expected(_pick(J=13, call="pad_cl", io="fp32")) if any(CASES[k]["J"] == 13 and CASES[k]["call"] == "pad_cl" for k in RUN) \
        else rv.expected(_pick(J=15, call="pad_cl", io="fp32"))
    assert e.shape[1] == 16
    got = _oracle_got(e)
    got["cubes"][1, e.J, 2, 3, 4] = np.float32(1e-30).view(np.int32)
    assert _names(e, got) == ["cubes:pad"]
    # the unflipped table's cubes
    cid = next(k for k in RUN if CASES[k]["flip"] and CASES[k]["call"] == "plain" and CASES[k]["io"] == "fp32" and CASES[k]["centres"] == "shared")
    e = rv.expected(cid)
    got = _oracle_got(e)
    got["cubes"][:, :e.J] = rv.bits(rv.oracle_cubes(e.c, e.maps, flip=False)[0], e.dtype)
    assert _names(e, got) == ["cubes:bits"]
    # two views' gradients swapped
    cid = next(k for k in RUN if rv.wants_grad(CASES[k]) and CASES[k]["hand"] == "planar" and CASES[k]["J"] == 15)
    e = rv.expected(cid)
    got = _oracle_got(e)
    got["grads"][0], got["grads"][1] = got["grads"][1], got["grads"][0]
    got["again"] = [g.copy() for g in got["grads"]]
    assert "grad:bound" in _names(e, got) and "cubes:bits" not in _names(e, got)
    # the same through an nhwc buffer: views 0 and 1 of the one leaf
    cid = next(k for k in RUN if rv.wants_grad(CASES[k]) and CASES[k]["hand"] in ("nhwc", "nhwc_bf16"))
    e = rv.expected(cid)
    got = _oracle_got(e)
    got["grads"][0][[0, 1]] = got["grads"][0][[1, 0]]
    assert "grad:bound" in _names(e, got)
    # a gradient in a channel outside the slice
    for hand in ("slice_planar", "slice_nhwc", "slice_nhwc_bf16", "planar_bf16"):
        cid = next(k for k in RUN if rv.wants_grad(CASES[k]) and CASES[k]["hand"] == hand)
        e = rv.expected(cid)
        got = _oracle_got(e)
        g = got["grads"][0]
        if g.ndim == 5:
            g[0, 0, 3, 4, 0] = 1e-20            # channel 0 instead of channel 2
        else:
            g[0, 0, 3, 4] = 1e-20
        assert "grad:outside_slice" in _names(e, got), hand
        # ... and channel 0's values handed back in place of channel 2's
        got = _oracle_got(e)
        g = got["grads"][0]
        if g.ndim == 5:
            g[..., 0], g[..., rv.SLICE_CH] = g[..., rv.SLICE_CH].copy(), 0
        else:
            g[:, 0], g[:, rv.SLICE_CH] = g[:, rv.SLICE_CH].copy(), 0
        assert "grad:outside_slice" in _names(e, got), hand
    # a gradient of sample 1 when it is invalid
    cid = next(k for k in RUN if rv.wants_grad(CASES[k]) and CASES[k]["centres"] == "invalid1" and CASES[k]["hand"] != "expanded")
    e = rv.expected(cid)
    got = _oracle_got(e)
    live = np.argwhere(e.inside[0])
    idx = tuple(next(i for i in live if e.dead[0][tuple(i)]))
    got["grads"][0][idx] = 1e-12
    assert "grad:no_valid_cube" in _names(e, got)
    # a bf16 leaf that got the fp32 gradient of the widened copy (dtype), an fp32 gradient rounded twice (bound)
    cid = next(k for k in RUN if CASES[k].get("own") and "bf16_train" in CASES[k]["sw"])
    e = rv.expected(cid)
    got = _oracle_got(e)
    got["grad_dtypes"] = ["float32"]
    assert _names(e, got) == ["grad:dtype"]
    # a deterministic backward that differs run to run, and one beyond the deterministic bound but inside the fp32 one
    cid = next(k for k in RUN if rv.masked(CASES[k]) and CASES[k]["hand"] == "planar" and CASES[k]["J"] == 15)
    e = rv.expected(cid)
    got = _oracle_got(e, deterministic=True)
    i = tuple(np.argwhere(e.S[0] > 0)[3])
    got["again"][0][i] += 1e-9
    assert _names(e, got) == ["grad:det_repeat"]
    got = _oracle_got(e, deterministic=True)
    got["grads"][0][i] += 0.5 * (e.T + 4) * 2.0 ** -24 * e.S[0][i]
    got["again"] = [g.copy() for g in got["grads"]]
    assert _names(e, got) == ["grad:det_bound"]
    assert rv.compare_case(e, dict(got, deterministic=False)) == []
    # an expanded leaf that got one sample's gradient, not the sum over B
    cid = next((k for k in RUN if rv.wants_grad(CASES[k]) and CASES[k]["hand"] == "expanded"), None)
    if cid is not None:
        e = rv.expected(cid)
        got = _oracle_got(e)
        got["grads"] = [e.per_view[v][:1].copy() for v in range(rv.V)]
        assert "grad:bound" in _names(e, got)
    # a spectrum of an invalid sample, a spectrum beyond the cap
    cid = next(k for k in RUN if CASES[k]["call"] == "zspectrum" and CASES[k]["centres"] == "invalid1")
    e = rv.expected(cid)
    got = _oracle_got(e)
    got["spectrum"][1, 0, 0, 0, 0, 0] = 1e-9
    assert _names(e, got) == ["spectrum:invalid"]
    got = _oracle_got(e)
    got["spectrum"][0, 0, 3, 1, 1, 5] += 4e-6 * max(1.0, np.abs(e.spectrum[0]).max())
    assert _names(e, got) == ["spectrum:tol"]
