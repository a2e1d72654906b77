"""Cases, inputs, CPU referee and comparison of the route VALUE census (tests/test_route_values_reference.py proves this side
on the CPU, tests/test_gpu_route_values.py runs every case through ``ProjectLayer.get_voxel`` / ``get_voxel_zspectrum`` on the
GPU).  Plain helper module: no pytest hooks, no GPU, every input generated from fixed seeds.

tests/test_gpu_route_census.py holds the ``_lib`` CALLS of every route to a recording; this module holds the NUMBERS of the
same cases to the oracle: which maps are packed, widened or rounded, which buffer is cached, which channel of a slice is read,
where pad channels go, how ``sample_of``, ``out``, float64 callers and bf16 leaves travel, how gradients of slices and expanded
leaves are reduced.

Cases: every case of ``route_cases.layer_cases()`` (the census geometry: 24 x 18 maps, image 96 x 72, V = 3, B = 2, cube
(8, 12, 20), SZ = 28, space (8000, 8000, 2000)) and OWN cases the recording of an old commit cannot hold: ``bf16_train`` alone,
with ``wide_grad`` and with ``one_channel_grad`` (two new hand-overs: a slice of a bf16 NHWC buffer, a slice of planar bf16
tensors), each with the switch on and off, each as ``pad_cl`` and ``plain``.

Inputs: cameras of ``synthetic.random_meta(..., augment=True)``; a ``flip_xcoords`` tensor (flip on sample 1 only) on every
second case; of the cases that are no ``sample_of`` call every third passes a (B,5) centre tensor with a centre per sample, and
every other one of those marks sample 1 invalid; ``sample_of`` cases keep [0,1,1] and get three centres.  Maps uniform in
[-0.3, 1.3) (both clamps act), seeded per case id and call; the second call of a ``twice`` / ``capture`` case gets new values
in the same storage.  Loss = (cubes.float() * W).sum(), W = bf16_round(randn) * 2^k, k integer in [-6, 3], per (cube, channel):
bf16-representable, so bf16 cubes carry exactly W as their gradient.

Which maps the kernel must see is stated HERE, by ``sees_rounded`` (not read from ``Route``); which gradients get the
deterministic bound by ``masked``; the shape / strides / dtype of the result by ``result_form``.  The CPU test cross-checks the
three against ``ProjectLayer.route`` and the census file - two independently written tables.

Referees: ``oracle.unproject_fwd`` on the gathered batch (bf16 cubes: its result rounded RNE); the complex128 DFT along z of
its cubes, zero-padded to SZ, bins 0..SZ//2, 4 x 4-tiled; ``oracle.unproject_bwd`` with grad_cubes = W, rows added into their
samples, S the same with |W|, T = 4 N max cubes per sample, det_step = 2^(ceil(log2 max|W|) - 40)."""
import functools
import json
import math
import os
import zlib

import numpy as np

from tests import route_cases as rc
from tests.fwd_option_sweep_cases import bf16_round

B, V, P3 = rc.B, rc.V, rc.P
X, Y, Z = rc.CUBE
N = X * Y * Z
SZ, KZ = rc.SZ, rc.SZ // 2 + 1
META_SEED = 16                                           # see test_route_values_reference.py::test_signal: changed HERE if it misses
CENTRES2 = ((300.0, -900.0, 700.0), (-500.0, -100.0, 900.0))                # one per sample
CENTRES3 = ((300.0, -900.0, 700.0), (-500.0, -100.0, 900.0), (100.0, -400.0, 1000.0))       # one per cube of sample_of = [0,1,1]
SAMPLE_OF = (0, 1, 1)
BF16_HANDS = ("nhwc_bf16", "slice_nhwc_bf16", "planar_bf16")
SLICE_OF, SLICE_CH = 15, 2                               # a slice hand-over is channel 2 of 15
PARITY_CAP = 3e-6                                        # front_sweep_cases.PARITY_CAP: the project's figure for its FFT kernels


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _own_cases():
    out = []
    for J, hand, sw in ((15, "nhwc_bf16", ()), (17, "nhwc_bf16", ("wide_grad",)), (32, "nhwc_bf16", ("wide_grad",)),
                        (1, "slice_nhwc_bf16", ("one_channel_grad",)), (1, "planar_bf16", ("one_channel_grad",))):
        for on in (True, False):
            for call in ("pad_cl", "plain"):
                out.append(dict(rc.BASE, J=J, hand=hand, grad="required", sw=(("bf16_train",) if on else ()) + sw, call=call, own=True))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """{id: case}, the census' layer cases in their order, then the own ones ("own:" in front of the id); a case knows its
    index (``idx``) and what the index decides: ``flip`` and ``centres``"""
    out, k = {}, 0
    for c in [dict(c) for c in rc.layer_cases()] + _own_cases():
        cid = ("own:" if c.get("own") else "") + rc.case_id(c)
        assert cid not in out, cid
        c["id"], c["idx"] = cid, len(out)
        c["flip"] = c["idx"] % 2 == 1
        if c["call"] == "sample_of":
            c["centres"] = "sample_of"
        elif c["idx"] % 3 == 0:
            c["centres"] = "invalid1" if k % 2 else "per_sample"
            k += 1
        else:
            c["centres"] = "shared"
        out[cid] = c
    return out


@functools.lru_cache(maxsize=None)
def census():
    """{id: outcome} of the layer-level cases of tests/golden/route_census.json, ``intended`` applied"""
    with open(os.path.join(rc.ROOT, "tests", "golden", "route_census.json")) as fh:
        f = json.load(fh)
    out = {cid: g["outcome"] for g in f["outcomes"] for cid in g["cases"]}
    out.update({cid: e["outcome"] for cid, e in f["intended"].items()})
    return out


def raises(c):
    """the cases left out of the value run: those whose census outcome is a raise; of the own cases none"""
    return not c.get("own") and isinstance(census()[c["id"]], list)


def repeats(c):
    return 2 if c.get("ctx") else 1


# ---- the rules, written out -------------------------------------------------------------------------------------------------------
def jp_of(J):
    return 32 if J > 16 else 4 * ((J + 3) // 4)


def wants_grad(c):
    return c["grad"] == "required" and c["call"] != "zspectrum"


def nhwc_path(c):
    """README: mode "auto" takes the NHWC kernels wherever they apply - maps of at least 2 x 2, up to 16 joints, 17..32 without
    a heat-map gradient or, fp32 storage, with ``wide_grad``; mode "nhwc" / "planar" is the caller's word"""
    w, h = rc.hm_size(c)
    J = c["J"]
    if c["mode"] != "auto":
        return c["mode"] == "nhwc"
    wide_ok = 16 < J <= 32 and (not wants_grad(c) or ("wide_grad" in c["sw"] and c["io"] == "fp32"))
    return w >= 2 and h >= 2 and (J <= 16 or wide_ok)


def sees_rounded(c):
    """the kernel must see the bf16-rounded maps iff the tensors are bf16, or the storage is (``io``), or ``bf16_maps`` is on,
    no gradient is wanted and a bf16 kernel covers the request: 13..32 joints on the NHWC path (J = 1 in place is covered for
    bf16 TENSORS only, the first clause: a one-channel kernel reads where the values lie, and fp32 values lie unrounded).
    A z-spectrum call makes no path decision: mode "auto" / "nhwc" and a map of at least 2 x 2."""
    if c["hand"] in BF16_HANDS or c["io"] == "bf16":
        return True
    if "bf16_maps" not in c["sw"] or wants_grad(c):
        return False
    w, h = rc.hm_size(c)
    on_path = (c["mode"] in ("auto", "nhwc") and w >= 2 and h >= 2) if c["call"] == "zspectrum" else nhwc_path(c)
    return on_path and 13 <= c["J"] <= 32


def masked(c):
    """a wanted gradient comes from a pass mask (and so has a deterministic form): NHWC path, fp32 io, h, w >= 2, J <= 16 or
    17 <= J <= 32 with ``wide_grad``"""
    w, h = rc.hm_size(c)
    J = c["J"]
    return wants_grad(c) and nhwc_path(c) and c["io"] == "fp32" and w >= 2 and h >= 2 and \
        (J <= 16 or (17 <= J <= 32 and "wide_grad" in c["sw"]))


def num_cubes(c):
    return P3 if c["call"] == "sample_of" else B


def result_form(c):
    """(dtype name, shape, strides) of the result of a non-raising case: pad and channels-last act on the NHWC path up to 16
    joints, channels-last only where the channel count is a multiple of 4; ``out`` is the corner of a (X+2, Y+4, Z+8) block;
    float64 callers get float64; bf16 storage bf16"""
    P, J = num_cubes(c), c["J"]
    if c["call"] == "zspectrum":
        shape = (B, J, KZ, X // 4, Y // 4, 16)
        return "complex64", shape, _dense(shape)
    acts = nhwc_path(c) and J <= 16
    Jc = jp_of(J) if acts and c["call"] in ("pad", "pad_cl") else J
    cl = acts and c["call"] in ("cl", "pad_cl") and Jc % 4 == 0
    dtype = "float64" if c["hand"] == "f64" else ("bfloat16" if c["io"] == "bf16" else "float32")
    shape = (P, Jc, X, Y, Z)
    if cl:
        return dtype, shape, (Jc * N, 1, Y * Z * Jc, Z * Jc, Jc)
    if c["call"] == "out":
        return dtype, shape, _dense((P, J, X + 2, Y + 4, Z + 8))
    return dtype, shape, _dense(shape)


def _dense(shape):
    s, out = 1, []
    for n in reversed(shape):
        out.append(s)
        s *= n
    return tuple(reversed(out))


def same_strides(shape, a, b):
    """a dimension of size 1 carries an arbitrary stride"""
    return all(n == 1 or x == y for n, x, y in zip(shape, a, b))


def returns_grids(c):
    return c["call"] not in ("no_grids", "out", "pad_cl", "zspectrum")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _rng(c, what, call_no=0):
    return np.random.default_rng([zlib.crc32(c["id"].encode()), zlib.crc32(what.encode()), call_no])


def leaf_arrays(c, call_no=0):
    """the values of the case's leaf tensors at call ``call_no`` (host, float32 - float64 for the f64 hand-over; bf16 leaves:
    bf16-representable): V planar tensors, or ONE (V,B,h,w,jp) buffer whose pad channels are zero"""
    w, h = rc.hm_size(c)
    J, hand = c["J"], c["hand"]
    g = _rng(c, "maps", call_no)
    u = lambda *s: (g.random(s) * 1.6 - 0.3)
    if hand == "f64":
        return [u(B, J, h, w) for _ in range(V)]
    if hand in ("planar", "contiguous1"):
        return [u(B, J, h, w).astype(np.float32) for _ in range(V)]
    if hand == "expanded":
        return [u(1, 1, h, w).astype(np.float32) for _ in range(V)]
    if hand == "slice_planar":
        return [u(B, SLICE_OF, h, w).astype(np.float32) for _ in range(V)]
    if hand == "planar_bf16":
        return [bf16_round(u(B, SLICE_OF, h, w).astype(np.float32)) for _ in range(V)]
    Jn = SLICE_OF if hand.startswith("slice_nhwc") else J
    buf = u(V, B, h, w, jp_of(Jn)).astype(np.float32)
    buf[..., Jn:] = 0
    return [bf16_round(buf) if hand in BF16_HANDS else buf]


def make_leaves(c, arrays, device):
    import torch
    dt = torch.float64 if c["hand"] == "f64" else (torch.bfloat16 if c["hand"] in BF16_HANDS else torch.float32)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt).requires_grad_(c["grad"] == "required") for a in arrays]


def views_of(c, leaves):
    """the list[V] of (B,J,h,w) heat-maps handed to the layer, views of the leaves"""
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    w, h = rc.hm_size(c)
    hand = c["hand"]
    if hand in ("planar", "f64", "contiguous1"):
        return list(leaves)
    if hand == "expanded":
        return [x.expand(B, 1, h, w) for x in leaves]
    if hand in ("slice_planar", "planar_bf16"):
        return [x[:, SLICE_CH:SLICE_CH + 1] for x in leaves]
    sl = hand.startswith("slice_nhwc")
    views = nhwc_heatmap_views(leaves[0], SLICE_OF if sl else c["J"])
    return [x[:, SLICE_CH:SLICE_CH + 1] for x in views] if sl else views


def logical_maps(c, arrays):
    """list[V] of (B,J,h,w) float32: the values of the heat-maps as handed over (float64 maps cast to fp32)"""
    w, h = rc.hm_size(c)
    hand = c["hand"]
    if hand in ("planar", "f64", "contiguous1"):
        return [a.astype(np.float32) for a in arrays]
    if hand == "expanded":
        return [np.ascontiguousarray(np.broadcast_to(a, (B, 1, h, w))) for a in arrays]
    if hand in ("slice_planar", "planar_bf16"):
        return [np.ascontiguousarray(a[:, SLICE_CH:SLICE_CH + 1]) for a in arrays]
    planes = arrays[0].transpose(0, 1, 4, 2, 3)
    if hand.startswith("slice_nhwc"):
        return [np.ascontiguousarray(planes[v][:, SLICE_CH:SLICE_CH + 1]) for v in range(V)]
    return [np.ascontiguousarray(planes[v][:, :c["J"]]) for v in range(V)]


def to_leaves(c, per_view, fill=0.0):
    """(V,B,J,h,w) per-view gradients of the heat-maps -> list of arrays of the leaves' shapes (what autograd must leave in
    ``leaf.grad``): slices fill their channel, expanded leaves take the sum over B; everything else is ``fill``"""
    w, h = rc.hm_size(c)
    hand = c["hand"]
    if hand in ("planar", "f64", "contiguous1"):
        return [per_view[v].copy() for v in range(V)]
    if hand == "expanded":
        return [per_view[v].sum(axis=0, keepdims=True) for v in range(V)]
    if hand in ("slice_planar", "planar_bf16"):
        out = [np.full((B, SLICE_OF, h, w), fill, per_view.dtype) for _ in range(V)]
        for v in range(V):
            out[v][:, SLICE_CH] = per_view[v][:, 0]
        return out
    sl = hand.startswith("slice_nhwc")
    buf = np.full((V, B, h, w, jp_of(SLICE_OF if sl else c["J"])), fill, per_view.dtype)
    if sl:
        buf[..., SLICE_CH] = per_view[:, :, 0]
    else:
        buf[..., :c["J"]] = per_view.transpose(0, 1, 3, 4, 2)
    return [buf]


@functools.lru_cache(maxsize=None)
def meta():
    from selfpose3d_amd import synthetic as syn
    return syn.random_meta(B, V, list(rc.IMG), seed=META_SEED, augment=True)


def flip_tensor(c):
    import torch
    return torch.tensor([False, True]) if c["flip"] else None


def centre_argument(c):
    """``grid_center`` as the case passes it: the shared list centre, a (B,5) tensor [x, y, z, flag, score] or, for
    ``sample_of``, a (3,3) tensor"""
    import torch
    if c["centres"] == "shared":
        return [list(rc.CENTER)]
    if c["centres"] == "sample_of":
        return torch.tensor(CENTRES3)
    gc = torch.zeros(B, 5)
    gc[:, :3] = torch.tensor(CENTRES2)
    gc[:, 4] = 0.5
    if c["centres"] == "invalid1":
        gc[1, 3] = -1.0
    return gc


def geometry(c, flip=None):
    """-> (cam (P,V,64) of the gathered batch, centres (P,3), valid (P) uint8, sample_of (P))"""
    from selfpose3d_amd.camera_pack import pack_cameras
    import torch
    flip = c["flip"] if flip is None else flip
    cam = pack_cameras(meta(), B, list(rc.IMG), torch.tensor([False, True]) if flip else None).reshape(B, V, 64)
    so = np.asarray(SAMPLE_OF if c["centres"] == "sample_of" else range(B))
    centres = {"shared": (rc.CENTER,) * B, "sample_of": CENTRES3}.get(c["centres"], CENTRES2)
    valid = np.ones(len(so), np.uint8)
    if c["centres"] == "invalid1":
        valid[1] = 0
    return cam[so], np.asarray(centres, np.float32), valid, so


def loss_weights(c, call_no=0):
    """(P, Jc, 1, 1, 1) float32, bf16-representable: bf16_round(randn) * 2^k, k integer in [-6, 3]"""
    _, shape, _ = result_form(c)
    g = _rng(c, "weights", call_no)
    w = bf16_round(g.standard_normal(shape[:2]).astype(np.float32)) * np.exp2(g.integers(-6, 4, shape[:2])).astype(np.float32)
    assert np.array_equal(bf16_round(w), w) and np.all(w != 0)
    return w.reshape(shape[:2] + (1, 1, 1))


# ---- referees -------------------------------------------------------------------------------------------------------------------
def tile44(planes):
    """(..., X, Y) -> (..., X/4, Y/4, 16), by index arithmetic: element (x, y) lies in tile (x // 4, y // 4) at 4 (x % 4) + y % 4"""
    lead = planes.shape[:-2]
    out = np.empty(lead + (X // 4, Y // 4, 16), planes.dtype)
    for x in range(X):
        for y in range(Y):
            out[..., x // 4, y // 4, 4 * (x % 4) + y % 4] = planes[..., x, y]
    return out


def z_spectrum(cubes):
    """(P,J,X,Y,Z) real -> (P,J,KZ,X/4,Y/4,16) complex128: DFT along z of the rows zero-padded to SZ, bins 0..SZ//2"""
    pad = np.zeros(cubes.shape[:-1] + (SZ,), np.float64)
    pad[..., :Z] = cubes
    return tile44(np.fft.fft(pad, axis=-1)[..., :KZ].transpose(0, 1, 4, 2, 3))


def oracle_cubes(c, maps, flip=None, want_grids=True):
    """the oracle on the gathered batch -> ((P,J,X,Y,Z) fp32, (P,N,3) fp32)"""
    from oracle import oracle
    cam, centres, valid, so = geometry(c, flip)
    return oracle.unproject_fwd([m[so] for m in maps], cam, centres, valid, list(rc.SPACE), list(rc.CUBE), list(rc.IMG), want_grids=want_grids)


def oracle_grads(c, maps, weights):
    """the oracle's backward with grad_cubes = ``weights`` (P,J,1,1,1), rows added into their samples -> (V,B,J,h,w) float64"""
    from oracle import oracle
    cam, centres, valid, so = geometry(c)
    J = maps[0].shape[1]
    grad = np.ascontiguousarray(np.broadcast_to(weights[:, :J], (len(so), J, X, Y, Z)), np.float32)
    rows = np.stack(oracle.unproject_bwd([m[so] for m in maps], cam, centres, valid, grad, list(rc.SPACE), list(rc.CUBE), list(rc.IMG)))
    out = np.zeros((V, B) + rows.shape[2:], np.float64)
    np.add.at(out, (slice(None), so), rows)
    return out


def seen_maps(c, maps):
    return [bf16_round(m) for m in maps] if sees_rounded(c) else maps


def bits(values, dtype):
    """the bit pattern of ``values`` (fp32 numpy) stored as ``dtype``: int16 for bf16 (values already rounded), int32 for fp32,
    int64 for the float64 a float64 caller gets (the fp32 result widened)"""
    import torch
    v = np.ascontiguousarray(values, np.float32)
    if dtype == "bfloat16":
        return torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy()
    return v.astype(np.float64).view(np.int64) if dtype == "float64" else v.view(np.int32)


class Expected:
    """what call ``call_no`` of a case must return, from the oracle alone"""

    def __init__(self, c, call_no=0):
        self.c, self.call_no = c, call_no
        self.arrays = leaf_arrays(c, call_no)
        self.maps = seen_maps(c, logical_maps(c, self.arrays))
        self.dtype, self.shape, self.strides = result_form(c)
        self.J = c["J"]
        cam, centres, self.valid, self.so = geometry(c)
        cubes, grids = oracle_cubes(c, self.maps)
        if c["io"] == "bf16":
            cubes = bf16_round(cubes)
        self.cubes = cubes                                           # (P,J,X,Y,Z) fp32 values; channels >= J of the result are zero
        self.grids = grids if returns_grids(c) else None
        self.spectrum = z_spectrum(cubes) if c["call"] == "zspectrum" else None
        self.seen = oracle_cubes(c, [np.ones_like(m) for m in self.maps], want_grids=False)[0][:, 0] > 0      # (P,X,Y,Z)
        self.grads = None
        if wants_grad(c):
            self.weights = loss_weights(c, call_no)
            per_view = oracle_grads(c, self.maps, self.weights)
            self.ref = to_leaves(c, per_view)
            self.S = to_leaves(c, oracle_grads(c, self.maps, np.abs(self.weights)))
            self.per_view = per_view
            self.inside = [m > 0 for m in to_leaves(c, np.ones_like(per_view))]
            # samples of the LEAVES: an expanded leaf has one, which owns every cube
            expanded = c["hand"] == "expanded"
            owns = np.bincount(self.so, weights=self.valid, minlength=B) > 0
            if expanded:
                self.dead = [np.full(r.shape, not owns.any()) for r in self.ref]
            else:
                dead = np.broadcast_to((~owns).astype(np.float64).reshape(1, B, 1, 1, 1), per_view.shape)
                self.dead = [m > 0 for m in to_leaves(c, np.ascontiguousarray(dead))]
            self.T = 4 * N * (len(self.so) if expanded else int(np.bincount(self.so, minlength=B).max()))
            self.det_step = 2.0 ** (math.ceil(math.log2(float(np.abs(self.weights[:, :self.J]).max()))) - 40)
            self.masked = masked(c)
            self.leaf_dtype = "float64" if c["hand"] == "f64" else ("bfloat16" if c["hand"] in BF16_HANDS else "float32")

    def cube_bits(self):
        return bits(self.cubes, self.dtype)

    def grid_bits(self):
        return None if self.grids is None else bits(self.grids, "float64" if self.dtype == "float64" else "float32")


@functools.lru_cache(maxsize=16)
def expected(cid, call_no=0):
    return Expected(cases()[cid], call_no)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def compare_case(e, got, figures=None):
    """``got``: dict(cubes= bit pattern (P,Jc,X,Y,Z) int16 / int32 / int64, grids= bit pattern or None, spectrum= complex array,
    grads= list of float64 arrays (one per leaf), grad_dtypes= list of names, deterministic= bool, again= the grads of a second
    backward on a fresh graph or None) - only the keys the case has.  -> list of (name, text) failures; ``figures`` (a dict)
    receives every measured figure."""
    bad, fig = [], ({} if figures is None else figures)

    def fail(name, *text):
        bad.append((name, " ".join(str(t) for t in text)))

    fig["seen_share"] = float(e.seen[e.valid > 0].mean()) if e.valid.any() else 0.0
    if e.spectrum is not None:
        spec = np.asarray(got["spectrum"])
        if spec.shape != e.spectrum.shape:
            fail("spectrum:shape", spec.shape, e.spectrum.shape)
        else:
            worst = 0.0
            for p in range(spec.shape[0]):
                scale = max(1.0, float(np.abs(e.spectrum[p]).max()))
                worst = max(worst, float(np.abs(spec[p] - e.spectrum[p]).max()) / (PARITY_CAP * scale))
                if not e.valid[p] and spec[p].any():
                    fail("spectrum:invalid", "sample", p, "is invalid, its spectrum is not zero")
            fig["spectrum_err_over_bound"], fig["spectrum_max_ref"] = worst, float(np.abs(e.spectrum).max())
            if not worst <= 1.0:
                fail("spectrum:tol", "max|got - ref| is", worst, "times 3e-6 max(1, max|ref|)")
    else:
        cubes = np.asarray(got["cubes"])
        want = e.cube_bits()
        if cubes.shape != tuple(e.shape) or cubes.dtype != want.dtype:
            fail("cubes:shape", cubes.shape, cubes.dtype, "for", e.shape, want.dtype)
        else:
            diff = cubes[:, :e.J] != want
            fig["cubes_wrong"], fig["cubes_max_ref"] = int(diff.sum()), float(np.abs(e.cubes).max())
            if diff.any():
                fail("cubes:bits", int(diff.sum()), "of", diff.size, "elements differ from the referee's, the first at", tuple(np.argwhere(diff)[0]))
            if (cubes[:, e.J:] & (np.iinfo(cubes.dtype).max)).any():
                fail("cubes:pad", "channels >=", e.J, "of the padded result are not zero")
        if e.grids is not None:
            grids = got.get("grids")
            if grids is None or np.asarray(grids).shape != e.grids.shape or not np.array_equal(np.asarray(grids), e.grid_bits()):
                fail("grids:bits", "the grids differ from the referee's")
        elif got.get("grids") is not None:
            fail("grids:bits", "grids returned where none were asked for")
    if e.c["grad"] == "required" and e.spectrum is None:
        grads = got.get("grads")
        if grads is None or len(grads) != len(e.ref) or any(g is None for g in grads):
            fail("grad:missing", "a leaf has no gradient")
            return bad
        det = bool(got.get("deterministic")) and e.masked
        tag = "det" if det else ("fp32_on_det" if got.get("deterministic") else "fp32")
        worst = dict(bound=0.0, project=0.0, det=0.0)
        for i, (g, ref, S, inside, dead) in enumerate(zip(grads, e.ref, e.S, e.inside, e.dead)):
            g = np.asarray(g, np.float64)
            if g.shape != ref.shape:
                fail("grad:shape", "leaf", i, g.shape, "for", ref.shape)
                continue
            if got["grad_dtypes"][i] != e.leaf_dtype:
                fail("grad:dtype", "leaf", i, got["grad_dtypes"][i], "for", e.leaf_dtype)
            if g[~inside].any():
                fail("grad:outside_slice", "leaf", i, int((g[~inside] != 0).sum()), "non-zero elements outside the slice's channel / in pad channels")
            if g[dead].any():
                fail("grad:no_valid_cube", "leaf", i, "gradient on a sample that owns no valid cube")
            if g[ref == 0].any():
                fail("grad:zero_where_ref_zero", "leaf", i, int((g[ref == 0] != 0).sum()), "non-zero elements where the reference is zero")
            err = np.abs(g - ref)
            widen = 2.0 ** -8 * np.abs(ref) if e.leaf_dtype == "bfloat16" else 0.0      # one RNE rounding to bf16: half an ulp
            bound = (e.T + 4) * 2.0 ** -24 * S + widen
            pos = bound > 0
            worst["bound"] = max(worst["bound"], float((err[pos] / bound[pos]).max()) if pos.any() else 0.0)
            if np.any(err > bound):
                fail("grad:bound", "leaf", i, int((err > bound).sum()), "elements beyond (T + 4) 2^-24 S, worst ratio", worst["bound"])
            scale = max(1.0, float(np.abs(ref).max()))
            tol = 2e-5 * scale + widen
            worst["project"] = max(worst["project"], float((err / tol).max()))
            if np.any(err > tol):
                fail("grad:project_tol", "leaf", i, "max error", float(err.max()), "> 2e-5 *", scale)
            if det:
                dbound = 2.0 ** -22 * S + e.T * e.det_step + widen
                worst["det"] = max(worst["det"], float((err / dbound).max()))
                if np.any(err > dbound):
                    fail("grad:det_bound", "leaf", i, int((err > dbound).sum()), "elements beyond 2^-22 S + T step, worst ratio", worst["det"])
                again = got.get("again")
                if again is None or not np.array_equal(np.asarray(again[i], np.float64), g):
                    fail("grad:det_repeat", "leaf", i, "a second deterministic backward gives other bits")
        fig[tag + "_err_over_bound"], fig[tag + "_err_over_project_tol"] = worst["bound"], worst["project"]
        if det:
            fig["det_err_over_det_bound"] = worst["det"]
        fig["grad_max_ref"] = max(float(np.abs(r).max()) for r in e.ref)
    return bad
