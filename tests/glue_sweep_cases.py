"""Case tables, seeded CPU inputs, referees and restated geometry of the sweep of joint rendering and the memory-bound helper
kernels: sp3d_render_joints_fwd / _bwd (sp3d_synth.hip), sp3d_pack_heatmaps_ex (sp3d_unproject_tile.hip),
sp3d_channel_shift_act, sp3d_maxpool2x_cl, sp3d_fetch_ring, sp3d_upsample2x_scatter[_head] (sp3d_epilogue.hip) and
sp3d_fixed_to_float (sp3d_unproject_bwd.hip).  Needs no GPU: tests/test_glue_sweep_reference.py checks everything here on
the CPU, tests/test_gpu_glue_sweep.py runs the kernels.

Everything a kernel decides from its shapes is restated here (``*_geometry``), so a case NAMES the classes it is in
(``*_classes``) and the CPU test proves that each table enters every class it is there for.

Joint rendering, the error rule.  With u = 2^-24, a_p the exponent of person p's Gaussian at a pixel, e_p = exp(a_p) and
s = sum_p e_p over the np = min(count, P) people of the entry:
    T_fwd = u (sum_p e_p (4 |a_p| + 4) + (np - 1) s) + np 2^-126
(a_p is built from about four fp32 roundings, expf is a few ulp, np - 1 additions; the last term is the number format's: a
Gaussian below the smallest normal fp32 number may be flushed to zero where float64 still holds 1e-60).  Per gradient
component c of person p, with d_c = (pixel - key-point)_c and g the incoming gradient of the pixel,
    T_bwd = sum_pixels [ u (4 |a_p| + 4) + u (ceil(h w / 256) + 8) ] |g| e_p |d_c| / sigma^2  +  2^-126 sum_pixels (1 + |d_c|)
(the same per-term factor, then the accumulation: ceil(h w / 256) serial additions in a lane and the 8-level tree across the
workgroup).  The assertion is |got - ref| <= C T with the constants below.

Clip mask.  A pixel whose float64 sum lies within C_FWD T_fwd of 1, and is not exactly 1, is UNDECIDED: the fp32 sum may fall on
the other side of the clip.  The gradient check adds sum over those pixels of |g| e_p |d_c| / sigma^2 to its allowance; the
table keeps them below 0.1 % of the pixels of every case (checked on the CPU).  A sum of exactly 1 is one Gaussian at its
pixel centre next to Gaussians that are zero in both formats: both sides pass the gradient there, and it is 0 (d = 0).

The constants C_FWD, C_BWD (rendering) and C_HEAD (the head of the up-conv scatter) are the next power of two at or above
4 x the worst ratio |got - ref| / T measured on an MI355X against the float64 referees, over the whole tables
(tests/test_gpu_glue_sweep.py has the figures).  Nothing measured on a CPU enters them.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
TINY = 2.0 ** -126
EINVAL, ENULL, ERANGE, EUNSUPPORTED = -1, -2, -3, -4            # include/sp3d.h

C_FWD = 8.0                 # worst measured ratio 1.128
C_BWD = 2.0                 # 0.265, with C_FWD = 8 in the undecided set
C_HEAD = 0.5                # 0.086

UNDECIDED_CAP = 1e-3
NAN_FILL = 0x7FC17FC1               # a NaN as one fp32 word and as two bf16 halves: what every output holds before a launch


# ===========================================================================================================================
# A. joint rendering
# ===========================================================================================================================
RJ_MAXP, RJ_FWD_CAP = 16, 32        # RJ_MAXP and the forward's workgroup cap (sp3d_synth.hip:117, :208)


def render_geometry(h, w):
    """what sp3d_render_joints_fwd / _bwd derive from the image (sp3d_synth.hip:208, :161, :184-195)"""
    hw = h * w
    blocks = min((hw + 255) // 256, RJ_FWD_CAP)
    return dict(hw=hw, fwd_blocks=blocks, fwd_trips=(hw + blocks * 256 - 1) // (blocks * 256), bwd_serial=(hw + 255) // 256,
                bwd_depth=(hw + 255) // 256 + 8)


# name, N, P, J, h, w, sigma, count, placements [(kind, n, j)], backward
RENDER_CASES = [
    dict(name="5x7 one person on a centre", N=1, P=1, J=1, h=5, w=7, sigma=0.5, count=None, place=[("centre", 0, 0)]),
    dict(name="16x16 coincident pair", N=1, P=2, J=1, h=16, w=16, sigma=3.0, count=[2], place=[("coincident", 0, 0)]),
    dict(name="257x1 count 1 of 2", N=1, P=2, J=15, h=257, w=1, sigma=3.0, count=[1], place=[("centre", 0, 3)]),
    dict(name="1x257 wide sigma, count per n", N=6, P=15, J=1, h=1, w=257, sigma=20.0, count=[0, 1, 15, 16, 3, 7],
         place=[("outside_near", 2, 0), ("one_sigma", 4, 0)]),
    dict(name="19x30 every placement", N=6, P=16, J=17, h=19, w=30, sigma=3.0, count=[0, 1, 16, 40, 2, 5],
         place=[("centre", 1, 2), ("coincident", 2, 0), ("one_sigma", 3, 16), ("outside_near", 4, 5), ("outside_far", 5, 9),
                ("coincident", 4, 11), ("outside_far", 4, 1)]),
    dict(name="65x127 grid-stride, 16 people", N=1, P=16, J=1, h=65, w=127, sigma=20.0, count=None,
         place=[("one_sigma", 0, 0)]),
    dict(name="65x127 grid-stride, pairs", N=6, P=2, J=15, h=65, w=127, sigma=3.0, count=[2, 0, 1, 2, 5, 2],
         place=[("coincident", 0, 14), ("one_sigma", 3, 7), ("centre", 2, 0), ("outside_near", 4, 1), ("outside_far", 5, 2)]),
    dict(name="19x30 narrow sigma, 15 people", N=1, P=15, J=17, h=19, w=30, sigma=0.5, count=None,
         place=[("coincident", 0, 8), ("one_sigma", 0, 9)]),
    dict(name="16x16 narrow sigma, P = 1", N=6, P=1, J=17, h=16, w=16, sigma=0.5, count=[1, 0, 1, 5, 1, 1],
         place=[("centre", 0, 0), ("centre", 3, 16), ("outside_near", 4, 4)]),
    dict(name="19x30 infinite co-ordinates", N=1, P=2, J=15, h=19, w=30, sigma=3.0, count=None, backward=False,
         place=[("inf", 0, 0), ("inf", 0, 7), ("centre_beside_inf", 0, 7)]),
    dict(name="5x7 infinite co-ordinates, narrow", N=6, P=2, J=1, h=5, w=7, sigma=0.5, count=[2, 2, 1, 2, 0, 3], backward=False,
         place=[("inf", 1, 0), ("inf", 2, 0)]),
]
RENDER_PIXEL_CLASSES = ("hw<256", "hw=256", "hw=257,w=1", "hw=257,h=1", "ragged", "grid-stride")
RENDER_COUNT_CLASSES = ("count NULL", "count=0", "count=1", "count=P", "count>P")
RENDER_PLACEMENTS = ("centre", "coincident", "one_sigma", "outside_near", "outside_far", "inf")


def render_effective_count(case):
    cnt = case["count"]
    return [case["P"]] * case["N"] if cnt is None else [min(int(c), case["P"]) for c in cnt]


def render_inputs(case, index=None):
    """kps (N,P,J,2) fp32, count (N,) int32 | None, grad_out (N,J,h,w) fp32.  Rows p >= count hold NaN: the kernels must not
    read them.  Key-points are drawn a quarter pixel or more away from every pixel centre, placements then overwrite people
    0 and 1 of their (n, j)."""
    idx = RENDER_CASES.index(case) if index is None else index
    rng = np.random.default_rng(7100 + idx)
    N, P, J, h, w, sg = (case[k] for k in ("N", "P", "J", "h", "w", "sigma"))
    cell = rng.integers(0, [w, h], size=(N, P, J, 2)).astype(np.float64)
    off = rng.uniform(0.25, 0.45, size=(N, P, J, 2)) * rng.choice([-1.0, 1.0], size=(N, P, J, 2))
    kps = (cell + off).astype(np.float32)
    for kind, n, j in case["place"]:
        if kind in ("centre", "centre_beside_inf"):
            p = 1 if kind == "centre_beside_inf" else 0
            kps[n, p, j] = (w // 2, h // 3)
        elif kind == "coincident":
            kps[n, 1, j] = kps[n, 0, j]
        elif kind == "one_sigma":
            along = 0 if w > 1 else 1
            kps[n, 0, j] = (np.float32(w / 2 - sg / 2 + 0.3), np.float32(h / 2 + 0.3)) if along == 0 else \
                (np.float32(0.3), np.float32(h / 2 - sg / 2 + 0.3))
            kps[n, 1, j] = kps[n, 0, j]
            kps[n, 1, j, along] += np.float32(sg)
        elif kind == "outside_near":
            kps[n, 0, j, 0 if w > 1 else 1] = np.float32(-2.0 * sg)
        elif kind == "outside_far":
            kps[n, 0, j] = (np.float32(w + 1e4), np.float32(-1e4))
        elif kind == "inf":
            kps[n, 0, j] = (np.float32(np.inf), np.float32(h / 2 + 0.3)) if (n + j) % 2 == 0 else \
                (np.float32(w / 2 + 0.3), np.float32(-np.inf))
        else:
            raise KeyError(kind)
    count = None if case["count"] is None else np.asarray(case["count"], np.int32)
    for n, c in enumerate(render_effective_count(case)):
        kps[n, c:] = np.nan
    gout = rng.standard_normal((N, J, h, w)).astype(np.float32)
    return torch.from_numpy(kps), None if count is None else torch.from_numpy(count), torch.from_numpy(gout)


def render_classes(case, kps=None):
    """the classes a case is in, read off its shapes, counts and the key-points themselves"""
    if kps is None:
        kps = render_inputs(case)[0]
    k = kps.numpy().astype(np.float64)
    N, P, J, h, w, sg = (case[q] for q in ("N", "P", "J", "h", "w", "sigma"))
    g = render_geometry(h, w)
    out = {"P=%d" % P, "J=%d" % J, "N=%d" % N, "sigma=%g" % sg}
    if g["hw"] < 256:
        out.add("hw<256")
    if g["hw"] == 256:
        out.add("hw=256")
    if g["hw"] == 257:
        out.add("hw=257,w=1" if w == 1 else "hw=257,h=1" if h == 1 else "hw=257")
    if g["hw"] % 256 and g["hw"] > 257 and g["fwd_trips"] == 1:
        out.add("ragged")
    if g["hw"] > RJ_FWD_CAP * 256 and g["fwd_trips"] > 1:
        out.add("grid-stride")
    if case["count"] is None:
        out.add("count NULL")
    else:
        for c in case["count"]:
            out.add("count=0" if c == 0 else "count=1" if c == 1 else "count=P" if c == P else "count>P" if c > P else "count other")
        if N > 1 and len(set(case["count"])) > 1:
            out.add("count differs per n")
    for n, c in enumerate(render_effective_count(case)):
        kk = k[n, :c]                                              # (c, J, 2)
        if c == 0:
            continue
        fin = np.isfinite(kk).all(-1)
        if (~fin).any():
            out.add("inf")
        on = fin & (kk == np.round(kk)).all(-1) & (kk[..., 0] >= 0) & (kk[..., 0] < w) & (kk[..., 1] >= 0) & (kk[..., 1] < h)
        if on.any():
            out.add("centre")
        kf = np.where(np.isfinite(kk), kk, 0.0)
        dist = np.maximum(np.maximum(-kf[..., 0], kf[..., 0] - (w - 1)), np.maximum(-kf[..., 1], kf[..., 1] - (h - 1)))
        if (fin & (dist > 0) & (dist < 3 * sg)).any():
            out.add("outside_near")
        if (fin & (dist >= 1e4)).any():
            out.add("outside_far")
        for p in range(c):
            for q in range(p + 1, c):
                ok = fin[p] & fin[q]
                d = np.hypot(*(kf[p] - kf[q]).T)
                if (ok & (d == 0)).any():
                    out.add("coincident")
                if (ok & (np.abs(d - sg) <= 1e-5 * sg)).any():
                    out.add("one_sigma")
    return out


def render_referee(kps, count, h, w, sigma, gout=None):
    """the float64 torch graph of multi_person_posenet_ssv.py:409-465 on the fp32 key-points widened to float64 ->
    dict(out (N,J,h,w), s: the unclipped sum, T_fwd; with ``gout``: grad (N,P,J,2) by autograd of (out * gout).sum(), and
    the pieces of T_bwd that tests build the allowance from)"""
    k = kps.double().clone().requires_grad_(gout is not None)
    N, P, J = (int(v) for v in k.shape[:3])
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    sums, scales = [], []
    nps = [P] * N if count is None else [min(int(c), P) for c in count]
    for n in range(N):
        kn = k[n, :nps[n]]                                          # rows p >= count are never touched
        a = -((xx - kn[..., 0, None, None]) / sigma) ** 2 / 2 - ((yy - kn[..., 1, None, None]) / sigma) ** 2 / 2   # (np,J,h,w)
        e = torch.exp(a)
        s = e.sum(0) if nps[n] else torch.zeros((J, h, w), dtype=torch.float64)
        sums.append(s)
        with torch.no_grad():
            per = torch.where(e > 0, e * (4 * a.abs() + 4), torch.zeros_like(e))          # exp(-inf) = 0 contributes nothing
            t = U24 * (per.sum(0) + max(nps[n] - 1, 0) * s) + nps[n] * TINY if nps[n] else torch.zeros_like(s)
        scales.append(t)
    s = torch.stack(sums)
    out = torch.clip(s, 0.0, 1.0)
    ref = dict(out=out.detach(), s=s.detach(), T_fwd=torch.stack(scales), np=nps)
    if gout is not None:
        (out * gout.double()).sum().backward()
        ref["grad"] = k.grad.detach()
    return ref


def render_undecided(ref, c_fwd=None):
    """(N,J,h,w) bool: the float64 sum is within C_FWD T_fwd of 1 without being 1"""
    c = C_FWD if c_fwd is None else c_fwd
    return ((ref["s"] - 1.0).abs() <= c * ref["T_fwd"]) & (ref["s"] != 1.0)


def render_bwd_scales(case, kps, gout, ref, c_fwd=None):
    """T_bwd and the undecided-pixel allowance, both (N,P,J,2) float64; rows p >= count are 0 (exact zeros are demanded)"""
    N, P, J, h, w, sg = (case[q] for q in ("N", "P", "J", "h", "w", "sigma"))
    depth = render_geometry(h, w)["bwd_depth"]
    k = kps.double()
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    und = render_undecided(ref, c_fwd)
    T = torch.zeros((N, P, J, 2), dtype=torch.float64)
    A = torch.zeros((N, P, J, 2), dtype=torch.float64)
    g = gout.double().abs()
    for n in range(N):
        c = ref["np"][n]
        if not c:
            continue
        kn = k[n, :c]
        dx, dy = xx - kn[..., 0, None, None], yy - kn[..., 1, None, None]                       # (c,J,h,w)
        a = -(dx / sg) ** 2 / 2 - (dy / sg) ** 2 / 2
        e = torch.exp(a)
        passed = (ref["s"][n] <= 1.0) | und[n]                      # where a contribution can exist at all
        for comp, d in enumerate((dx, dy)):
            term = g[n] * e * d.abs() / sg ** 2
            T[n, :c, :, comp] = (U24 * (4 * a.abs() + 4 + depth) * term * passed).sum((-1, -2)) + TINY * (1 + d.abs()).sum((-1, -2))
            A[n, :c, :, comp] = (term * und[n]).sum((-1, -2))
    return T, A


def render_naive(kps, count, h, w, sigma, gout):
    """the same maps and gradients by plain loops (math.exp, one pixel and one person at a time); ``gout`` None: maps only"""
    k = kps.numpy().astype(np.float64)
    N, P, J = k.shape[:3]
    out = np.zeros((N, J, h, w))
    grad = np.zeros((N, P, J, 2))
    go = None if gout is None else gout.numpy().astype(np.float64)
    for n in range(N):
        c = P if count is None else min(int(count[n]), P)
        for j in range(J):
            for y in range(h):
                for x in range(w):
                    es = [math.exp(-((x - k[n, p, j, 0]) / sigma) ** 2 / 2 - ((y - k[n, p, j, 1]) / sigma) ** 2 / 2) for p in range(c)]
                    s = sum(es)
                    out[n, j, y, x] = min(max(s, 0.0), 1.0)
                    if go is not None and s <= 1.0:
                        for p in range(c):
                            grad[n, p, j, 0] += go[n, j, y, x] * es[p] * (x - k[n, p, j, 0]) / sigma ** 2
                            grad[n, p, j, 1] += go[n, j, y, x] * es[p] * (y - k[n, p, j, 1]) / sigma ** 2
    return out, grad


# ===========================================================================================================================
# B. heat-map packing
# ===========================================================================================================================
PACK_ROWS = [(4, 0, 0), (8, 0, 0), (12, 0, 0), (16, 0, 0), (32, 0, 0), (16, 1, 1), (16, 1, 0), (16, 0, 1), (32, 1, 1), (32, 1, 0),
             (32, 0, 1)]            # (Jp, in_bf16, out_bf16): the 11 rows of find_pack_kernel (sp3d_unproject_tile.hip:319-326)
PACK_IMAGES = [(1, 1), (15, 17), (16, 16), (257, 1), (24, 32), (33, 65)]       # h*w = 1, 255, 256, 257, 3*256, ragged 2145
PACK_SPECIALS = [0x00000000, 0x80000000, 0x00000001, 0x80400000, 0x7F800000, 0xFF800000, 0x3F808000, 0x3F818000, 0x7F7FFFFF,
                 0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0xFFFFFFFF]
PACK_NANS = PACK_SPECIALS[9:]


def pack_geometry(h, w):
    hw = h * w
    return dict(hw=hw, blocks=(hw + 255) // 256, tail=hw % 256)


def pack_row_name(row):
    return "Jp%d %s->%s" % (row[0], "bf16" if row[1] else "fp32", "bf16" if row[2] else "fp32")


def pack_cases(row):
    """six cases per row, one per image size; J, B and V rotate so that every row sees J in {1, Jp-1, Jp} (and 17 at Jp = 32),
    B in {1, 3} and V in {1, 16}; the 256-pixel case of every row reads its views one element into a larger tensor"""
    Jp, ib, ob = row
    js = [1, Jp - 1, Jp] + ([17] if Jp == 32 else [])
    r = PACK_ROWS.index(row)
    out = []
    for i, (h, w) in enumerate(PACK_IMAGES):
        B = (1, 3)[(i + r) % 2]
        V = 16 if i in (1, 4) else 1
        out.append(dict(Jp=Jp, in_bf16=ib, out_bf16=ob, J=js[(i + r) % len(js)], h=h, w=w, B=B, V=V, offset=(h * w == 256)))
    if Jp == 32:                                                    # four values of J, six images: name the fourth explicitly
        out.append(dict(Jp=Jp, in_bf16=ib, out_bf16=ob, J=17, h=15, w=17, B=3, V=1, offset=False))
        out.append(dict(Jp=Jp, in_bf16=ib, out_bf16=ob, J=31, h=1, w=1, B=1, V=16, offset=False))
    return out


def pack_inputs(case, seed=0):
    """list[V] of (B,J,h,w) CPU tensors in the input storage type.  fp32 values have a wide exponent spread (every rounding
    case of the conversion turns up); rows with bf16 on either side carry PACK_SPECIALS at fixed flat positions of every view"""
    rng = np.random.default_rng(8200 + seed + 131 * case["Jp"] + 17 * case["J"] + case["h"] * case["w"])
    shape = (case["B"], case["J"], case["h"], case["w"])
    views = []
    for v in range(case["V"]):
        x = (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 20, size=shape))).astype(np.float32)
        if case["in_bf16"] or case["out_bf16"]:
            flat = x.reshape(-1).view(np.uint32)
            for i, bits in enumerate(PACK_SPECIALS):
                flat[(3 + 5 * i + v) % flat.size] = bits
        t = torch.from_numpy(x)
        views.append(t.to(torch.bfloat16) if case["in_bf16"] else t)
    return views


def pack_referee(views, Jp, out_bf16):
    """permute(0, 2, 3, 1) with zero pad channels, torch's storage conversion -> (V,B,h,w,Jp)"""
    B, J, h, w = views[0].shape
    out = torch.zeros((len(views), B, h, w, Jp), dtype=torch.float32)
    for v, x in enumerate(views):
        out[v, ..., :J] = x.float().permute(0, 2, 3, 1)
    return out.to(torch.bfloat16) if out_bf16 else out


def pack_naive(views, Jp, out_bf16):
    """the same by loops; the fp32 -> bf16 rounding spelled out on the bits (nearest even, NaN kept)"""
    B, J, h, w = views[0].shape
    xs = [x.float().numpy().view(np.uint32) for x in views]
    out = np.zeros((len(views), B, h, w, Jp), np.uint32)
    for v in range(len(views)):
        for b in range(B):
            for j in range(J):
                for y in range(h):
                    for x in range(w):
                        out[v, b, y, x, j] = xs[v][b, j, y, x]
    if not out_bf16:
        return out
    u = out.astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def bits_of(t):
    """integer view of a CPU tensor's storage (fp32 -> int32, bf16 -> int16)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits_nan_free(got, ref):
    """bit for bit where the referee is a number, NaN (any payload) where it is NaN"""
    rn = torch.isnan(ref)
    return bool((torch.isnan(got) == rn).all()) and bool((bits_of(got)[~rn] == bits_of(ref)[~rn]).all())


# ===========================================================================================================================
# C. channel shift + activation
# ===========================================================================================================================
CSA_CAP = 8192                      # workgroups x 256 lanes x 4 elements = 8 388 608 elements per trip (sp3d_epilogue.hip:63)
# (batch, C, inner, channels_last): the memory is (batch, C, inner) planar or (batch, inner, C) channels-last
CSA_SHAPES = [
    (2, 8, 4, 0),                   # planar, inner = 4: the channel changes every vector
    (3, 1, 8, 0),                   # planar, C = 1
    (2, 5, 36, 0),                  # planar, odd C, n4 = 90 < 256
    (1, 3, 1028, 0),                # planar, 771 vectors: four workgroups, the last one ragged
    (2, 4, 3, 1),                   # channels-last C = 4, n4 = 6
    (1, 12, 45, 1),                 # channels-last C = 12: the vector's channel walks 0, 4, 8
    (3, 64, 7, 1),                  # channels-last C = 64
    (1, 12, 171, 1),                # channels-last, 513 vectors
]
CSA_LARGE = (1, 8, 128 * 128 * 65)  # 8 519 680 elements: a second, ragged trip of the grid-stride loop; both layouts
CSA_LARGE_MODES = {0: 2, 1: 3}      # layout -> the mode the large case runs


def csa_geometry(batch, C, inner):
    n4 = batch * C * inner // 4
    blocks = min((n4 + 255) // 256, CSA_CAP)
    return dict(n=batch * C * inner, n4=n4, blocks=blocks, trips=(n4 + blocks * 256 - 1) // (blocks * 256),
                last_trip=n4 - (n4 - 1) // (blocks * 256) * (blocks * 256))


def csa_refusal(C, inner, channels_last):
    return EUNSUPPORTED if ((C & 3) if channels_last else (inner & 3)) else 0


def csa_classes(shape):
    batch, C, inner, cl = shape
    g = csa_geometry(batch, C, inner)
    out = {"channels-last" if cl else "planar"}
    if not cl and inner == 4:
        out.add("planar inner=4")
    if not cl and C == 1:
        out.add("planar C=1")
    if cl:
        out.add("channels-last C=%d" % C)
    if g["n4"] < 256:
        out.add("n4<256")
    if g["blocks"] > 1 and g["n4"] % 256:
        out.add("ragged last workgroup")
    if g["trips"] > 1:
        out.add("second trip, partial" if g["last_trip"] < g["blocks"] * 256 else "second trip")
    return out


def csa_inputs(shape, seed, nan=False):
    """y, shift, residual as the kernel's memory sees them: y and residual (batch, C, inner) or (batch, inner, C), shift (C).
    ``nan``: NaN at a few fixed elements of y, and +-inf"""
    batch, C, inner, cl = shape
    g = torch.Generator().manual_seed(8300 + seed)
    mem = (batch, inner, C) if cl else (batch, C, inner)
    y = torch.randn(mem, generator=g)
    res = torch.randn(mem, generator=g)
    shift = torch.randn(C, generator=g)
    if nan:
        f = y.view(-1)
        n = f.numel()
        f[torch.tensor([0, n // 3, n - 1])] = float("nan")
        f[n // 2] = float("inf")
        f[n // 2 - 1] = float("-inf")
    return y, shift, res


def csa_referee(y, shift, res, mode, cl):
    """torch fp32 on the CPU in the kernel's order: y + shift, + res (2), ReLU as fmaxf(., 0) (1-3), + res (3)"""
    t = y + (shift.view(1, 1, -1) if cl else shift.view(1, -1, 1))
    if mode == 2:
        t = t + res
    if mode >= 1:
        t = torch.fmax(t, torch.zeros((), dtype=t.dtype))           # fmaxf: NaN -> 0
    if mode == 3:
        t = t + res
    return t


def csa_naive(y, shift, res, mode, cl):
    yn, rn, sn = y.numpy(), res.numpy(), shift.numpy()
    out = np.empty_like(yn)
    zero = np.float32(0.0)
    for i in np.ndindex(*yn.shape):
        c = i[2] if cl else i[1]
        t = np.float32(yn[i] + sn[c])
        if mode == 2:
            t = np.float32(t + rn[i])
        if mode >= 1:
            t = zero if (t != t or t < zero) else t
        if mode == 3:
            t = np.float32(t + rn[i])
        out[i] = t
    return torch.from_numpy(out)


# ===========================================================================================================================
# D. 2x max-pool, channels-last
# ===========================================================================================================================
# (B, X, Y, Z, C).  The workgroup cap of the launch (65535 * 16 workgroups of 256 lanes, sp3d_epilogue.hip:336) needs
# B * X/2 * Y/2 * Z/2 * C/4 > 268 million lanes - an input of 34 GB: it cannot be reached at testable sizes and is not tested.
POOL_SHAPES = [(1, 2, 2, 2, 4), (3, 6, 10, 2, 12), (1, 10, 2, 6, 32), (3, 2, 6, 10, 128), (1, 6, 6, 6, 4), (3, 10, 10, 10, 32)]
POOL_FAMILIES = ["random", "ties", "neg_inf"] + ["nan_at_%d" % t for t in range(8)] + ["all_nan"]
POOL_CAP_LANES = 65535 * 16 * 256


def pool_geometry(B, X, Y, Z, C):
    n = B * (X // 2) * (Y // 2) * (Z // 2) * (C // 4)
    return dict(lanes=n, blocks=min((n + 255) // 256, 65535 * 16), capped=n > POOL_CAP_LANES)


def pool_refusal(B, X, Y, Z, C):
    if B <= 0 or X <= 1 or Y <= 1 or Z <= 1 or C <= 0:
        return EINVAL
    return EUNSUPPORTED if (C & 3) or (X & 1) or (Y & 1) or (Z & 1) else 0


def pool_inputs(shape, family, seed=0):
    """x as the kernel's memory sees it, (B, X, Y, Z, C) fp32.  Window position t = 4 dx + 2 dy + dz as the kernel walks it
    (t = 0 seeds its maximum).  The special families touch every third window (all channels alternate), the rest is random."""
    B, X, Y, Z, C = shape
    g = torch.Generator().manual_seed(8400 + seed + POOL_SHAPES.index(shape) * 31 + POOL_FAMILIES.index(family))
    x = torch.randn(shape, generator=g)
    if family == "random":
        return x
    if family == "ties":
        return torch.randint(-2, 3, shape, generator=g).float() + 0.5          # five values, none of them +-0
    win = x.view(B, X // 2, 2, Y // 2, 2, Z // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(-1, 8).clone()   # (windows, t)
    pick = torch.arange(win.shape[0]) % 3 == 0
    if family == "neg_inf":
        win[pick] = float("-inf")
    elif family == "all_nan":
        win[pick] = float("nan")
    else:
        win[pick, int(family[-1])] = float("nan")
    return win.view(B, X // 2, Y // 2, Z // 2, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(shape).contiguous()


def pool_referee(x):
    return F.max_pool3d(x.permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1).contiguous()


def pool_naive(x):
    xn = x.numpy()
    B, X, Y, Z, C = xn.shape
    out = np.empty((B, X // 2, Y // 2, Z // 2, C), np.float32)
    for i in np.ndindex(*out.shape):
        b, xo, yo, zo, c = i
        w = xn[b, 2 * xo:2 * xo + 2, 2 * yo:2 * yo + 2, 2 * zo:2 * zo + 2, c].reshape(-1)
        out[i] = np.float32(np.nan) if np.isnan(w).any() else w.max()
    return torch.from_numpy(out)


# ===========================================================================================================================
# E. fixed point -> float
# ===========================================================================================================================
FIX_NS = [1, 255, 256, 257, 100003]
FIX_SCALES = [2.0 ** -10, 1.0, 2.0 ** 40]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
FIX_SPECIALS = [0, 1, -1, 2 ** 53 + 1, -(2 ** 53 + 1), INT64_MIN, INT64_MAX]


def fix_halfway(count, seed):
    """integers (2 M + 1) 2^e, 2^23 <= M < 2^24: exactly halfway between two neighbouring floats, and still so after the
    division by a power of two; every other one negative.  Then the same +-1 at e >= 30 (no longer halfway: the double sees it)"""
    rng = np.random.default_rng(8500 + seed)
    M = rng.integers(2 ** 23, 2 ** 24, size=count, dtype=np.int64)
    e = rng.integers(0, 38, size=count, dtype=np.int64)
    v = (2 * M + 1) << e
    v[1::2] *= -1
    near = v[e >= 30]
    return np.concatenate([v, near + 1, near - 1])


def fix_inputs(n, seed):
    """int64 accumulators: the specials and 24 halfway integers first (rotated by the seed, so n = 1 meets another value in every
    case), then random integers of every magnitude"""
    rng = np.random.default_rng(8600 + seed)
    head = np.concatenate([np.asarray(FIX_SPECIALS, np.int64), fix_halfway(24, seed)])
    head = np.roll(head, -seed)
    body = rng.integers(INT64_MIN, INT64_MAX, size=max(n, 1), dtype=np.int64, endpoint=True) >> rng.integers(0, 63, size=max(n, 1))
    return np.concatenate([head, body])[:n].copy()


def fix_geometry(n):
    return dict(blocks=(n + 255) // 256, tail=n % 256)


def fix_referee(acc, scale):
    return (acc.astype(np.float64) / np.float64(np.float32(scale))).astype(np.float32)


def fix_naive(acc, scale):
    from fractions import Fraction
    out = np.empty(len(acc), np.float32)
    for i, a in enumerate(acc.tolist()):
        d = float(a)                                                # int -> double, round to nearest even (Python rounds correctly)
        q = float(Fraction(d) / Fraction(float(np.float32(scale))))  # double division, correctly rounded
        out[i] = np.float32(q)
    return out


# ===========================================================================================================================
# F. fetch ring
# ===========================================================================================================================
# (n, R, dst offset in floats): the vector path needs n % 4 == 0 and 16-byte aligned slot and dst (sp3d_epilogue.hip:218)
RING_CASES = [(4, 1, 0), (4, 3, 0), (4096, 3, 0), (4100, 1, 0), (4100, 3, 0), (1, 3, 0), (1283, 1, 0), (1283, 3, 0), (1280, 3, 1)]
RING_WRAP = 2 ** 32 - 1


def ring_geometry(n, dst_offset):
    vector = n % 4 == 0 and dst_offset % 4 == 0                     # ring and result buffers are 16-byte aligned themselves
    n4 = n // 4
    return dict(path="vector" if vector else "scalar", trips=(n4 + 1023) // 1024 if vector else (n + 255) // 256,
                idle_last=vector and n4 > 1024 and (n4 % 1024) < 256)


def ring_classes(case):
    n, R, off = case
    g = ring_geometry(n, off)
    out = {g["path"], "R=%d" % R}
    if g["path"] == "vector":
        out.add("fewer than 256 vectors" if n // 4 < 256 else "one full trip" if n == 4096 else "second trip, almost idle" if g["idle_last"] else "other")
    else:
        out.add("n=1" if n == 1 else "n%4!=0" if n % 4 else "dst misaligned")
    return out


def ring_data(n, R, seed):
    """(R, n) int32: random bits (a copy must keep every one of them, NaN payloads included), slot r tagged in word 0"""
    rng = np.random.default_rng(8700 + seed)
    d = rng.integers(-2 ** 31, 2 ** 31, size=(R, n), dtype=np.int64).astype(np.int32)
    d[:, 0] = np.arange(R) + 1000
    return d


def ring_expected(R, start, launches):
    """[(slot read, counter afterwards)] of consecutive launches from ``start`` (uint32 arithmetic)"""
    return [(((start + t) % 2 ** 32) % R, (start + t + 1) % 2 ** 32) for t in range(launches)]


# ===========================================================================================================================
# G. up-conv scatter and scatter + head
# ===========================================================================================================================
UP_CAP = 16384                      # workgroups of 256 lanes per trip (sp3d_epilogue.hip:173, :188)
# (batch, (X, Y, Z), O, J): J = 0 is the plain scatter
UP_CASES = [
    (2, (3, 4, 5), 4, 0), (2, (3, 4, 5), 64, 0), (2, (3, 4, 5), 32, 1), (2, (3, 4, 5), 32, 9),
    (1, (9, 11, 331), 64, 0),       # 32 769 input voxels: 4 194 432 lanes, 128 beyond one trip; a 67 MB result
    (1, (1, 65537, 1), 32, 15),     # 65 537 input voxels: 4 194 368 lanes
]


def up_geometry(batch, size, O, J):
    n_in = batch * size[0] * size[1] * size[2]
    total = n_in * 8 * (8 if J else O // 4)
    blocks = min((total + 255) // 256, UP_CAP)
    return dict(n_in=n_in, total=total, blocks=blocks, trips=(total + blocks * 256 - 1) // (blocks * 256),
                second_trip_lanes=max(0, total - blocks * 256))


def up_classes(case):
    g = up_geometry(*case)
    out = {"head J=%d" % case[3] if case[3] else "scatter O=%d" % case[2]}
    out.add("second trip" if g["trips"] == 2 else "one trip" if g["trips"] == 1 else "more trips")
    if g["total"] % 256:
        out.add("ragged")
    if case[3] and case[3] > 8:
        out.add("second head group")
    return out


def up_inputs(case, seed):
    batch, (X, Y, Z), O, J = case
    g = torch.Generator().manual_seed(8800 + seed)
    n_in = batch * X * Y * Z
    G = torch.randn((n_in, 8 * O), generator=g)
    shift = torch.randn(O, generator=g)
    skip = torch.randn((batch, 2 * X, 2 * Y, 2 * Z, O), generator=g)
    w = torch.randn((max(J, 1), O), generator=g) / math.sqrt(O)
    b = torch.randn(max(J, 1), generator=g)
    return G, shift, skip, w, b


def up_place(G, batch, size, O):
    """G (n_in, (i, j, k, o)) -> (batch, 2X, 2Y, 2Z, O) by index arithmetic alone"""
    X, Y, Z = size
    return G.view(batch, X, Y, Z, 2, 2, 2, O).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(batch, 2 * X, 2 * Y, 2 * Z, O)


def up_scatter_referee(G, shift, skip, batch, size, O):
    """fp32, bit for bit: relu(G + shift) + skip"""
    return torch.relu(up_place(G, batch, size, O) + shift) + skip


def up_head_referee(G, shift, skip, w, b, batch, size, O):
    """float64 head and its scale 33 u (|b| + sum_o |w| |v|): 32 fmas and the shuffle tree"""
    v = torch.relu(up_place(G, batch, size, O).double() + shift.double()) + skip.double()
    head = v @ w.double().t() + b.double()
    scale = 33 * U24 * (v.abs() @ w.double().abs().t() + b.double().abs())
    return head, scale


def up_naive(G, shift, skip, w, b, batch, size, O, J):
    """loops over the input voxels; the plain scatter in fp32 (its referee is exact), the head in float64"""
    dt = np.float64 if J else np.float32
    Gn, sn, kn, wn, bn = (t.numpy().astype(dt) for t in (G, shift, skip, w, b))
    X, Y, Z = size
    out = np.zeros((batch, 2 * X, 2 * Y, 2 * Z, O), dt)
    for bb in range(batch):
        for x in range(X):
            for y in range(Y):
                for z in range(Z):
                    n = ((bb * X + x) * Y + y) * Z + z
                    for ijk in range(8):
                        i, j, k = ijk >> 2, (ijk >> 1) & 1, ijk & 1
                        row = Gn[n, ijk * O:(ijk + 1) * O] + sn
                        out[bb, 2 * x + i, 2 * y + j, 2 * z + k] = np.maximum(row, dt(0)) + kn[bb, 2 * x + i, 2 * y + j, 2 * z + k]
    if not J:
        return out
    return np.einsum("bxyzo,jo->bxyzj", out, wn) + bn


def power_of_two_at_or_above(x):
    return 2.0 ** math.ceil(math.log2(x)) if x > 0 else 2.0 ** -10


@functools.lru_cache(maxsize=None)
def render_problem(index):
    """inputs and referee of one rendering case, computed once and shared (nothing modifies them)"""
    case = RENDER_CASES[index]
    kps, count, gout = render_inputs(case, index)
    backward = case.get("backward", True)
    ref = render_referee(kps, count, case["h"], case["w"], case["sigma"], gout if backward else None)
    return case, kps, count, gout, ref
