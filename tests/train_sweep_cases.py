"""Case tables, seeded inputs, float64 referees and geometry helpers of the training-step sweep: grouped BatchNorm
(selfpose3d_amd/csrc/sp3d_gbn.hip) and the rendering kernels of the self-supervised losses (sp3d_synth.hip).  Needs no GPU:
tests/test_train_sweep_reference.py checks everything here on the CPU, tests/test_gpu_train_sweep.py runs the kernels.

Everything a kernel decides from its shapes is restated here (``gbn_geometry``), so a case NAMES the classes it is in
(``gbn_classes``) and the CPU test proves that the table enters each of them."""
import math

import numpy as np
import torch

F32, F64 = 0, 1                     # SP3D_GBN_F32 / SP3D_GBN_F64
EINVAL, EUNSUPPORTED = -1, -4       # include/sp3d.h
EPS = 1e-5
U24, U23 = 2.0 ** -24, 2.0 ** -23
TPB, REPLICAS, GB = 256, 16, 8      # GBN_TPB, SP3D_GBN_REPLICAS, GBN_GB


# ---- geometry of sp3d_gbn.hip ---------------------------------------------------------------------------------------------
def gbn_geometry(dtype, C, N, S):
    """what sp3d_gbn_forward / _backward derive from (dtype, C, N, S): GbnMap (sp3d_gbn.hip:50-62), gbn_rows (:413-420) and
    the grid lines (:452-460)"""
    W = 4 if dtype == F32 else 2
    CV = C // W
    cpp = min(CV, TPB)
    RP = TPB // cpp
    rows = (N * S + 2047) // 2048
    rows = (rows + RP * 8 - 1) // (RP * 8) * (RP * 8)
    rows = max(rows, RP * 8)
    chunks = (S + rows - 1) // rows
    ab_free = (S * CV + TPB * 4 - 1) // (TPB * 4)
    cap = (4096 + N - 1) // N
    return dict(W=W, CV=CV, RP=RP, rows=rows, rows_min=RP * 8, chunks=chunks, ab=max(1, min(ab_free, cap)), ab_free=ab_free,
                cap=cap, idle_threads=TPB - RP * cpp, passes=(CV + TPB - 1) // TPB, fin_blocks=(C + 15) // 16)


def gbn_refusal(dtype, C):
    """gbn_check (sp3d_gbn.hip:403-410): the answer for a width, 0 = served"""
    W = 4 if dtype == F32 else 2
    return EUNSUPPORTED if C % W or C // W > 2 * TPB else 0


def gbn_classes(case):
    """the names of the row, group and state classes a case is in"""
    g = gbn_geometry(case["dtype"], case["C"], case["N"], case["S"])
    S, G, sizes = case["S"], case["G"], case["sizes"]
    out = set()
    if S == 1:
        out.add("S=1")
    if S < g["RP"]:
        out.add("S<RP")
    if S == g["rows"]:
        out.add("S=rows")
    if S == g["rows"] + 1:
        out.add("S=rows+1")
    if S == 2 * g["rows"] - 1:
        out.add("S=2rows-1")
    if g["chunks"] >= 18:
        out.add("replicas wrap")
    if g["rows"] > g["rows_min"]:
        out.add("rows>min")
    if g["ab_free"] > g["cap"]:
        out.add("apply cap binds")
    if g["idle_threads"]:
        out.add("idle threads")
    if case["C"] % 16:
        out.add("C%16!=0")
    if g["passes"] == 2:
        out.add("second column pass")
    out.add("G=%d" % G)
    if G > GB:
        out.add("second replica fetch")
    if G > 2 * GB:
        out.add("third replica fetch")
    go = case["group_of"]
    if any(a > b for a, b in zip(go, go[1:])):
        out.add("interleaved")
    if len({s for s in sizes if s}) > 1:
        out.add("ragged")
    if any(s == 0 and any(sizes[:i]) and any(sizes[i + 1:]) for i, s in enumerate(sizes)):
        out.add("empty group in the middle")
    if any(s * S == 1 for s in sizes):
        out.add("one value")
    out.add("G_update=" + ("0" if case["G_update"] == 0 else "G" if case["G_update"] == G else "G-1"
                           if case["G_update"] == G - 1 else "other"))
    if not case["affine"]:
        out.add("no affine")
    if not case["running"]:
        out.add("no running")
    out.add("momentum=%g" % case["momentum"])
    return out


# ---- the grouped BatchNorm table ------------------------------------------------------------------------------------------
COLUMNS = [(F32, 4), (F32, 20), (F32, 32), (F32, 48), (F32, 1024), (F32, 1028), (F32, 1536), (F32, 2048),
           (F64, 2), (F64, 6), (F64, 32), (F64, 512), (F64, 514), (F64, 1024)]
REFUSED = [(F32, 2052), (F64, 1026), (F32, 6), (F64, 7), (F64, 1)]
FAMILIES = ("normal", "offset100", "offset1000", "scaled", "constant", "zero-pad")
LARGE = dict(dtype=F32, C=1024, N=2, S=8300)
GROUP_COLUMNS = [(F32, 32), (F32, 2048), (F64, 2), (F64, 32), (F64, 1024)]        # these carry the group classes


def column_name(dtype, C):
    return ("f32" if dtype == F32 else "f64") + "-C%d" % C


def _case(dtype, C, S, group_of, G=None, G_update=None, mode=0, family="normal", affine=True, running=True, momentum=0.1,
          seed=0):
    G = max(group_of) + 1 if G is None else G
    sizes = [list(group_of).count(g) for g in range(G)]
    return dict(dtype=dtype, C=C, N=len(group_of), S=S, group_of=list(group_of), G=G, sizes=sizes,
                G_update=G if G_update is None else G_update, mode=mode, family=family, affine=affine, running=running,
                momentum=momentum, seed=seed)


def _shuffled(N, G, seed):
    go = [n % G for n in range(N)]
    np.random.default_rng(seed).shuffle(go)
    return go


def gbn_cases(dtype, C):
    """the cases of one column class: its row classes, its modes and families; the group classes ride on GROUP_COLUMNS (C = 32 and
    the widest class of both types, the narrowest in float64)"""
    geo = gbn_geometry(dtype, C, 4, 1)
    RP, rmin = geo["RP"], geo["rows_min"]
    out = []
    # row classes on N = 4, groups [0, 1, 0, 0] (interleaved; group 1 of S = 1 holds ONE value), modes in turn
    row_S = [1, rmin, rmin + 1, 2 * rmin - 1] + ([3] if RP > 3 else [])
    for i, S in enumerate(row_S):
        out.append(_case(dtype, C, S, [0, 1, 0, 0], mode=i % 3, momentum=(0.1, 0.5, 1.0)[i % 3]))
    # every mode x every family on a ragged three-group batch of a few chunks
    S = rmin + 5 if rmin * C <= 1 << 16 else 11
    for fi, fam in enumerate(FAMILIES):
        for mode in (0, 1, 2):
            if fam == "zero-pad":
                out.append(_case(dtype, C, S, [0, 0, 1, 2, 2, 3, 3, 3], G=5, G_update=3, mode=mode, family=fam))  # groups 3, 4: padding
            else:
                out.append(_case(dtype, C, S, [0, 0, 1, 2, 2, 2], mode=mode, family=fam, momentum=(0.1, 0.5, 1.0)[(fi + mode) % 3]))
    S = 7 if C >= 512 else 40
    out.append(_case(dtype, C, S, [0, 1, 0, 1], mode=1, affine=False))
    out.append(_case(dtype, C, S, [0, 1, 0, 1], mode=2, running=False))
    out.append(_case(dtype, C, S, [0, 1, 0, 1], mode=0, affine=False, running=False, G_update=0))
    if (dtype, C) in GROUP_COLUMNS:                          # the group classes: modes 1 and 2 on each
        S = 5 if C >= 1024 else 33
        for mode in (1, 2):
            for G in (1, 8, 9, 16, 17):
                N = G + 3
                out.append(_case(dtype, C, S, [n % G for n in range(N)], mode=mode, momentum=1.0 if G in (9, 17) else 0.5,
                                 family="scaled" if G in (9, 16) else "normal"))
                out.append(_case(dtype, C, S, [n % G for n in range(N)], G_update=G - 1, mode=mode, momentum=1.0))
            out.append(_case(dtype, C, S, _shuffled(40, 17, 5), mode=mode, family="scaled"))            # N = 40, G = 17
            out.append(_case(dtype, C, S, [0, 0, 2, 2, 2], mode=mode, momentum=1.0))                   # sizes [2, 0, 3]
            out.append(_case(dtype, C, S, [0, 1, 1, 2, 2, 2, 3, 4, 4], G=6, G_update=3, mode=mode, family="zero-pad"))   # 3, 4: zeros; 5: empty
            out.append(_case(dtype, C, S, [2, 0, 1, 1, 0, 2, 2], G_update=0, mode=mode))
            out.append(_case(dtype, C, 1, [0, 1, 1, 1, 2, 2, 1], mode=mode, momentum=1.0))             # group 0: 1 sample x S = 1
    if (dtype, C) == (F32, 20):
        out.append(_case(dtype, C, 409, [0, 1, 0], mode=1))
    if (dtype, C) == (F32, 32):
        out += [_case(dtype, C, S, [0, 1, 1], mode=m) for S in (256, 257) for m in (0, 2)]
    if (dtype, C) == (F32, 1024):
        out += [_case(dtype, C, 139, [0, 1, 0], mode=m, family="scaled") for m in (0, 1, 2)]           # 18 chunks x 3 samples
    for i, c in enumerate(out):
        c["seed"] = 1000 * C + 17 * i + dtype
        c["name"] = "%s S%d N%d G%d/%d m%d %s%s%s mom%g #%d" % (column_name(dtype, C), c["S"], c["N"], c["G"], c["G_update"],
                                                                c["mode"], c["family"], "" if c["affine"] else " noaffine",
                                                                "" if c["running"] else " norunning", c["momentum"], i)
    return out


def large_case():
    c = _case(LARGE["dtype"], LARGE["C"], LARGE["S"], [0, 1], mode=2, family="scaled", momentum=0.5, seed=99)
    c["name"] = "large f32-C1024 S8300 N2 m2 scaled"
    return c


def all_gbn_cases(with_large=False):
    out = [c for d, C in COLUMNS for c in gbn_cases(d, C)]
    return out + [large_case()] if with_large else out


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def gbn_inputs(case):
    """fp32-representable inputs as float32 CPU tensors (the float64 cases read the same values): x, dy, residual (N, S, C),
    weight, bias, running_mean, running_var (C), ``zero_bias`` channels of the zero-pad family"""
    rng = np.random.default_rng(case["seed"])
    N, S, C, fam = case["N"], case["S"], case["C"], case["family"]
    f = np.float32
    std = (rng.random((1, 1, C)) * 3 + 0.2).astype(f)
    if fam == "offset1000":            # values away from the middle of their distribution: no pre-activation near 0, see mask_edges
        u = rng.standard_normal((N, S, C)).astype(f)
        u = np.sign(u) * (np.abs(u) * 0.5 + 0.6)
    else:
        u = rng.standard_normal((N, S, C)).astype(f)
    off = {"offset100": 100.0, "offset1000": 1000.0}.get(fam)
    mean = (std * off * np.sign(rng.standard_normal((1, 1, C)))).astype(f) if off else (rng.standard_normal((1, 1, C)) * 2).astype(f)
    x = (u * std + mean).astype(f)
    go = np.asarray(case["group_of"])
    if fam == "scaled":
        x = x * (1000.0 ** (go % 2)).astype(f)[:, None, None]
    if fam == "constant":              # channels 1, 5, 9 ...: constant within every group (another constant per group)
        for g in range(case["G"]):
            x[go == g, :, 1::4] = (rng.standard_normal((1, 1, len(range(1, C, 4)))) * 3).astype(f)
    weight = (rng.random(C) + 0.5).astype(f)
    bias = (rng.standard_normal(C) * (0.15 if fam == "offset1000" else 0.5)).astype(f)
    res = rng.standard_normal((N, S, C)).astype(f) * (0.1 if fam == "offset1000" else 1.0)
    if fam == "constant":              # there the pre-activation is bias [+ residual] for a whole group: kept off the mask's edge
        bias[1::4] = np.where(bias[1::4] < 0, -0.25, 0.25) + bias[1::4]
        res[:, :, 1::4] *= f(0.1)
    zero_bias = np.zeros(C, bool)
    if fam == "zero-pad":
        pad = go >= case["G_update"]
        x[pad] = 0.0
        zero_bias[::3] = True
        bias[zero_bias] = 0.0
        r = res[pad]
        r[:, :, zero_bias] = 0.0
        res[pad] = r
    if not case["affine"]:
        weight, bias = np.ones(C, f), np.zeros(C, f)
    dy = rng.standard_normal((N, S, C)).astype(f)
    rm, rv = rng.standard_normal(C).astype(f), (rng.random(C) + 0.5).astype(f)
    t = torch.from_numpy
    return dict(x=t(x), dy=t(dy), residual=t(res.astype(f)), weight=t(weight), bias=t(bias), running_mean=t(rm),
                running_var=t(rv), zero_bias=t(zero_bias))


# ---- the float64 referee -----------------------------------------------------------------------------------------------------
def gbn_referee(case, x, dy, residual, weight, bias, running_mean, running_var, defect=None):
    """include/sp3d.h:570-592 in float64, group by group, on the device of ``x`` ((N, S, C), any float type).  Empty group:
    mean 0, invstd 1/sqrt(eps); a group of at most one value makes no running update.  ``weight`` / ``bias`` /
    ``running_*`` may be None.  ``defect`` emulates a wrong kernel (tests/test_train_sweep_reference.py)."""
    d = torch.float64
    x, dy = x.to(d), dy.to(d)
    N, S, C = x.shape
    G, mode, mom = case["G"], case["mode"], case["momentum"]
    dev = x.device
    w = torch.ones(C, dtype=d, device=dev) if weight is None else weight.to(d)
    b = torch.zeros(C, dtype=d, device=dev) if bias is None else bias.to(d)
    go = torch.as_tensor(case["group_of"], device=dev)
    mean, var = torch.zeros(G, C, dtype=d, device=dev), torch.zeros(G, C, dtype=d, device=dev)
    cnt = [s * S for s in case["sizes"]]
    idx = [torch.nonzero(go == g).flatten() for g in range(G)]
    for g in range(G):
        if cnt[g]:
            xg = x[idx[g]].reshape(-1, C)
            mean[g] = xg.mean(0)
            var[g] = ((xg - mean[g]) ** 2).mean(0)
    if defect == "pooled" and G >= 2:                      # groups 0 and 1 share their statistics
        xg = x[torch.cat([idx[0], idx[1]])].reshape(-1, C)
        mean[0] = mean[1] = xg.mean(0)
        var[0] = var[1] = ((xg - mean[0]) ** 2).mean(0)
    if defect == "replica":                                # one of sixteen replica sums of group 0 is lost
        ex2 = (var[0] + mean[0] ** 2) * 15 / 16
        mean[0] = mean[0] * 15 / 16
        var[0] = (ex2 - mean[0] ** 2).clamp_min(0)
    if defect == "skip8":                                  # the second round of gbn_replica_fetch never happens
        mean[8:], var[8:] = 0.0, 0.0
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale, shift = w * invstd, b - mean * w * invstd
    sc_n, sh_n = scale[go][:, None, :], shift[go][:, None, :]
    pre = (x - mean[go][:, None, :]) * sc_n + b
    if mode == 2:
        pre = pre + residual.to(d)
    mask = (pre >= 0 if defect == "ge" else pre > 0) if mode else torch.ones_like(pre, dtype=torch.bool)
    y = torch.where(mask, pre, torch.zeros_like(pre)) if mode else pre
    dym = dy * mask
    xhat = (x - mean[go][:, None, :]) * invstd[go][:, None, :]
    gb_g, gw_g = torch.zeros(G, C, dtype=d, device=dev), torch.zeros(G, C, dtype=d, device=dev)
    for g in range(G):
        if cnt[g]:
            gb_g[g] = dym[idx[g]].sum((0, 1))
            gw_g[g] = (dym[idx[g]] * xhat[idx[g]]).sum((0, 1))
    cn = torch.tensor([max(c, 1) for c in cnt], dtype=d, device=dev)[:, None]
    a_g, b_g = gb_g / cn, gw_g / cn
    k1, k2 = scale, -scale * b_g * invstd
    k3a, k3b = -scale * a_g, -k2 * mean                    # k3 = k3a + k3b
    dx = scale[go][:, None, :] * (dym - a_g[go][:, None, :] - xhat * b_g[go][:, None, :])
    rm = None if running_mean is None else running_mean.to(d).clone()
    rv = None if running_var is None else running_var.to(d).clone()
    order = range(case["G_update"])
    for g in (reversed(order) if defect == "reverse" else order):
        if cnt[g] > 1 and rm is not None:
            unb = 1.0 if defect == "biased" else cnt[g] / (cnt[g] - 1.0)
            rm = (1 - mom) * rm + mom * mean[g]
            rv = (1 - mom) * rv + mom * var[g] * unb
    # first-order rounding bounds of the header's formula as the kernels evaluate it (fp32): y = fma(x, s, t) with s and t
    # rounded, t = b - mean s with mean and invstd rounded first; dx = fma(k1, dy, fma(k2, x, k3)), see test_gpu_train_sweep.py
    xs = (x * sc_n).abs()
    ms = (mean * scale).abs()[go][:, None, :]
    y_bound = 1.5 * U24 * (2 * xs + 3 * ms + b.abs() + y.abs())
    k1d, k2x = (k1[go][:, None, :] * dym).abs(), (k2[go][:, None, :] * x).abs()
    k3m = (k3a.abs() + k3b.abs())[go][:, None, :]
    mis = (mean * invstd).abs()[go][:, None, :]
    lever = mis * scale.abs()[go][:, None, :] * (b_g.abs()[go][:, None, :] + (xhat * a_g[go][:, None, :]).abs())
    dx_bound = 1.5 * U24 * (2 * k1d + 3 * k2x + 3 * k3m + dx.abs() + lever)
    return dict(y=y, pre=pre, mask=mask, dx=dx, grad_residual=dym if mode == 2 else None, mean=mean, var=var, invstd=invstd,
                scale=scale, shift=shift, grad_weight=gw_g.sum(0), grad_bias=gb_g.sum(0), gw_g=gw_g, gb_g=gb_g,
                running_mean=rm, running_var=rv, cnt=cnt, idx=idx, y_bound=y_bound, dx_bound=dx_bound,
                tau=32 * U24 * torch.clamp(xs + sh_n.abs(), min=1.0))


MASK_EDGE_CAP = 1e-3


def mask_edges(case, ref):
    """elements whose pre-activation is within rounding of 0: the fp32 and the float64 side may disagree on the ReLU mask
    there, so dy is set to 0 on them (modes 1 and 2; not the zero-pad family, whose exact zeros agree on both sides).
    -> bool (N, S, C)"""
    if case["mode"] == 0 or case["family"] == "zero-pad":
        return torch.zeros_like(ref["mask"])
    return ref["pre"].abs() < ref["tau"]


def gbn_problem(case, device="cpu", defect=None):
    """inputs on ``device`` in the case's type with dy zeroed at the mask edges, and the referee on them:
    -> (inputs, referee, share of dy zeroed)"""
    ins = {k: v.to(device) for k, v in gbn_inputs(case).items()}
    if not case["affine"]:
        ins["weight"] = ins["bias"] = None
    if not case["running"]:
        ins["running_mean"] = ins["running_var"] = None
    args = [ins[k] for k in ("x", "dy", "residual", "weight", "bias", "running_mean", "running_var")]
    edge = mask_edges(case, gbn_referee(case, *args))
    ins["dy"] = torch.where(edge, torch.zeros_like(ins["dy"]), ins["dy"])
    args[1] = ins["dy"]
    return ins, gbn_referee(case, *args, defect=defect), float(edge.double().mean())


def gbn_library(case, x, dy, residual, weight, bias):
    """the library's form in the type of ``x``: one F.batch_norm [+ add] [+ relu] per group under autograd
    -> dict(y, dx, grad_residual), None for a group the library refuses (at most one value per channel)"""
    import torch.nn.functional as Fn
    out = dict(y=torch.zeros_like(x), dx=torch.zeros_like(x), grad_residual=torch.zeros_like(x), served=[])
    go = torch.as_tensor(case["group_of"], device=x.device)
    for g in range(case["G"]):
        idx = torch.nonzero(go == g).flatten()
        if case["sizes"][g] * case["S"] <= 1:
            out["served"].append(False)
            continue
        xg = x[idx].clone().requires_grad_(True)
        rg = residual[idx].clone().requires_grad_(True)
        y = Fn.batch_norm(xg.permute(0, 2, 1), None, None, weight, bias, True, 0.0, EPS).permute(0, 2, 1)
        if case["mode"] == 2:
            y = y + rg
        if case["mode"]:
            y = torch.relu(y)
        y.backward(dy[idx])
        out["y"][idx] = y.detach()
        out["dx"][idx] = xg.grad
        if case["mode"] == 2:
            out["grad_residual"][idx] = rg.grad
        out["served"].append(True)
    return out


# ---- the comparison -------------------------------------------------------------------------------------------------------
F64_TOL = dict(y=1e-9, grad=1e-7, stat=1e-12)          # tests/test_gpu_grouped_bn.py
FACTOR = 1.5
# groups whose y / dx / grad_residual may be over FACTOR x the library form + 1e-7 if they stay within the first-order
# rounding bound of the referee: (what qualifies, the reason)
FLAGGED = {
    "one value": "the library refuses a group of one value per channel (training-mode F.batch_norm raises): no yardstick",
    "constant": "a channel constant within its group (var = 0): y = fma(x, s, t) rounds t = b - mean s at |mean| w / sqrt(eps), "
                "about 300 |mean|, where the library subtracts the mean first and is exact; the error is the bound's 3 |mean s| term",
}


def flag_of(case, g):
    if case["sizes"][g] * case["S"] == 1:
        return "one value"
    if case["family"] == "constant":
        return "constant"
    return None


def group_err(got, ref, idx):
    """max|got - f64| / max(1, max|f64|) over the samples ``idx``"""
    r = ref[idx]
    return float((got[idx].double() - r).abs().max() / max(1.0, float(r.abs().max())))


def f64_factor(ref):
    """digits the documented E[x^2] - mean^2 loses: max(1, mean^2 / var) of the worst channel (var + eps: finite at var = 0)"""
    return max(1.0, float((ref["mean"] ** 2 / (ref["var"] + EPS)).max()))


def gbn_compare(case, got, ref, lib=None, forward_only=False):
    """every accuracy rule of the sweep on one forward + backward: ``got`` holds y, dx, grad_residual, mean, invstd,
    grad_weight, grad_bias, running_mean, running_var as the kernels left them, ``lib`` the library's fp32 form (fp32 only)
    -> (failures, record)"""
    fails, rec = [], dict(case=case["name"], groups=[])
    f32 = case["dtype"] == F32
    fac = 1.0 if f32 else f64_factor(ref)
    names = ["y"] if forward_only else ["y", "dx"] + (["grad_residual"] if case["mode"] == 2 else [])
    for g in range(case["G"]):
        idx = ref["idx"][g]
        if not ref["cnt"][g]:
            continue
        for nm in names:
            e = group_err(got[nm], ref[nm], idx)
            if not f32:
                tol = (F64_TOL["y"] if nm == "y" else F64_TOL["grad"]) * fac
                rec["groups"].append(dict(g=g, what=nm, err=e, tol=tol))
                if not e <= tol:
                    fails.append((case["name"], "float64 %s of group %d over its tolerance" % (nm, g), e, tol))
                continue
            el = group_err(lib[nm], ref[nm], idx) if lib is not None and lib["served"][g] else None
            r = dict(g=g, what=nm, err=e, library=el, ratio=None if el is None else e / max(el, 1e-12))
            if el is None or not e <= FACTOR * el + 1e-7:
                flag = flag_of(case, g)
                bound = ref["y_bound"] if nm == "y" else ref["dx_bound"] if nm == "dx" else U24 * ref[nm].abs()    # a copy of dy: exact
                share = float(((got[nm][idx].double() - ref[nm][idx]).abs() / bound[idx].clamp_min(1e-300)).max())
                r.update(flagged=flag, bound_share=share)
                if flag is None:
                    fails.append((case["name"], "%s of group %d over %g x the library form + 1e-7 (kernel, library)" % (nm, g, FACTOR), e, el))
                elif not share <= 1.0:
                    fails.append((case["name"], "%s of the flagged group %d over the first-order bound (share)" % (nm, g), share, flag))
            rec["groups"].append(r)
    tol_stat = U23 if f32 else F64_TOL["stat"]
    tol_is = U23 if f32 else F64_TOL["y"] * fac
    used = {}

    def rule(name, err, bound):
        """err <= bound elementwise; records the largest share of the bound in use"""
        share = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        used[name] = share
        if not share <= 1.0:
            fails.append((case["name"], name + " over its bound (share of the bound)", share))
    live = torch.tensor([c > 0 for c in ref["cnt"]], device=ref["mean"].device)
    rule("mean", (got["mean"].double() - ref["mean"]).abs(), tol_stat * ref["mean"].abs() + (0 if f32 else tol_stat))
    rule("invstd", (got["invstd"].double() - ref["invstd"]).abs(), tol_is * ref["invstd"].abs())
    if not bool((got["mean"][~live] == 0).all()):
        fails.append((case["name"], "the mean of an empty group is not 0"))
    for nm in ("running_mean", "running_var"):
        if ref[nm] is not None:
            rule(nm, (got[nm].double() - ref[nm]).abs(), torch.full_like(ref[nm], tol_stat * fac * float(ref[nm].abs().max())))
    gb, gw = ref["grad_bias"], ref["grad_weight"]
    if forward_only:
        pass
    elif f32:
        lever = (ref["gw_g"].abs() + ref["gb_g"].abs() * (ref["mean"] * ref["invstd"]).abs()).sum(0)
        rule("grad_bias", (got["grad_bias"].double() - gb).abs(), U23 * gb.abs())
        rule("grad_weight", (got["grad_weight"].double() - gw).abs(), U23 * (gw.abs() + lever))
    else:
        tg = F64_TOL["grad"] * fac
        rule("grad_bias", (got["grad_bias"].double() - gb).abs(), torch.full_like(gb, tg * max(1.0, float(gb.abs().max()))))
        rule("grad_weight", (got["grad_weight"].double() - gw).abs(), torch.full_like(gw, tg * max(1.0, float(gw.abs().max()))))
    rec["bound_used"] = used
    return fails, rec


def round_like(case, ref):
    """the referee's outputs rounded to the case's type: what a faultless kernel may return at best"""
    t = torch.float32 if case["dtype"] == F32 else torch.float64
    return {k: (None if ref[k] is None else ref[k].to(t)) for k in ("y", "dx", "grad_residual", "mean", "invstd", "grad_weight",
                                                                    "grad_bias", "running_mean", "running_var")}


# ---- rendering: tables ------------------------------------------------------------------------------------------------------
TARGET_TOL, ROOT_TOL = 1e-6, 2e-5       # tests/test_gpu_end_to_end.py


# the 3-D target volume: integer-valued grids and an integer sigma, roots on quarter units - every subtraction is exact in fp32
def target_cases():
    out = []
    for shape in ((5, 7, 9), (1, 1, 1)):
        for R in (1, 10):
            for fam in ("random", "window edge", "outside"):
                out.append(dict(shape=shape, R=R, family=fam, sigma=2.0, step=3, B=2, seed=300 + len(out),
                                name="target %dx%dx%d R%d %s" % (shape + (R, fam))))
    return out


def target_inputs(case):
    rng = np.random.default_rng(case["seed"])
    X, Y, Z = case["shape"]
    B, R, s, step = case["B"], case["R"], case["sigma"], case["step"]
    grids = [np.arange(n, dtype=np.float32) * step + o for n, o in zip((X, Y, Z), (-6.0, 10.0, 100.0))]
    hi = [g[-1] for g in grids]
    roots = np.stack([np.round(rng.uniform(g[0] - 2 * s, g[-1] + 2 * s, (B, R)) * 4) / 4 for g in grids], -1).astype(np.float32)
    edge = []
    if case["family"] == "window edge":         # root r: on the grid in two axes, exactly 3 sigma off a grid plane in axis r % 3
        for b in range(B):
            for r in range(R):
                at = [int(rng.integers(0, n)) for n in (X, Y, Z)]
                roots[b, r] = [grids[a][at[a]] for a in range(3)]
                roots[b, r, r % 3] += 3 * s * (1 if (r // 3 + b) % 2 else -1)
                edge.append((b,) + tuple(at))
    if case["family"] == "outside":
        roots[0] = [[hi[0] + 3 * s + 0.25, grids[1][0], grids[2][0]]] * R      # a quarter unit beyond the window of every voxel
    return dict(roots=torch.from_numpy(roots), gx=torch.from_numpy(grids[0]), gy=torch.from_numpy(grids[1]),
                gz=torch.from_numpy(grids[2]), edge=edge)


def target_referee(roots, gx, gy, gz, sigma, inclusive=True):
    """sp3d.h:445: clip(max over roots of the 3-sigma-windowed Gaussian), float64; the window includes its edge"""
    d = torch.float64
    mu = roots.to(d)[:, :, None, None, None, :]
    dx = gx.to(d).view(1, 1, -1, 1, 1) - mu[..., 0]
    dy = gy.to(d).view(1, 1, 1, -1, 1) - mu[..., 1]
    dz = gz.to(d).view(1, 1, 1, 1, -1) - mu[..., 2]
    lim = 3.0 * sigma
    inside = ((dx.abs() <= lim) & (dy.abs() <= lim) & (dz.abs() <= lim)) if inclusive else \
        ((dx.abs() < lim) & (dy.abs() < lim) & (dz.abs() < lim))
    g = torch.exp(-(dx ** 2 + dy ** 2 + dz ** 2) / (2 * sigma ** 2)) * inside
    return g.amax(dim=1).clamp(0, 1)


# the root heat-maps
ROOT_IMAGES = [(3, 5), (129, 130)]


def root_blocks(h, w):
    b = (h * w + 255) // 256
    return min(b, 64), b > 64


def root_cases(h, w):
    return [dict(h=h, w=w, R=R, B=3, V=V, behind=behind, seed=500 + R + V, name="roots %dx%d R%d V%d%s" % (h, w, R, V, " behind" if behind else ""))
            for R, V, behind in ((1, 5, False), (10, 5, False), (10, 2, True), (1, 1, True))]


def root_inputs(case):
    """roots (B, R, 3) mm and the (B, V, 64) camera table with per-sample crops, every view under view 0's affine as
    CuboidProposalNetSoft._render_hip builds it; ``behind``: root 0 of sample 1 lies 1 m behind camera 0"""
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import CAM_A, finish, pack_cameras
    B, V, R = case["B"], case["V"], case["R"]
    meta = syn.make_meta(B, V, (960, 512), rotations=[0.0, 20.0, -35.0], scale_mults=[1.0, 0.8, 1.2])
    rng = np.random.default_rng(case["seed"])
    roots = (rng.uniform(-1, 1, (B, R, 3)) * [2500.0, 2500.0, 400.0] + [0.0, -500.0, 800.0]).astype(np.float32)
    tab = pack_cameras(meta, B, (960, 512))
    tab[:, :, CAM_A:CAM_A + 6] = tab[:, :1, CAM_A:CAM_A + 6]
    finish(tab)
    if case["behind"]:
        Rm, T = tab[1, 0, 0:9].reshape(3, 3).astype(np.float64), tab[1, 0, 9:12].astype(np.float64)
        roots[1, 0] = (T + Rm.T @ np.array([100.0, -50.0, -1000.0])).astype(np.float32)
    return dict(roots=torch.from_numpy(roots), cam=torch.from_numpy(tab), meta=meta, stride=960.0 / case["w"])       # the whole 960 px image on w heat-map px


def root_referee(roots, cam, h, w, stride):
    """the projection as sp3d_synth.hip:49-63 states it (cameras.py without the r^2 clamp, then the crop affine), float64
    -> (V, B, 1, h, w), the camera-space depths (B, V, R)"""
    d = torch.float64
    X, c = roots.to(d), cam.to(d)
    B, V = c.shape[:2]
    Rm, T = c[..., 0:9].reshape(B, V, 3, 3), c[..., 9:12]
    xc = torch.einsum("bvij,bvrj->bvri", Rm, X[:, None] - T[:, :, None])
    y = xc[..., :2] / (xc[..., 2:3] + 1e-5)
    r2 = (y ** 2).sum(-1, keepdim=True)
    k, p = c[..., None, 16:19], c[..., None, 19:21]
    radial = 1 + k[..., 0:1] * r2 + k[..., 1:2] * r2 ** 2 + k[..., 2:3] * r2 ** 3
    tan = p[..., 0:1] * y[..., 1:2] + p[..., 1:2] * y[..., 0:1]
    u = y * (radial + 2 * tan) + torch.cat([p[..., 1:2], p[..., 0:1]], -1) * r2
    px = c[..., None, 12:14] * u + c[..., None, 14:16]
    A = c[..., 21:27].reshape(B, V, 2, 3)
    q = (torch.einsum("bvij,bvrj->bvri", A[..., :2], px) + A[..., None, :, 2]) / stride
    ys = torch.arange(h, dtype=d, device=q.device).view(1, 1, 1, -1, 1)
    xs = torch.arange(w, dtype=d, device=q.device).view(1, 1, 1, 1, -1)
    g = torch.exp(-(((xs - q[..., 0, None, None]) / 3.0) ** 2) / 2 - (((ys - q[..., 1, None, None]) / 3.0) ** 2) / 2)
    return g.sum(2).clamp(0, 1).permute(1, 0, 2, 3).unsqueeze(2), xc[..., 2]
