"""The hand-written kernels that only the training step runs, against float64 at their edges: grouped BatchNorm
(sp3d_gbn_forward / _backward, six kernels) and the rendering kernels of the self-supervised losses (sp3d_gaussian_target_3d,
sp3d_render_root_heatmaps; sp3d_render_joints: see NOT HERE), reached through the C ABI.  tests/train_sweep_cases.py has the
tables, the inputs, the referees and the comparison; tests/test_train_sweep_reference.py checks those without a GPU.  One
parameter per column class (image class); inside it every case of the class.  Failures are collected and asserted once.

For every case:
  guarded buffers   every output is a view into the middle of a larger buffer, NaN inside, 4096 sentinel words on each side;
                    afterwards no NaN is left and the sentinels hold their bits.  Every input sits between 4096 NaN words on
                    each side.  The running statistics and the float64 workspace lie between sentinels too.
  workspace         one workspace per case serves a forward, a repeat of it, the backward and a forward on other data (-x);
                    after EACH call every word of it is bit-zero, and the last forward meets the bounds of the first.
  accuracy, fp32    per group, max|got - f64| / max(1, max|f64|): y, dx, grad_residual <= 1.5 x the error of the library's
                    fp32 form (per-group F.batch_norm [+ add] [+ relu] under autograd on the GPU) + 1e-7; a group of
                    ts.FLAGGED may be over that if it stays within the first-order rounding bound of the referee
                    (y: 1.5 2^-24 (2|x s| + 3|mean s| + |b| + |y|); dx: the same for fma(k1, dy, fma(k2, x, k3)) plus the
                    lever of the rounded mean, |mean invstd| |s| (|mean(dy xhat)| + |xhat mean(dy)|)).  mean, invstd within
                    2^-23 relative; running statistics within 2^-23 max|value|; grad_bias within 2^-23 |gb|; grad_weight
                    within 2^-23 (|gw| + sum_g (|gw_g| + |gb_g| |mean_g invstd_g|)).
  accuracy, float64 1e-9 (y), 1e-7 (gradients), 1e-12 (mean, running statistics) of tests/test_gpu_grouped_bn.py, the first
                    two times max(1, mean^2 / (var + eps)) of the case's worst channel.
  repeat            the statistics merge with float64 atomics, so their last bits may differ between two calls; where the
                    repeat's scale and shift have the bits of the first call's, its y has them too.  The rendering kernels
                    have no atomics: a second launch gives the same bits.

SP3D_TRAIN_SWEEP_RECORD=<file.json>: write one line per case (``compact``: the worst group of every output with the library's
error there, the share of each rule and bound in use, every flagged group) and one summary line per parameter
(profiles/r19_train_sweep_errors.json); -s prints the same per parameter.

Worst figures on the MI355X (profiles/r19_train_sweep_errors.json; 536 cases, none over a bound).
NOT HERE: sp3d_render_joints_fwd / _bwd.  A sweep of them met an illegal memory access on the GPU in its negative-count
cases: with count = -1 both kernels compare the unsigned thread index with it (``threadIdx.x < np``), so all 256 threads
load a keypoint row, up to 255 rows past the entry and past the end of kps (the results are right all the same).  With np
clamped to 0 .. P that sweep passed, but a run of the whole suite still ended with an illegal access of unknown origin,
so neither the clamp nor that sweep is part of this change; both wait for that cause.
fp32 grouped BatchNorm, per column class: the worst per-group error of y and of dx outside the flagged groups with the
library form's error on the same group, the largest share of the rule e <= 1.5 e_library + 1e-7 any group uses (y of either
forward / dx), and the largest share of the 2^-23 bounds (mean, invstd, running statistics, grad_bias, grad_weight):
  C 4      y 3.4e-5 (library 0.15)    dx 1.3e-6 (library 0.57)    rule used 0.97 / 0.43   statistics 0.48
  C 20     y 4.3e-5 (library 0.13)    dx 3.6e-6 (library 1.2e-4)  rule used 0.60 / 0.33   statistics 0.49
  C 32     y 4.9e-5 (library 0.087)   dx 2.1e-4 (library 0.020)   rule used 0.71 / 0.43   statistics 0.50
  C 48     y 5.3e-5 (library 0.10)    dx 3.9e-6 (library 0.042)   rule used 0.92 / 0.36   statistics 0.50
  C 1024   y 6.4e-5 (library 61)      dx 1.7e-5 (library 3.1e-3)  rule used 0.66 / 0.43   statistics 0.50
  C 1028   y 9.4e-5 (library 2.0)     dx 2.0e-5 (library 0.40)    rule used 0.96 / 0.64   statistics 0.50
  C 1536   y 5.8e-5 (library 0.29)    dx 1.9e-5 (library 0.27)    rule used 0.64 / 0.80   statistics 0.50
  C 2048   y 7.0e-5 (library 7.0)     dx 5.4e-5 (library 2.8)     rule used 0.85 / 0.42   statistics 0.50
  large    y 1.6e-7 (library 1.5e-5)  dx 7.2e-8 (library 1.6e-5)  rule used 0.01 / 0.00   statistics 0.50
The worst errors are all of the offset1000 family (|mean| / std = 1000: 2^-24 x 1000 = 6e-5 is the rounding of the inputs'
own offset) or of groups of two or three values; there the library's fp32 BatchNorm is off by 0.1 to 60 (its variance
cancels), so the rule binds on the other families: largest share 0.97, where both sides are at a few 1e-7.
FLAGGED groups (over the rule, held to the first-order bound instead): "one value" (no library form; worst y 2.0e-4, dx
8.8e-5, at most 0.27 of the bound) and "constant" (worst y 3.7e-5 against the library's 1.3e-6 .. 2e-5, at most 0.73 of the
bound, the 3 |mean s| term).  No other group is over the rule.
float64, per column class (tolerance x max(1, mean^2 / var), about 1e6 at the worst case): y at most 9.9e-10 (C 512,
offset1000), dx 4.0e-10, mean 2.2e-4 of its 1e-12, running_var 1.1e-3 of its bound.
Repeats: in 516 of 516 cases the second call's scale and shift had the bits of the first (and so had y).
Rendering: target 3.2e-8 (1e-6), root maps 3.4e-6 at 129 x 130 (2e-5); every repeat bit-equal.
Wrong kernels built on a scratch copy and run once (not committed), and what caught them: the re-zeroing dropped for
groups 8.. - "the workspace is not all bit-zero" after every call with G > 8 (and dx, grad_weight, grad_bias of group 8..);
the running updates in reverse order - running_mean and running_var in every column class; cnt / (cnt - 1) dropped -
running_var alone; >= in the masks - dx, grad_residual, grad_bias and grad_weight (mode 2 everywhere, mode 1 in the
zero-pad family); < at the window edge - the "window edge" targets.  The pooled statistics, the lost replica, the
skipped groups and the two out-of-bounds breakages (``c < C``, ``col < CV`` dropped): emulated in
tests/test_train_sweep_reference.py.
"""
import collections
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import train_sweep_cases as ts

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0x5A5A5A5A
_T = {ts.F32: torch.float32, ts.F64: torch.float64}


class Guarded:
    """``n`` elements of ``dtype`` inside a larger buffer, with GUARD sentinel elements on each side; NaN inside unless
    ``init`` (running statistics) or ``zero`` (the workspace: its guards are zero words too - a stray atomic ADD would
    leave a word as large as the sentinel pattern, 6e125, unchanged)"""

    def __init__(self, n, dtype, dev, init=None, zero=False):
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        k = self.buf.element_size() // 4
        self.bits = self.buf.view(torch.int32)
        self.lo, self.hi = GUARD * k, (GUARD + n) * k
        self.sentinel = 0 if zero else SENTINEL
        self.bits[:self.lo] = self.sentinel
        self.bits[self.hi:] = self.sentinel
        self.t = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(init.reshape(-1))
        else:
            self.t.fill_(0.0 if zero else float("nan"))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def problems(self, what, nan_ok=False):
        p = []
        if not bool((self.bits[:self.lo] == self.sentinel).all()):
            p.append("the guard BEFORE %s was written" % what)
        if not bool((self.bits[self.hi:] == self.sentinel).all()):
            p.append("the guard AFTER %s was written" % what)
        if not nan_ok and bool(torch.isnan(self.t).any()):
            p.append("a NaN is left in %s" % what)
        return p

    def untouched(self):
        return bool(torch.isnan(self.t).all()) and not self.problems("", nan_ok=True)


def padded(t, dtype, dev):
    """a tensor on the GPU in ``dtype`` between GUARD NaN elements on each side"""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = t.reshape(-1).to(dev, dtype)
    return buf[GUARD:GUARD + n].view(t.shape)


def bits_equal(a, b):
    v = torch.int32 if a.element_size() == 4 else torch.int64
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def r3(v):
    return None if v is None else float("%.3e" % v)


# ---- grouped BatchNorm ------------------------------------------------------------------------------------------------------
class GbnRun:
    """the buffers of one case and the two entries on them"""

    def __init__(self, case, ins, dev):
        from selfpose3d_amd import _lib
        self.lib, self.case, self.dev = _lib.load(), case, dev
        self.t = t = _T[case["dtype"]]
        N, S, C, G = case["N"], case["S"], case["C"], case["G"]
        self.go = torch.tensor(case["group_of"], dtype=torch.int32, device=dev)
        self.gs = torch.tensor(case["sizes"], dtype=torch.int32, device=dev)
        self.x, self.dy, self.res = (padded(ins[k], t, dev) for k in ("x", "dy", "residual"))
        self.w = None if ins["weight"] is None else padded(ins["weight"], t, dev)
        self.b = None if ins["bias"] is None else padded(ins["bias"], t, dev)
        self.rm = None if ins["running_mean"] is None else Guarded(C, t, dev, init=ins["running_mean"])
        self.rv = None if ins["running_var"] is None else Guarded(C, t, dev, init=ins["running_var"])
        words = self.lib.sp3d_gbn_workspace_bytes(G, C) // 8
        assert words == 16 * G * C * 2
        self.ws = Guarded(words, torch.float64, dev, zero=True)

    def workspace_problems(self, after):
        p = self.ws.problems("the workspace")
        if int(torch.count_nonzero(self.ws.t.view(torch.int64))):
            p.append("the workspace is not all bit-zero after " + after)
        return p

    def forward(self, x, running=True):
        from selfpose3d_amd import _lib
        c, t, dev = self.case, self.t, self.dev
        N, S, C, G = c["N"], c["S"], c["C"], c["G"]
        o = dict(y=Guarded(N * S * C, t, dev), **{k: Guarded(G * C, t, dev) for k in ("mean", "invstd", "scale", "shift")})
        rm, rv = (self.rm, self.rv) if running else (None, None)
        rc = self.lib.sp3d_gbn_forward(x.data_ptr(), o["y"].ptr, c["dtype"], self.go.data_ptr(), self.gs.data_ptr(), N, S, C, G,
                                       c["G_update"], _lib._opt(self.w), _lib._opt(self.b), None if rm is None else rm.ptr,
                                       None if rv is None else rv.ptr, ts.EPS, c["momentum"], c["mode"],
                                       self.res.data_ptr() if c["mode"] == 2 else None, o["mean"].ptr, o["invstd"].ptr,
                                       o["scale"].ptr, o["shift"].ptr, self.ws.ptr, _lib._stream(dev))
        _lib.check(rc, "sp3d_gbn_forward")
        return o

    def backward(self, fwd):
        from selfpose3d_amd import _lib
        c, t, dev = self.case, self.t, self.dev
        N, S, C, G = c["N"], c["S"], c["C"], c["G"]
        o = dict(dx=Guarded(N * S * C, t, dev), k123=Guarded(3 * G * C, t, dev), grad_weight=Guarded(C, t, dev),
                 grad_bias=Guarded(C, t, dev))
        if c["mode"] == 2:
            o["grad_residual"] = Guarded(N * S * C, t, dev)
        ysaved = padded(fwd["y"].t, t, dev)
        stats = {k: padded(fwd[k].t, t, dev) for k in ("mean", "invstd", "scale", "shift")}
        rc = self.lib.sp3d_gbn_backward(self.x.data_ptr(), self.dy.data_ptr(), o["dx"].ptr, c["dtype"], self.go.data_ptr(),
                                        self.gs.data_ptr(), N, S, C, G, _lib._opt(self.w), stats["mean"].data_ptr(),
                                        stats["invstd"].data_ptr(), stats["scale"].data_ptr(), stats["shift"].data_ptr(), c["mode"],
                                        ysaved.data_ptr() if c["mode"] == 2 else None,
                                        o["grad_residual"].ptr if c["mode"] == 2 else None, o["grad_weight"].ptr,
                                        o["grad_bias"].ptr, o["k123"].ptr, self.ws.ptr, _lib._stream(dev))
        _lib.check(rc, "sp3d_gbn_backward")
        return o


def sweep_gbn_case(case, dev, failures, records, tally):
    name = case["name"]
    N, S, C, G = case["N"], case["S"], case["C"], case["G"]
    ins, ref, edge = ts.gbn_problem(case, dev)
    run = GbnRun(case, ins, dev)
    shape = (N, S, C)

    def guards(bufs, after):
        for k, g in bufs.items():
            for p in g.problems(k):
                failures.append((name, p + " (" + after + ")"))
        for k, g in (("running_mean", run.rm), ("running_var", run.rv)):
            if g is not None:
                for p in g.problems(k):
                    failures.append((name, p + " (" + after + ")"))
        for p in run.workspace_problems(after):
            failures.append((name, p))
    f1 = run.forward(run.x)
    guards(f1, "the forward")
    got = {k: f1[k].t.view(G, C).clone() for k in ("mean", "invstd")}
    got["y"] = f1["y"].t.view(shape)
    if run.rm is not None:
        got["running_mean"], got["running_var"] = run.rm.t.clone(), run.rv.t.clone()
    f1b = run.forward(run.x, running=False)                  # the repeat: same data, no running update
    guards(f1b, "the repeated forward")
    same_stats = bits_equal(f1["scale"].t, f1b["scale"].t) and bits_equal(f1["shift"].t, f1b["shift"].t)
    tally["repeats"] += 1
    tally["repeat_stats_differ"] += int(not same_stats)
    if same_stats and not bits_equal(f1["y"].t, f1b["y"].t):
        failures.append((name, "the same scale and shift gave other bits of y in a second call"))
    bw = run.backward(f1)
    guards(bw, "the backward")
    got.update(dx=bw["dx"].t.view(shape), grad_weight=bw["grad_weight"].t, grad_bias=bw["grad_bias"].t)
    if case["mode"] == 2:
        got["grad_residual"] = bw["grad_residual"].t.view(shape)
    lib = None
    if case["dtype"] == ts.F32:
        lib = ts.gbn_library(case, run.x, run.dy, run.res, run.w, run.b)
    fails, rec = ts.gbn_compare(case, got, ref, lib)
    failures += fails
    # a forward on other data through the same workspace, the running statistics going on from where the first left them
    x2 = padded(-run.x, run.t, dev)
    rm0 = None if run.rm is None else run.rm.t.clone()
    rv0 = None if run.rv is None else run.rv.t.clone()
    f2 = run.forward(x2)
    guards(f2, "the forward on other data")
    ref2 = ts.gbn_referee(case, x2, torch.zeros_like(x2), run.res, run.w, run.b, rm0, rv0)
    got2 = dict(y=f2["y"].t.view(shape), mean=f2["mean"].t.view(G, C), invstd=f2["invstd"].t.view(G, C))
    if run.rm is not None:
        got2["running_mean"], got2["running_var"] = run.rm.t, run.rv.t
    lib2 = ts.gbn_library(case, x2, torch.zeros_like(x2), run.res, run.w, run.b) if case["dtype"] == ts.F32 else None
    fails2, rec2 = ts.gbn_compare(case, got2, ref2, lib2, forward_only=True)
    failures += [(f[0], "[forward on other data] " + f[1]) + tuple(f[2:]) for f in fails2]
    # the compact record: per output the per-group errors, the library's, the shares of the bounds
    out = dict(case=name, edge_share=r3(edge), repeat_stats_equal=same_stats, bound_used={k: r3(v) for k, v in rec["bound_used"].items()},
               second_forward_bound_used={k: r3(v) for k, v in rec2["bound_used"].items()})
    for tag, rr in (("", rec), ("second_forward_", rec2)):
        for g in rr["groups"]:
            d = out.setdefault(tag + g["what"], collections.defaultdict(list))
            d["g"].append(g["g"])
            d["err"].append(r3(g["err"]))
            if "library" in g:
                d["library"].append(r3(g["library"]))
            if g.get("flagged"):
                d["flagged"].append([g["g"], g["flagged"], r3(g["bound_share"])])
    records.append(out)


USED = ("mean", "invstd", "running_mean", "running_var", "grad_weight", "grad_bias")
OUTPUTS = ("y", "dx", "grad_residual", "second_forward_y")


def compact(rec):
    """a case's line of the error file: per output [group, error, library error] of its worst group and the largest share
    of the rule e <= 1.5 e_library + 1e-7 an unflagged group uses; every flagged group as [output, group, flag, share of the
    first-order bound, error]; the shares of the bounds on USED (null: not checked) and the largest of them in the second forward"""
    out = dict(case=rec["case"], edge_share=rec["edge_share"])
    if not rec["repeat_stats_equal"]:
        out["repeat_stats_equal"] = False
    flags = []
    for what in OUTPUTS:
        d = rec.get(what)
        if not d:
            continue
        lib = d.get("library") or [None] * len(d["err"])
        flagged = {f[0]: f for f in d.get("flagged", [])}
        i = max(range(len(d["err"])), key=lambda j: d["err"][j])
        rule = [e / (ts.FACTOR * l + 1e-7) for g, e, l in zip(d["g"], d["err"], lib) if l is not None and g not in flagged]
        out[what] = [d["g"][i], d["err"][i], lib[i], r3(max(rule)) if rule else None]
        flags += [[what, g, f[1], f[2], d["err"][d["g"].index(g)]] for g, f in flagged.items()]
    if flags:
        out["flagged"] = flags
    out["used"] = [rec["bound_used"].get(k) for k in USED]
    out["used_second_forward"] = max(rec["second_forward_bound_used"].values())
    return out


def gbn_summary(name, records, tally):
    s = dict(summary=True, param=name, cases=len(records), repeats=tally["repeats"], repeat_stats_differ=tally["repeat_stats_differ"])
    for what in ("y", "dx", "grad_residual", "second_forward_y"):
        best = None
        for r in records:
            d = r.get(what)
            if not d:
                continue
            flagged = {f[0] for f in d.get("flagged", [])}
            for i, e in enumerate(d["err"]):
                l = d["library"][i] if d.get("library") else None
                rule = None if l is None or d["g"][i] in flagged else e / (ts.FACTOR * l + 1e-7)
                if best is None or e > best["err"]:
                    best = dict(err=e, library=l, case=r["case"], group=d["g"][i])
                if rule is not None:
                    s[what + "_rule_used"] = max(s.get(what + "_rule_used", 0.0), r3(rule))
        s[what] = best
    for k in ("mean", "invstd", "running_mean", "running_var", "grad_weight", "grad_bias"):
        v = [r["bound_used"][k] for r in records if k in r["bound_used"]]
        if v:
            s[k + "_bound_used"] = max(v)
    s["flagged"] = sorted({(f[1]) for r in records for what in ("y", "dx", "grad_residual", "second_forward_y")
                           for f in (r.get(what) or {}).get("flagged", [])})
    s["flagged_bound_share"] = max([f[2] for r in records for what in ("y", "dx", "grad_residual", "second_forward_y")
                                    for f in (r.get(what) or {}).get("flagged", [])] or [0.0])
    return s


def write_records(records):
    path = os.environ.get("SP3D_TRAIN_SWEEP_RECORD")
    if not path:
        return
    old = []
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in old + records) + "\n]\n")


def report(failures):
    kinds = collections.Counter(f[1] for f in failures)
    lines = [f"{len(failures)} failed checks: " + "; ".join(f"{n} x {k}" for k, n in kinds.items())]
    return "\n".join(lines + [repr(f) for f in failures[:60]])


def _run_gbn(name, cases):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    failures, records, tally = [], [], collections.Counter()
    t0 = time.perf_counter()
    for case in cases:
        sweep_gbn_case(case, dev, failures, records, tally)
    torch.cuda.synchronize(dev)
    summary = gbn_summary(name, records, tally)
    print(f"train sweep {name}: {len(records)} cases in {time.perf_counter() - t0:.1f} s, {summary}")
    write_records([compact(r) for r in records] + [summary])
    torch.cuda.empty_cache()
    assert not failures, report(failures)


@pytest.mark.parametrize("name", [ts.column_name(d, C) for d, C in ts.COLUMNS])
def test_gbn_sweep(name):
    dtype, C = next((d, C) for d, C in ts.COLUMNS if ts.column_name(d, C) == name)
    _run_gbn("gbn " + name, ts.gbn_cases(dtype, C))


def test_gbn_sweep_large():
    """rows above its minimum, 519 chunks, the apply grid capped at 2048 blocks: about 70 MB a tensor, the one slow case"""
    _run_gbn("gbn large", [ts.large_case()])


def test_gbn_widths_it_cannot_serve_are_refused_before_any_launch():
    from selfpose3d_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for dtype, C in ts.REFUSED:
        t = _T[dtype]
        N, S, G = 2, 3, 2
        go = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        gs = torch.tensor([1, 1], dtype=torch.int32, device=dev)
        x = padded(torch.ones(N, S, C), t, dev)
        outs = [Guarded(n, t, dev) for n in (N * S * C, G * C, G * C, G * C, G * C, N * S * C, 3 * G * C, C, C)]
        ws = Guarded(16 * G * C * 2, torch.float64, dev, zero=True)
        rc = lib.sp3d_gbn_forward(x.data_ptr(), outs[0].ptr, dtype, go.data_ptr(), gs.data_ptr(), N, S, C, G, G, None, None, None,
                                  None, ts.EPS, 0.1, 0, None, outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, ws.ptr,
                                  _lib._stream(dev))
        assert rc == ts.EUNSUPPORTED == ts.gbn_refusal(dtype, C), (dtype, C, rc)
        rc = lib.sp3d_gbn_backward(x.data_ptr(), x.data_ptr(), outs[5].ptr, dtype, go.data_ptr(), gs.data_ptr(), N, S, C, G, None,
                                   x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, None, None, outs[7].ptr, outs[8].ptr,
                                   outs[6].ptr, ws.ptr, _lib._stream(dev))
        assert rc == ts.EUNSUPPORTED, (dtype, C, rc)
        torch.cuda.synchronize(dev)
        assert all(o.untouched() for o in outs), (dtype, C)
        assert not ws.problems("the workspace") and not int(torch.count_nonzero(ws.t.view(torch.int64)))


# ---- rendering ---------------------------------------------------------------------------------------------------------------
def test_gaussian_target_sweep():
    from selfpose3d_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    failures, records = [], []
    for case in ts.target_cases():
        ins = ts.target_inputs(case)
        X, Y, Z = case["shape"]
        B, R = case["B"], case["R"]
        roots, gx, gy, gz = (padded(ins[k], torch.float32, dev) for k in ("roots", "gx", "gy", "gz"))
        ref = ts.target_referee(roots, gx, gy, gz, case["sigma"])
        got = []
        for rep in range(2):
            out = Guarded(B * X * Y * Z, torch.float32, dev)
            _lib.check(lib.sp3d_gaussian_target_3d(roots.data_ptr(), B, R, gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), X, Y, Z,
                                                   case["sigma"], out.ptr, _lib._stream(dev)), "sp3d_gaussian_target_3d")
            failures += [(case["name"], p) for p in out.problems("the target")]
            got.append(out.t.view(B, X, Y, Z))
        e = float((got[0].double() - ref).abs().max())
        if not e <= ts.TARGET_TOL:
            failures.append((case["name"], "target over 1e-6", e))
        if not bits_equal(got[0], got[1]):
            failures.append((case["name"], "a second launch gave other bits"))
        if case["family"] == "outside" and int(torch.count_nonzero(got[0][0])):
            failures.append((case["name"], "a root farther than 3 sigma from every voxel left a nonzero sample"))
        records.append(dict(case=case["name"], err=r3(e), max=r3(float(ref.max()))))
    summary = dict(summary=True, param="gaussian_target_3d", cases=len(records), err=max(r["err"] for r in records))
    print("train sweep", summary)
    write_records(records + [summary])
    assert not failures, report(failures)


@pytest.mark.parametrize("image", ["%dx%d" % hw for hw in ts.ROOT_IMAGES])
def test_render_root_heatmaps_sweep(image):
    from selfpose3d_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    h, w = next(hw for hw in ts.ROOT_IMAGES if "%dx%d" % hw == image)
    failures, records = [], []
    for case in ts.root_cases(h, w):
        ins = ts.root_inputs(case)
        B, R, V = case["B"], case["R"], case["V"]
        roots, cam = padded(ins["roots"], torch.float32, dev), padded(ins["cam"], torch.float32, dev)
        ref, depth = ts.root_referee(roots, cam, h, w, ins["stride"])
        got = []
        for rep in range(2):
            out = Guarded(V * B * h * w, torch.float32, dev)
            _lib.check(lib.sp3d_render_root_heatmaps(roots.data_ptr(), B, R, cam.data_ptr(), V, h, w, ins["stride"], out.ptr,
                                                     _lib._stream(dev)), "sp3d_render_root_heatmaps")
            failures += [(case["name"], p) for p in out.problems("the root maps")]
            got.append(out.t.view(V, B, 1, h, w))
        e = float((got[0].double() - ref).abs().max())
        if not e <= ts.ROOT_TOL:
            failures.append((case["name"], "root maps over 2e-5", e))
        if not bits_equal(got[0], got[1]):
            failures.append((case["name"], "a second launch gave other bits"))
        records.append(dict(case=case["name"], err=r3(e), max=r3(float(ref.max())), behind=int((depth < 0).sum())))
    summary = dict(summary=True, param="render_root_heatmaps " + image, cases=len(records), err=max(r["err"] for r in records))
    print("train sweep", summary)
    write_records(records + [summary])
    assert not failures, report(failures)
