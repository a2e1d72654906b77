"""Every kernel of the frequency-domain 7x7x7 opening conv against float64 at its tile, row and batch edges
(tests/front_sweep_cases.py has the table, the inputs and the referees; tests/test_front_sweep_reference.py checks those
without a GPU).  One parameter per row; inside it every case of the row.  Failures are collected and asserted once.

For every case:
  guarded output  ``out=`` is a view into the middle of a larger buffer: NaN inside, 4096 sentinel words on each side (the
                  in-place plane transform gets such a view as its data).  After the launch no NaN is left where a result is
                  specified and both guards hold their bits.  The inputs sit in buffers of their own with 4096 NaN words on
                  each side; rows of a plane the kernel "does not read" and the cropped-away part of a volume hold NaN.
  accuracy        per sample (sample / plane 1 is 1000x sample 0), max|got - f64| / max(1, max|f64|).  The stages have no
                  project bound: each is held to the library's fp32 form of the same operation on the same inputs on the GPU
                  (torch.fft in complex64, the hipFFT plan, torch.einsum in complex64, slice + add), e <= f e_library + 1e-7
                  with f = 1.5, and the library form itself to LIB_CAP so that no rule lets through more than 3e-6.  The whole
                  front is held to BOUNDS["front"] of tests/test_gpu_v2v_plan_f64.py, and every route asserts which _lib
                  entries it called.
  repeat          a second launch into a second guarded buffer gives the same bits (hand-written kernels).
  batch position  sample / plane 0 of a batch, run alone, gives the same bits: the decode of a block index into (sample, tile).

SP3D_FRONT_SWEEP_RECORD=<file.json>: write every measured error and library ratio, and one summary line per row
(profiles/r18_front_sweep_errors.json).

Worst per-sample error of each row on the MI355X, the case, the library form's error there, and the largest share of its
rule any case of the row uses (e / (1.5 e_library + 1e-7)):
  zdft_fwd_cl         1.41e-7  (2x3 in 4x4, Cout 1, B 2)                        library 1.00e-7   rule used 0.72
  zdft_inv_cl         2.72e-7  (1x33 in 1x33, ReLU, B 2)                        library 1.35e-7   rule used 0.90
  cfft2d_ 88 x 88     1.85e-7  (inverse, rows_in 87, rows_out 3, 3 planes)      library 1.37e-7   rule used 0.61
  cfft2d_88_tiled     1.63e-7  (88x88, 3 planes)                                library 1.44e-7   rule used 0.52
  freq_contract(_ex)  2.76e-7  (I 5, J 8, K 15, F 256, plain)                   library 1.91e-7   rule used 0.71
  freq_contract_ty    2.76e-7  (33 rows, O 5, C 16, SY 20, B 5)                 library 1.57e-7   rule used 0.82
  crop_shift_act_cl   4.95e-8  (ragged, ReLU)                                   library 4.95e-8   rule used 0.28
  unproject_fwd_zdft  1.33e-7  (76x84x20, 5 views)                              library 9.34e-8   rule used 0.56
  whole front         4.31e-7  (76x82x20 B 2, z-DFT with 88 x 88 planes)        bound 1.7e-6
Every row keeps f = 1.5.  A kernel's error is above 1.5x the library's only where both are within a few 1e-7 and the rule's
1e-7 term carries the case (at most 2.0x, zdft_inv_cl: 13 direct cosine terms against the library's C2R).  Every hand-written
kernel repeats its bits and gives sample 0 the bits it has alone; the fused unprojection's spectrum has the bits of the
two-kernel form on all three grids and its cubes are the oracle's exactly.
"""
import collections
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import front_sweep_cases as fs
from tests.test_gpu_v2v_plan_f64 import BOUNDS, conv3d_slabs

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0x5A5A5A5A
CUBE_TOL = 5e-7             # the unprojection's cubes against the reference's: the bound of tests/test_gpu_fused_zdft.py
_names = [r.name for r in fs.ROWS]


class Guarded:
    """``n`` fp32 words inside a larger buffer: NaN, with GUARD sentinel words on each side (``skew`` words further in: a
    result that is 8- but not 16-byte aligned)"""

    def __init__(self, n, dev, skew=0):
        self.buf = torch.empty(n + skew + 2 * GUARD, dtype=torch.float32, device=dev)
        self.bits = self.buf.view(torch.int32)
        self.lo, self.hi = GUARD + skew, GUARD + skew + n
        self.bits[:self.lo] = SENTINEL
        self.bits[self.hi:] = SENTINEL
        self.words = self.buf[self.lo:self.hi]
        self.words.fill_(float("nan"))

    def cl3d(self, B, Cc, X, Y, Z):
        return self.words.view(B, X, Y, Z, Cc).permute(0, 4, 1, 2, 3)

    def cplx(self, shape):
        return torch.view_as_complex(self.words.view(tuple(shape) + (2,)))

    def problems(self, specified):
        p = []
        if not bool((self.bits[:self.lo] == SENTINEL).all()):
            p.append("the guard BEFORE the output was written")
        if not bool((self.bits[self.hi:] == SENTINEL).all()):
            p.append("the guard AFTER the output was written")
        s = torch.view_as_real(specified) if specified.is_complex() else specified
        if bool(torch.isnan(s).any()):
            p.append("a NaN is left where a result is specified")
        return p


def padded(t, dev, cl=False):
    """a CPU tensor on the GPU as a kernel reads it (dense; ``cl``: channels_last_3d), in the middle of a buffer whose GUARD
    words on each side are NaN: a read before or behind the tensor that reaches an output shows as a NaN there"""
    src = t.permute(0, 2, 3, 4, 1).contiguous() if cl else t.contiguous()
    flat = (torch.view_as_real(src) if src.is_complex() else src).reshape(-1)
    buf = torch.full((flat.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + flat.numel()] = flat.to(dev)
    v = buf[GUARD:GUARD + flat.numel()]
    v = torch.view_as_complex(v.view(tuple(src.shape) + (2,))) if src.is_complex() else v.view(src.shape)
    return v.permute(0, 4, 1, 2, 3) if cl else v


def bits_equal(a, b):
    a = torch.view_as_real(a.contiguous()) if a.is_complex() else a.contiguous()
    b = torch.view_as_real(b.contiguous()) if b.is_complex() else b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def numel_words(shape, cplx):
    return int(np.prod(shape)) * (2 if cplx else 1)


# ---- the stage rows: GPU inputs, the guarded launch and the library form of each kind --------------------------------------
def gpu_inputs(case, ins, dev):
    k = case["kind"]
    if k == "zfwd":
        return dict(x=padded(ins["x"], dev, cl=True))
    if k == "zinv":
        return dict(spec=padded(ins["spec"], dev), shift=ins["shift"].to(dev))
    if k in ("f88", "f88_unaligned", "f_other"):
        x = ins["x"].clone()
        x[:, case["rows"][0]:] = complex(float("nan"), float("nan"))        # "not even read"
        return dict(x=padded(x, dev), clean=ins["x"].to(dev))
    if k == "tiled":
        return dict(tiled=padded(fs.tile44(ins["x"]), dev), clean=fs.pad_xy(ins["x"], fs.F88, fs.F88).to(dev))
    if k == "contract":
        return dict(P=padded(ins["P"], dev), Q=padded(ins["Q"], dev))
    if k == "ty":
        return dict(X=padded(ins["X"], dev), T=padded(ins["T"], dev), tw=padded(ins["tw"], dev))
    if k == "ty_plan":
        T, tw = fs.ty_plan_tables(ins["w0"], case["S"])
        return dict(X=padded(ins["X"], dev), T=padded(T, dev), tw=padded(tw, dev),
                    W=fs.plan_spectrum(ins["w0"], case["S"]).to(torch.complex64).to(dev))
    if k == "crop":
        _, X, Y, Zc, _, _, _ = case["dims"]
        src = ins["src"].clone()
        keep = torch.zeros(src.shape[2:], dtype=torch.bool)
        keep[:X, :Y, :Zc] = True
        src[:, :, ~keep] = float("nan")                                       # the cropped-away region
        return dict(src=padded(src, dev), clean=ins["src"].to(dev), shift=ins["shift"].to(dev))
    raise KeyError(k)


def launch(case, gi, dev):
    """one guarded launch -> (Guarded, the returned tensor, the view the entry was given, the specified part of it)"""
    from selfpose3d_amd import _lib
    k = case["kind"]
    if k == "zfwd":
        _, _, SX, SY = case["dims"]
        B = gi["x"].shape[0]
        shape = (B, case["cout"], fs.KZ, SX, SY)
        g = Guarded(numel_words(shape, True), dev)
        out = g.cplx(shape)
        return g, _lib.zdft_fwd_cl(gi["x"], case["cout"], (SX, SY, fs.SZ), out=out), out, out
    if k == "zinv":
        X, Y, _, _ = case["dims"]
        B = gi["spec"].shape[0]
        g = Guarded(B * fs.CH * X * Y * fs.Z, dev)
        out = g.cl3d(B, fs.CH, X, Y, fs.Z)
        return g, _lib.zdft_inv_cl(gi["spec"], X, Y, fs.Z, fs.SZ, gi["shift"], case["relu"], out=out), out, out
    if k in ("f88", "f88_unaligned", "f_other"):
        g = Guarded(numel_words(gi["x"].shape, True), dev, skew=2 if k == "f88_unaligned" else 0)
        data = g.cplx(gi["x"].shape)
        data.copy_(gi["x"])
        if k == "f88_unaligned":                                            # the entry falls back to the library plan
            assert data.data_ptr() % 16 == 8
        y = _lib.cfft2d_(data, case["inverse"], rows_in=case["rows"][0], rows_out=case["rows"][1])
        return g, y, data, data[:, :case["rows"][1]]
    if k == "tiled":
        X, Y = case["xy"]
        shape = (gi["tiled"].shape[0], fs.F88, fs.F88)
        g = Guarded(numel_words(shape, True), dev)
        out = g.cplx(shape)
        return g, _lib.cfft2d_88_tiled(gi["tiled"], X, Y, out=out), out, out
    if k == "contract":
        form = case["form"]
        I = gi["P"].shape[1] if form == "dw" else gi["P"].shape[0]
        shape = (I, case["J"], case["F"])
        g = Guarded(numel_words(shape, True), dev)
        out = g.cplx(shape)
        if form == "plain":
            return g, _lib.freq_contract(gi["P"], gi["Q"], out=out), out, out
        return g, _lib.freq_contract_ex(gi["P"], gi["Q"], form, out=out), out, out
    if k in ("ty", "ty_plan"):
        B, _, K, SX, SY = gi["X"].shape
        shape = (B, gi["T"].shape[1], K, SX, SY)
        g = Guarded(numel_words(shape, True), dev)
        out = g.cplx(shape)
        return g, _lib.freq_contract_ty(gi["X"], gi["T"], gi["tw"], out=out), out, out
    if k == "crop":
        C, X, Y, Zc, _, _, _ = case["dims"]
        B = gi["src"].shape[0]
        g = Guarded(B * C * X * Y * Zc, dev)
        out = g.cl3d(B, C, X, Y, Zc)
        return g, _lib.crop_shift_act_cl(gi["src"], X, Y, Zc, gi["shift"], case["relu"], out=out), out, out
    raise KeyError(k)


def library(case, gi):
    """the library's fp32 form of the same operation on the same GPU inputs"""
    from selfpose3d_amd import _lib
    k = case["kind"]
    if k == "zfwd":
        _, _, SX, SY = case["dims"]
        s = torch.fft.rfft(gi["x"].contiguous(), n=fs.SZ, dim=-1)[:, :case["cout"]]
        return fs.pad_xy(s.permute(0, 1, 4, 2, 3), SX, SY)
    if k == "zinv":
        X, Y, _, _ = case["dims"]
        y = torch.fft.irfft(gi["spec"].permute(0, 1, 3, 4, 2).contiguous(), n=fs.SZ, dim=-1, norm="forward")
        y = y[:, :, :X, :Y, :fs.Z] + gi["shift"].view(1, -1, 1, 1, 1)
        return y.clamp_min(0) if case["relu"] else y
    if k in ("f88", "f88_unaligned"):
        return _lib.cfft2d_(gi["clean"].clone(), case["inverse"], library=True)[:, :case["rows"][1]]
    if k == "f_other":
        return torch.fft.fft2(gi["clean"])
    if k == "tiled":
        return _lib.cfft2d_(gi["clean"].clone(), False, library=True)
    if k == "contract":
        eq = {"plain": "ikf,jkf->ijf", "fwd": "ikf,jkf->ijf", "dx": "ikf,kjf->ijf", "dw": "kif,kjf->ijf"}[case["form"]]
        P = gi["P"].conj() if case["form"] == "dw" else gi["P"]
        Q = gi["Q"].conj() if case["form"] == "fwd" else gi["Q"]
        return torch.einsum(eq, P.resolve_conj(), Q.resolve_conj())
    if k in ("ty", "ty_plan"):
        B, C, K, SX, SY = gi["X"].shape
        W = gi["W"].reshape(-1, C, K * SX, SY) if k == "ty_plan" else fs.ty_weights(gi["T"], gi["tw"], torch.float32)
        return torch.einsum("bcrf,ocrf->borf", gi["X"].reshape(B, C, K * SX, SY), W).reshape(B, -1, K, SX, SY)
    if k == "crop":
        _, X, Y, Zc, _, _, _ = case["dims"]
        y = gi["clean"][:, :, :X, :Y, :Zc] + gi["shift"].view(1, -1, 1, 1, 1)
        return y.clamp_min(0) if case["relu"] else y
    raise KeyError(k)


HAND_WRITTEN = {"zfwd", "zinv", "f88", "tiled", "contract", "ty", "ty_plan", "crop"}       # not the library-plan fallbacks


def guarded_launch(case, gi, dev, tag, failures):
    g, y, out, spec = launch(case, gi, dev)
    if y is not out:
        failures.append((tag, "the entry did not return the tensor it was given"))
    for p in g.problems(spec):
        failures.append((tag, p))
    return g, spec


def sweep_stage_case(row, case, dev, failures, records):
    ins = fs.make_inputs(case)
    k = case["kind"]
    tag = fs.tag_of(case)
    ref = fs.referee(case, ins).to(dev)
    gi = gpu_inputs(case, ins, dev)
    g1, got = guarded_launch(case, gi, dev, tag, failures)
    cmp = fs.compare(got, ref)
    lib = fs.compare(library(case, gi), ref)
    ratio = [e / max(el, 1e-12) for e, el in zip(cmp["err"], lib["err"])]
    rec = dict(row=row.name, case={a: b for a, b in tag}, err=cmp["err"], library=lib["err"], ratio=ratio, range=cmp["range"],
               pos=cmp["pos"], factor=row.factor)
    print(row.name, dict(tag), "err", ["%.3e" % e for e in cmp["err"]], "library", ["%.3e" % e for e in lib["err"]])
    if not fs.has_signal(case, cmp):
        failures.append((tag, "no signal", cmp["pos"], cmp["range"]))
    if not all(el <= fs.LIB_CAP for el in lib["err"]):
        failures.append((tag, "the library form is no yardstick here (error, cap)", lib["err"], fs.LIB_CAP))
    if not fs.within(row.factor, cmp["err"], lib["err"]):
        failures.append((tag, f"over {row.factor} x the library form + 1e-7 (kernel, library)", cmp["err"], lib["err"]))
    if k == "tiled":                                       # the contract tests/test_gpu_fused_zdft.py asserts at 80 x 80
        from selfpose3d_amd import _lib
        same = bits_equal(got, _lib.cfft2d_(gi["clean"].clone(), False, rows_in=case["xy"][0]))
        rec["equals_padded"] = same
        if not same:
            failures.append((tag, "other bits than cfft2d_ of the un-tiled padded planes"))
    if k in HAND_WRITTEN:
        g2, again = guarded_launch(case, gi, dev, tag + ("repeat",), failures)
        rec["repeat_equal"] = bits_equal(got, again)
        if not rec["repeat_equal"]:
            failures.append((tag, "a second launch gave other bits", float((got - again).abs().max())))
        if ref.shape[0] >= 2:
            one = gpu_inputs(case, fs.first_sample(ins, case), dev)
            g3, alone = guarded_launch(case, one, dev, tag + ("alone",), failures)
            rec["alone_equal"] = bits_equal(alone, got[:1])
            if not rec["alone_equal"]:
                failures.append((tag, "sample 0 run alone gave other bits", float((alone - got[:1]).abs().max())))
    records.append(rec)


# ---- the fused unprojection away from 80 x 80 x 20 ------------------------------------------------------------------------
def sweep_unproject_case(row, case, dev, failures, records):
    from selfpose3d_amd import _lib
    tag = fs.tag_of(case)
    u = fs.unproject_inputs(case)
    X, Y, Zc = case["cube"]
    B, V, J = len(case["valid"]), case["V"], fs.UNPROJECT_J
    w, h = fs.UNPROJECT_HM
    n = V * B * h * w * 16
    hbuf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    packed = _lib.pack_heatmaps([x.to(dev) for x in u["hms"]], jp=16, out=hbuf[GUARD:GUARD + n].view(V, B, h, w, 16))
    views = [packed[c] for c in range(V)]
    cam, cen, val = (torch.from_numpy(u[a]).to(dev) for a in ("cam", "centers", "valid"))
    args = (B, 16, h, w, case["cube"], u["grid_size"], fs.UNPROJECT_IMG)
    cubes, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, 16, cam, cen, val, *args, False, channels_last=True)
    S = (fs.F88, fs.F88, fs.SZ)
    two = _lib.zdft_fwd_cl(cubes, J, S)[..., :X, :Y]

    def fused(views, cam, cen, val, B, t):
        shape = (B, J, fs.KZ, X // 4, Y // 4, 16)
        g = Guarded(numel_words(shape, True), dev)
        out = g.cplx(shape)
        y = _lib.unproject_fwd_zdft(views, 16, cam, cen, val, B, J, h, w, case["cube"], u["grid_size"], fs.UNPROJECT_IMG, fs.SZ,
                                    out=out)
        if y is not out:
            failures.append((t, "the entry did not return the tensor it was given"))
        for p in g.problems(out):
            failures.append((t, p))
        return g, out
    g1, one = fused(views, cam, cen, val, B, tag)
    if not bits_equal(fs.untile44(one, X, Y), two):
        failures.append((tag, "other bits than unproject_fwd(channels_last) -> zdft_fwd_cl"))
    for b, v in enumerate(case["valid"]):
        if not v and int(torch.count_nonzero(torch.view_as_real(one[b]))):
            failures.append((tag, "the invalid sample's spectrum is not all zero", b))
    dc = float((cubes[:, :J].cpu() - u["cubes"]).abs().max())
    if not dc <= CUBE_TOL or int(torch.count_nonzero(cubes[:, J:])):
        failures.append((tag, "the cubes behind it are not the oracle's", dc))
    # the z-DFT stage: float64 on the very cubes the library form transforms
    ref = fs.ref_unproject_spectrum(cubes.double(), J)
    cmp = fs.compare(fs.untile44(one, X, Y), ref)
    lib = fs.compare(torch.fft.rfft(cubes[:, :J].contiguous(), n=fs.SZ, dim=-1).permute(0, 1, 4, 2, 3), ref)
    if not fs.within(row.factor, cmp["err"], lib["err"]) or not all(el <= fs.LIB_CAP for el in lib["err"]):
        failures.append((tag, f"over {row.factor} x the library form + 1e-7 (kernel, library)", cmp["err"], lib["err"]))
    if not all((r > 1.0) == bool(v) for r, v in zip(cmp["range"], case["valid"])):
        failures.append((tag, "no signal", cmp["range"]))
    g2, again = fused(views, cam, cen, val, B, tag + ("repeat",))
    g3, alone = fused([v[:1] for v in views], cam[:1], cen[:1], val[:1], 1, tag + ("alone",))
    rec = dict(row=row.name, case={a: b for a, b in tag}, err=cmp["err"], library=lib["err"],
               ratio=[e / max(el, 1e-12) for e, el in zip(cmp["err"], lib["err"])], range=cmp["range"], cubes_vs_oracle=dc,
               factor=row.factor, repeat_equal=bits_equal(one, again), alone_equal=bits_equal(alone, one[:1]))
    print(row.name, dict(tag), "err", ["%.3e" % e for e in cmp["err"]], "library", ["%.3e" % e for e in lib["err"]], "cubes", dc)
    if not rec["repeat_equal"]:
        failures.append((tag, "a second launch gave other bits"))
    if not rec["alone_equal"]:
        failures.append((tag, "sample 0 run alone gave other bits"))
    records.append(rec)


# ---- the whole front ------------------------------------------------------------------------------------------------------
SPIED = ("zdft_fwd_cl", "zdft_inv_cl", "cfft2d_", "cfft2d_88_tiled", "freq_contract", "freq_contract_ty", "rfft3d", "irfft3d_",
         "crop_shift_act_cl", "channel_shift_act_")


_front_refs = {}


def sweep_front_case(row, case, dev, failures, records, monkeypatch):
    from selfpose3d_amd import _lib
    from selfpose3d_amd.v2v_net import TiledZSpectrum
    tag = fs.tag_of(case)
    net = fs.front_net(case["cin"], True).to(dev)
    net.contract_ty = case["ty"]
    plan = net._get_plan()
    plan._ensure_built()
    w0, s0 = plan.layers["front"][:2]
    ins = fs.make_inputs(case)
    x = padded(ins["x"], dev, cl=case["cl"])
    X, Y, Zc = case["grid"]
    key = (case["cin"], case["fc"], case["grid"], case["B"])                 # routes on one grid share inputs, net and referee
    if key not in _front_refs:
        _front_refs.clear()
        _front_refs[key] = fs.ref_front(x, w0, s0, conv=lambda xd, wd: conv3d_slabs(xd, wd, None))
    ref = _front_refs[key]
    if case["route"].startswith("zspectrum"):
        spec = fs.tile44(_lib.zdft_fwd_cl(x, case["cin"], (X, Y, fs.SZ)))
        feed = TiledZSpectrum(padded(spec.cpu(), dev), X, Y, Zc, fs.SZ)
    called = collections.Counter()
    with monkeypatch.context() as mp:
        for name in SPIED:
            def spy(*a, _n=name, _f=getattr(_lib, name), **kw):
                called[_n] += 1
                return _f(*a, **kw)
            mp.setattr(_lib, name, spy)
        with torch.no_grad():
            if case["route"].startswith("zspectrum"):
                got = plan._front_zspectrum(feed, w0, s0)
            else:
                got = plan._front_fft(x, w0, s0)
    torch.cuda.synchronize(dev)
    if any(called[n] == 0 for n in case["calls"]) or any(called[n] for n in case["never"]):
        failures.append((tag, "the route called other entries than it is named for", dict(called)))
    if tuple(got.shape) != tuple(ref.shape):
        failures.append((tag, "shape", tuple(got.shape)))
        return
    cmp = fs.compare(got, ref)
    print(row.name, dict(tag), "err", ["%.3e" % e for e in cmp["err"]], "pos", ["%.2f" % p for p in cmp["pos"]], dict(called))
    if not fs.has_signal(case, cmp):
        failures.append((tag, "share of positive outputs", cmp["pos"]))
    if not all(e <= BOUNDS["front"] for e in cmp["err"]):
        failures.append((tag, "over BOUNDS['front'] (per sample)", cmp["err"], BOUNDS["front"]))
    records.append(dict(row=row.name, case={a: b for a, b in tag}, err=cmp["err"], range=cmp["range"], pos=cmp["pos"],
                        bound=BOUNDS["front"], called=dict(called)))


def summary_of(row, records):
    """the row's line of the error file: the worst per-sample error, its case and its ratio to the library form there; how
    much of the rule the row uses at most (e / (f e_library + 1e-7)); and whether every repeat and every lone sample agreed"""
    worst = max(records, key=lambda r: max(r["err"]))
    i = max(range(len(worst["err"])), key=lambda j: worst["err"][j])
    out = dict(row=row.name, summary=True, cases=len(records), worst_err=worst["err"][i], worst_case=worst["case"], sample=i,
               factor=row.factor, repeat_equal=all(r.get("repeat_equal", True) for r in records),
               alone_equal=all(r.get("alone_equal", True) for r in records))
    if "library" in worst:
        out["library_at_worst"] = worst["library"][i]
        out["ratio_at_worst"] = worst["err"][i] / max(worst["library"][i], 1e-12)
        out["rule_used"] = max(e / (row.factor * el + 1e-7) for r in records for e, el in zip(r["err"], r["library"]))
    else:
        out["bound"] = worst["bound"]
    return out


def write_records(records):
    path = os.environ.get("SP3D_FRONT_SWEEP_RECORD")
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


@pytest.mark.parametrize("name", _names)
def test_front_sweep(name, monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    monkeypatch.delenv("SP3D_CONTRACT_TY", raising=False)
    row = fs.ROW[name]
    failures, records = [], []
    t0 = time.perf_counter()
    for case in fs.cases(row):
        if case["kind"] == "unproject":
            sweep_unproject_case(row, case, dev, failures, records)
        elif case["kind"] == "front":
            sweep_front_case(row, case, dev, failures, records, monkeypatch)
        else:
            sweep_stage_case(row, case, dev, failures, records)
    torch.cuda.synchronize(dev)
    summary = summary_of(row, records)
    print(f"front sweep {name}: {len(records)} cases in {time.perf_counter() - t0:.1f} s, {summary}")
    write_records(records + [summary])
    torch.cuda.empty_cache()
    assert not failures, report(failures)


def test_shapes_the_kernels_cannot_serve_are_refused():
    from selfpose3d_amd import _lib
    dev = torch.device("cuda:0")
    for X, Y in ((6, 8), (92, 8), (8, 6)):
        with pytest.raises(_lib.Sp3dError):
            _lib.cfft2d_88_tiled(torch.zeros((1, X // 4, Y // 4, 16), dtype=torch.complex64, device=dev), X, Y)
    for C, SY in ((17, 8), (4, 97)):
        Xf = torch.zeros((1, C, 1, 4, SY), dtype=torch.complex64, device=dev)
        with pytest.raises(_lib.Sp3dError):
            _lib.freq_contract_ty(Xf, torch.zeros((4, 4, C, 14), device=dev), torch.zeros((SY, 3, 2), device=dev))


def test_out_is_checked_before_any_launch():
    """``out`` of another shape, type, layout, alignment or device is refused by the entries that take it"""
    from selfpose3d_amd import _lib
    dev = torch.device("cuda:0")
    case = dict(kind="zinv", dims=(3, 17, 3, 17), relu=True, B=1)
    gi = gpu_inputs(case, fs.make_inputs(case), dev)
    good = torch.empty((1, 3, 17, fs.Z, fs.CH), device=dev).permute(0, 4, 1, 2, 3)
    assert _lib.zdft_inv_cl(gi["spec"], 3, 17, fs.Z, fs.SZ, gi["shift"], True, out=good) is good
    skew = torch.empty(3 * 17 * fs.Z * fs.CH + 4, device=dev)[1:-3].view(1, 3, 17, fs.Z, fs.CH).permute(0, 4, 1, 2, 3)
    for out in (torch.empty((1, 3, 18, fs.Z, fs.CH), device=dev).permute(0, 4, 1, 2, 3), torch.empty((1, fs.CH, 3, 17, fs.Z), device=dev),
                good.double(), good.cpu(), skew):
        with pytest.raises(_lib.Sp3dError):
            _lib.zdft_inv_cl(gi["spec"], 3, 17, fs.Z, fs.SZ, gi["shift"], True, out=out)
    case = dict(kind="contract", I=2, J=9, K=3, F=257, form="fwd")
    gi = gpu_inputs(case, fs.make_inputs(case), dev)
    good = torch.empty((2, 9, 257), dtype=torch.complex64, device=dev)
    assert _lib.freq_contract_ex(gi["P"], gi["Q"], "fwd", out=good) is good and _lib.freq_contract(gi["P"], gi["Q"], out=good) is good
    for out in (torch.empty((2, 9, 256), dtype=torch.complex64, device=dev), good.to(torch.complex128), good.cpu(),
                torch.empty((2, 9, 514), dtype=torch.complex64, device=dev)[:, :, ::2]):
        with pytest.raises(_lib.Sp3dError):
            _lib.freq_contract_ex(gi["P"], gi["Q"], "fwd", out=out)
        with pytest.raises(_lib.Sp3dError):
            _lib.freq_contract(gi["P"], gi["Q"], out=out)
