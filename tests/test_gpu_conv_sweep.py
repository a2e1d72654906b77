"""Every conv and up-conv kernel of the V2V inference plan against float64 at block, batch and walk boundaries
(tests/conv_sweep_cases.py has the table, the grids, the inputs and the referee; tests/test_conv_sweep_reference.py checks
those without a GPU).  One parameter per (row, width); inside it every grid class, every epilogue mode, and for the two
conv3_split_ rows the walk grids computed from this device's CU count, on which persistent workgroups walk two and three
blocks, unevenly, across the sample boundary.  Failures are collected and asserted once per parameter.

For every case:
  guarded output  ``out=`` is a view into the middle of a larger buffer: NaN inside, 4096 sentinel words on each side.  After
                  the launch no NaN is left (no input is non-finite) and both guards hold their bits.  The activations sit
                  in buffers of their own with 4096 NaN on each side: a read outside them that reaches an output shows.
  accuracy        per sample (sample 1 is 1000x sample 0: a halo read across the sample boundary swamps sample 0),
                  max|got - f64| / max(1, max|f64|) against the project's own bound: BOUNDS of test_gpu_v2v_plan_f64.py,
                  2.0e-6 for conv3_split128_; the O = 32 Winograd kernels e <= 1.5 e_three + 1e-7 against the three-launch
                  form on the same inputs (absolute errors: the rule of test_gpu_parity.py); the fused up-conv forms the
                  bound and at most 1.5x the GEMM + scatter form (the rule of test_gpu_upconv_fused.py).
  signal          10-90 % positive outputs in the ReLU modes on grids of at least one block.
  repeat          a second launch into a second guarded buffer gives the same bits (not the library-GEMM forms).
  batch position  sample 0 of a batch of two, run alone: the same bits from the one-kernel entries - on the walk grids this
                  pins the decode of a block index into (sample, bx, by, bz) without a tolerance; the library-GEMM forms
                  (their GEMM may pick another kernel for another row count) within the bound.

A case over its bound is measured against the library's fp32 F.conv3d on the same inputs (recorded as lib_fp32); only a case
listed in FLAGGED, with the reason, may then carry 1.5x that error.

SP3D_CONV_SWEEP_RECORD=<file.json>: write every measured error (profiles/r16_conv_sweep_errors.json).

Worst per-sample error of each row on the MI355X (256 CUs) next to its bound, every width, grid class and mode:
  conv3_split_                          1.36e-6  (32 -> 32, two rounds of blocks, ragged, mode 0)        bound 4.7e-6
  conv3_split_ + xs / skip_w            1.24e-6  (35x17x9)                                               bound 4.7e-6
  wino_fused_conv3d_ fp32               4.38e-7  (32 -> 32, 24x24x12, mode 0)    at most 0.97 of 1.5 e_three + 1e-7
  wino_fused_conv3d_ + U3 chunk 8       4.04e-7  (16 -> 32, 1x2x3, mode 1)       at most 0.93 of 1.5 e_three + 1e-7
  wino_fused_conv3d_ + U3 chunk 16      3.81e-7  (32 -> 64, 8x8x2, mode 1)                               bound 2.3e-6
  the same + xs / skip_w                3.97e-7  (8x8x2)                                                 bound 2.3e-6
  conv3_split128_                       8.61e-7  (128 -> 128, 15x15x15, mode 0)                          bound 2.0e-6
  wino_conv3d_ three launches           1.23e-6  (8 -> 4, 1x1x1, mode 2)                                 bound 2.0e-6
  upsample2x_ GEMM + scatter / fused    5.31e-7 / 4.79e-7  (fused at most 1.41x GEMM + scatter)          bound 1.5e-6
  upsample2x_head_ GEMM + scatter / fused  3.05e-7 / 3.10e-7  (fused at most 1.43x GEMM + scatter)       bound 9.0e-7
No case is over its bound: FLAGGED is empty.  Every one-kernel entry repeats its bits and gives sample 0 the bits it has
alone; of the library-GEMM forms only the GEMM + scatter head differs between the batch and the sample alone (6 cases,
inside the bound)."""
import collections
import json
import os
import time

import pytest
import torch
import torch.nn.functional as F

from tests import conv_sweep_cases as sw

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = 0x5A5A5A5A
FLAGGED = {}            # (row, width, class, mode) -> why this case carries 1.5x the library's fp32 error instead of its bound

ROW_WIDTHS = [(r.name, w) for r in sw.ROWS for w in r.widths]
_ids = [f"{n}-{'x'.join(str(v) for v in w)}" for n, w in ROW_WIDTHS]
CL = torch.channels_last_3d


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    monkeypatch.delenv("SP3D_FUSE_UPCONV", raising=False)


class Guarded:
    """a (B,C,X,Y,Z) channels_last_3d fp32 result inside a larger buffer: NaN, with GUARD sentinel words on each side"""

    def __init__(self, shape, dev):
        B, Cc, X, Y, Z = shape
        n = B * Cc * X * Y * Z
        self.buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=dev)
        self.bits = self.buf.view(torch.int32)
        self.bits[:GUARD] = SENTINEL
        self.bits[GUARD + n:] = SENTINEL
        self.buf[GUARD:GUARD + n] = float("nan")
        self.n = n
        self.out = self.buf[GUARD:GUARD + n].view(B, X, Y, Z, Cc).permute(0, 4, 1, 2, 3)

    def problems(self):
        p = []
        if not bool((self.bits[:GUARD] == SENTINEL).all()):
            p.append("the guard BEFORE the output was written")
        if not bool((self.bits[GUARD + self.n:] == SENTINEL).all()):
            p.append("the guard AFTER the output was written")
        if bool(torch.isnan(self.out).any()):
            p.append("an output was never written (NaN left)")
        return p


def padded(t, dev):
    """an activation on the GPU as the kernels read it (channels_last_3d), in the middle of a buffer whose GUARD words on each
    side are NaN: a read a few rows before or behind the tensor that reaches an output shows as a NaN there"""
    B, Cc, X, Y, Z = t.shape
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + n] = t.permute(0, 2, 3, 4, 1).reshape(-1).to(dev)
    return buf[GUARD:GUARD + n].view(B, X, Y, Z, Cc).permute(0, 4, 1, 2, 3)


def records_of(row, weights):
    """what the entry reads behind its weight pointers, on the GPU, once per (row, width)"""
    from selfpose3d_amd import _lib
    w = {k: v.cuda() for k, v in weights.items()}
    if row.block is None:
        Cin, O = w["wT"].shape[:2]
        w["wg"] = w["wT"].permute(0, 2, 3, 4, 1).reshape(Cin, 8 * O).contiguous()      # columns (i,j,k,o): _FoldedV2V._build
        w["w3"] = _lib.upconv_weights_split(w["wg"])
        return w
    O = w["w"].shape[0]
    if row.entry == "conv3_split_":
        w["W3"] = _lib.conv_weights_split(w["w"])
        if "ws" in w:
            w["S"] = _lib.conv_weights_split(w["ws"])
    elif row.entry == "conv3_split128_":
        w["W3"] = _lib.conv_weights_split24(w["w"])
    w["U"] = _lib.wino_weights(w["w"])                      # also the three-launch form the O = 32 Winograd rows are held to
    if row.kw.get("chunk"):
        w["U3"] = _lib.wino_weights_split(w["U"], row.kw["chunk"])
        if "ws" in w:
            CS = w["ws"].shape[1]
            w["S"] = _lib.wino_weights_split(w["ws"].reshape(O, CS).t().reshape(1, CS, O).contiguous(), 16)
    return w


def launch(row, w, gi, mode, out, form=None):
    """the row's entry on GPU inputs ``gi``, into ``out``; form: None | "fused" | "gemm" | "three" (the three-launch referee)"""
    from selfpose3d_amd import _lib
    x = gi["x"]
    if row.block is None:
        w3 = w["w3"] if form == "fused" else None
        if "wo" in w:
            return _lib.upsample2x_head_(x, w["wg"], w["shift"], gi["res"], w["wo"], w["bo"], w_split=w3, out=out)
        return _lib.upsample2x_(x, w["wg"], w["shift"], gi["res"], w_split=w3, out=out)
    r = gi["res"] if mode >= 2 else None
    if form == "three" or row.entry == "wino_conv3d_":
        return _lib.wino_conv3d_(x, w["U"], w["shift"], mode, r, out=out)
    skip = dict(xs=gi["xs"], skip_w=w["S"]) if row.kw.get("skip") else {}
    if row.entry == "conv3_split_":
        return _lib.conv3_split_(x, w["W3"], w["shift"], mode, r, out=out, **skip)
    if row.entry == "conv3_split128_":
        return _lib.conv3_split128_(x, w["W3"], w["shift"], mode, r, out=out)
    return _lib.wino_fused_conv3d_(x, w["U"], w["shift"], mode, r, w.get("U3"), out=out, **skip)


def library_fp32(row, w, gi, mode):
    """the same layer through the library's fp32 convolution: the yardstick of a case over its bound"""
    f32 = {k: v for k, v in w.items() if k in ("w", "ws", "wT", "shift", "wo", "bo")}
    if row.block is None:
        core = F.conv_transpose3d(gi["x"], w["wT"], None, 2)
    else:
        core = F.conv3d(gi["x"], w["w"], padding=1)
        if "ws" in w:
            core = core + F.conv3d(gi["xs"], w["ws"])
    O = core.shape[1]
    y = core + w["shift"].view(1, O, 1, 1, 1)
    if row.block is None:
        y = y.clamp_min(0) + gi["res"]
        return F.conv3d(y, f32["wo"], f32["bo"]) if "wo" in f32 else y
    if mode == 2:
        y = y + gi["res"]
    if mode >= 1:
        y = y.clamp_min(0)
    if mode == 3:
        y = y + gi["res"]
    return y


def guarded_launch(row, w, gi, mode, shape, form, tag, failures):
    g = Guarded(shape, gi["x"].device)
    y = launch(row, w, gi, mode, g.out, form)
    if y is not g.out:
        failures.append((tag, "the entry did not return out"))
    for p in g.problems():
        failures.append((tag, p))
    return g


def write_records(records):
    path = os.environ.get("SP3D_CONV_SWEEP_RECORD")
    if not path:
        return
    old = []
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in old + records) + "\n]\n")


def report(failures):
    """every failed check of a parameter, the kinds counted first (pytest cuts the repr of a long list short)"""
    kinds = collections.Counter(f[1] for f in failures)
    lines = [f"{len(failures)} failed checks: " + "; ".join(f"{n} x {k}" for k, n in kinds.items())]
    return "\n".join(lines + [repr(f) for f in failures[:60]])


def sweep_case(row, width, w, weights_gpu, cname, B, grid, dev, failures, records):
    ins = sw.make_inputs(row, width, B, grid)
    gi = {k: padded(v, dev) for k, v in ins.items()}
    one = {k: padded(v[:1], dev) for k, v in ins.items()} if B == 2 else None      # sample 1 is not behind it any more
    core = sw.referee_core(row, weights_gpu, gi)
    up = 2 if row.block is None else 1
    Cout = width[2] if len(width) == 3 else width[1]
    shape = (B, Cout, up * grid[0], up * grid[1], up * grid[2])
    forms = ("gemm", "fused") if row.rule == "gemm" else (None,)
    for mode in row.modes:
        ref = sw.epilogue(row, weights_gpu, gi, core, mode)
        assert tuple(ref.shape) == shape
        e_other = None                                            # the form a relative rule compares with, per sample
        if row.rule == "three_launch":
            e_other = sw.compare(launch(row, w, gi, mode, None, "three"), ref)["abs"]
        for form in forms:
            tag = (row.name, width, cname, B, grid, mode, form)
            library = bool(row.kw.get("library_gemm")) or form == "gemm"
            g1 = guarded_launch(row, w, gi, mode, shape, form, tag, failures)
            cmp = sw.compare(g1.out, ref)
            rec = dict(row=row.name, width=list(width), cls=cname, B=B, grid=list(grid), mode=mode, form=form, err=cmp["err"],
                       range=cmp["range"], pos=cmp["pos"], bound=row.bound)
            print(tag, "err", ["%.3e" % e for e in cmp["err"]], "pos", ["%.2f" % p for p in cmp["pos"]])
            if not sw.has_signal(row, mode, B, grid, cmp):
                failures.append((tag, "share of positive outputs", cmp["pos"]))
            # ---- accuracy, per sample
            over = []
            if row.rule == "three_launch":
                rec["abs"], rec["three_launch_abs"] = cmp["abs"], e_other
                over = [(b, e, 1.5 * e3 + 1e-7) for b, (e, e3) in enumerate(zip(cmp["abs"], e_other)) if not e <= 1.5 * e3 + 1e-7]
            else:
                over = [(b, e, row.bound) for b, e in enumerate(cmp["err"]) if not e <= row.bound]
                if form == "gemm":
                    e_other = cmp["err"]
                elif form == "fused":
                    rec["gemm_scatter"] = e_other
                    over += [(b, e, 1.5 * eg) for b, (e, eg) in enumerate(zip(cmp["err"], e_other)) if not e <= 1.5 * eg]
            if over:
                e32 = sw.compare(library_fp32(row, w, gi, mode), ref)
                rec["lib_fp32"] = e32["err"]
                key = (row.name, tuple(width), cname, mode)
                if key in FLAGGED and all(e <= 1.5 * e32["err"][b] for b, e, _ in over):
                    rec["flagged"] = FLAGGED[key]
                else:
                    failures.append((tag, "over its bound (sample, error, bound)", over, "library fp32", e32["err"]))
            # ---- repeat: the same bits from a second launch
            g2 = guarded_launch(row, w, gi, mode, shape, form, tag + ("repeat",), failures)
            same = torch.equal(g1.out, g2.out)
            rec["repeat_equal"] = same
            if not same and not library:
                failures.append((tag, "a second launch gave other bits", float((g1.out - g2.out).abs().max())))
            # ---- batch position: sample 0 alone
            if one is not None:
                g3 = guarded_launch(row, w, one, mode, (1,) + shape[1:], form, tag + ("alone",), failures)
                same = torch.equal(g3.out, g1.out[:1])
                rec["alone_equal"] = same
                if not same:
                    if not library:
                        failures.append((tag, "sample 0 run alone gave other bits", float((g3.out - g1.out[:1]).abs().max())))
                    else:
                        ea = sw.compare(g3.out, ref[:1])["err"][0]
                        rec["alone_err"] = ea
                        if not ea <= row.bound:
                            failures.append((tag, "sample 0 run alone over its bound", ea, row.bound))
            records.append(rec)
            del g1, g2
        del ref
    del core


@pytest.mark.parametrize("name,width", ROW_WIDTHS, ids=_ids)
def test_conv_sweep(name, width):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    row = sw.ROW[name]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    weights = sw.make_weights(row, width)
    w = records_of(row, weights)
    weights_gpu = {k: v.to(dev) for k, v in weights.items()}
    failures, records = [], []
    t0 = time.perf_counter()
    for cname, B, grid in sw.cases(row, cus):
        if "rounds" in cname:
            rounds, nwg = sw.launch_of(sw.block_count(B, grid, row.block), cus)
            assert rounds == (2 if cname.startswith("two") else 3) and nwg <= cus, (cname, rounds, nwg, cus)
        sweep_case(row, width, w, weights_gpu, cname, B, grid, dev, failures, records)
    torch.cuda.synchronize(dev)
    print(f"conv sweep {name} {width}: {len(records)} measurements on {cus} CUs in {time.perf_counter() - t0:.1f} s, "
          f"worst {max(max(r['err']) for r in records):.3e}")
    write_records(records)
    torch.cuda.empty_cache()
    assert not failures, report(failures)


def test_out_is_checked_before_any_launch():
    """``out`` of another shape, type, layout or device is refused by every entry that takes it"""
    from selfpose3d_amd import _lib
    dev = torch.device("cuda:0")
    for name, width in (("conv3_split", (16, 32)), ("wino_fused_split16", (32, 64)), ("conv3_split128", (64, 128)),
                        ("wino_three_launch", (8, 4)), ("upsample2x", (128, 64)), ("upsample2x_head", (64, 32, 15))):
        row = sw.ROW[name]
        w = records_of(row, sw.make_weights(row, width))
        grid = (3, 2, 2)
        gi = {k: v.to(dev).contiguous(memory_format=CL) for k, v in sw.make_inputs(row, width, 1, grid).items()}
        up = 2 if row.block is None else 1
        Cout = width[2] if len(width) == 3 else width[1]
        shape = (1, Cout, up * 3, up * 2, up * 2)
        form = "fused" if row.block is None else None
        mode = row.modes[0] if row.block is None else 1
        good = torch.empty(shape, device=dev).contiguous(memory_format=CL)
        assert launch(row, w, gi, mode, good, form) is good
        bad = [torch.empty((1, Cout, up * 3, up * 2, up * 2 + 1), device=dev).contiguous(memory_format=CL),      # another grid
               torch.empty((1, Cout + 1) + shape[2:], device=dev).contiguous(memory_format=CL),                  # another width
               torch.empty(shape, device=dev, dtype=torch.float64).contiguous(memory_format=CL),                 # another type
               torch.empty(shape).contiguous(memory_format=CL)]                                                  # another device
        if Cout > 1:
            bad.append(torch.empty(shape, device=dev))                                                           # planar
        for out in bad:
            with pytest.raises(_lib.Sp3dError):
                launch(row, w, gi, mode, out, form)
