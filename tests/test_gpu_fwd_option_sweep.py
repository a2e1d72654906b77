"""Forward unprojection (sp3d_unproject_fwd_indexed / _strided / _variant, through the C ABI) at ragged shapes in every result
layout, storage type and indexing production uses, bit for bit against the CPU oracle.  tests/fwd_option_sweep_cases.py has the
cases, the options of a case, what the library must answer to each (return code, kernels, store path) and the referee;
tests/test_fwd_option_sweep_reference.py proves that table without a GPU.  One parameter per case; inside it every option of
the case.  Failures are collected and asserted once.

For every pair the library accepts:
  guarded result   the result is a view into a larger buffer filled with a sentinel - a slab between 4096 sentinel elements
                   (dense, channels-last) or the corner of a padded block (strided: the padding is the guard).  Afterwards
                   every addressed element equals the referee (torch.equal: no tolerance) and every other element holds the
                   sentinel's bits.  Skipped cubes and the pad channels of a channels-last result are zeros in the referee.
  guarded inputs   the heat-maps of every view, the camera table and the centres lie between 4096 NaN words, so a tap or a
                   record read out of range poisons the result; ``valid`` and ``sample_of`` lie between 4096 zero words (an
                   index read from a guard becomes an address: it must stay a harmless one).
  grids            where asked for, in a sentinel-filled guarded buffer of their own: equal to the oracle's, no sentinel left
                   (at Jp = 32 only the first of the two launches may write them), zeros for a skipped cube.
  repeat           no atomics in these kernels: a second launch into a fresh buffer leaves the same bits in the whole buffer.
For every pair the library refuses: exactly the code the table names, result and grids still all sentinel.

The same inputs go through the planar-input kernel (LAYOUT_PLANAR; jc = 1 / 4 / 16) as options of their own, which puts
valid[0] == 0, sample_of and more than 4 cubes through it.

On the MI355X: 36 cases, 1677 pairs, 1062 accepted and bit-equal, 615 refused with their code, 2.5 s for the file.

A wrong library built on a scratch copy and run once (not committed; three changes, each leaving every store in bounds), and
what caught it - 21 of the 36 cases failed:
  out_off of the second channel group dropped (resolve_fwd)            every Jp = 32 case with a second launch (28 .. 35): all 40
                                                                       accepted pairs of a case "differ from the oracle";
  ``nvox == 64`` dropped from the pipe kernel's 16-byte store path      the cases with N % 4 == 0 and a last tile below 64 (05, 07,
                                                                       14 .. 19, 33): "an element outside the result was written",
                                                                       cubes differ, and two launches disagree (the stale LDS
                                                                       words of the ragged tile race with their neighbours');
  the dense channel stride g.N in the 16-byte store of the brick       the strided_aligned results of the Z = 32 / 64 cases
  stacks (unproject_brick_kernel only)                                 below Jp = 32 (08, 09, 25 .. 27), fp32 maps only.
Flipping ``(g.Z & 3) == 0`` in the brick stacks' store changes nothing a default request can see: the plan sends only Z % 32 == 0
to the stacks, where both store paths are right; the scalar path at other Z is reached by the tuning words alone, which
tests/test_gpu_random_sweep.py runs (word 56) at ragged Z.
"""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import fwd_option_sweep_cases as fs

pytestmark = pytest.mark.gpu

GUARD = fs.GUARD
SENTINEL = {4: 0x5A5A5A5A, 2: 0x5A5A}


def padded(t, dev, dtype=None, fill=float("nan")):
    """a tensor on the GPU between GUARD elements of ``fill`` on each side"""
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    dtype = dtype or t.dtype
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = t.reshape(-1).to(dev, dtype)
    return buf[GUARD:GUARD + n].view(t.shape)


class Guarded:
    """a strided (``shape``, ``strides``, ``offset`` in elements) result inside a flat buffer of ``total`` elements, every
    element of the buffer pre-filled with the sentinel"""

    def __init__(self, shape, strides, offset, total, dtype, dev):
        self.flat = torch.empty(total, dtype=dtype, device=dev)
        size = self.flat.element_size()
        self.sentinel = SENTINEL[size]
        self.bits = self.flat.view(torch.int32 if size == 4 else torch.int16)
        self.bits.fill_(self.sentinel)
        self.geometry = (tuple(shape), tuple(strides), offset)
        self.view = torch.as_strided(self.flat, *self.geometry)
        self.ptr = self.flat.data_ptr() + offset * size
        assert self.flat.data_ptr() % 16 == 0

    def all_sentinel(self):
        return bool((self.bits == self.sentinel).all())

    def outside_untouched(self):
        rest = self.bits.clone()
        torch.as_strided(rest, *self.geometry).fill_(self.sentinel)
        return bool((rest == self.sentinel).all())


def result_buffer(case, o, dev):
    lay = fs.result_layout(o["form"], case.P, o["Jc"], case.cube, o["out_bf16"])
    return Guarded((case.P, o["Jc"]) + tuple(case.cube), lay["strides"], lay["offset"], lay["total"],
                   torch.bfloat16 if o["out_bf16"] else torch.float32, dev), lay


def grids_buffer(case, dev):
    n = case.P * case.N * 3
    return Guarded((case.P, case.N, 3), (case.N * 3, 3, 1), GUARD, n + 2 * GUARD, torch.float32, dev)


class Device:
    """the inputs of a case on the GPU, every one between guards, and its references"""

    def __init__(self, case, dev):
        from selfpose3d_amd import _lib
        self.case, self.dev = case, dev
        self.planar = [padded(x, dev) for x in case.hms]
        self.packed = {}
        for in_bf16 in ((False, True) if case.jp >= 16 else (False,)):
            src = [torch.from_numpy(x).to(dev, torch.bfloat16 if in_bf16 else torch.float32) for x in (case.hms_bf16 if in_bf16 else case.hms)]
            pk = _lib.pack_heatmaps(src, jp=case.jp, out_dtype=torch.bfloat16 if in_bf16 else torch.float32)
            self.packed[in_bf16] = [padded(pk[c], dev) for c in range(case.V)]
        self.cam = padded(case.cam, dev)
        self.centers = padded(case.centers, dev)
        self.valid = padded(case.valid, dev, fill=0)
        self.sample_of = {m: (None if so is None else padded(so, dev, fill=0)) for m, so in case.sample_of.items()}
        self.gs = _lib._f3(case.grid_size)
        self.refs = {}

    def reference(self, o):
        key = (o["mode"], o["in_bf16"], o["out_bf16"], o["Jc"])
        if key not in self.refs:
            cubes, grids = self.case.reference(o)
            self.refs[key] = (torch.from_numpy(cubes).to(self.dev, torch.bfloat16 if o["out_bf16"] else torch.float32),
                              torch.from_numpy(grids).to(self.dev))
        return self.refs[key]

    def launch(self, o, res, lay, grids):
        """one request through the C ABI -> return code"""
        from selfpose3d_amd import _lib
        lib, case = _lib.load(), self.case
        X, Y, Z = case.cube
        if o["layout"] == "planar":
            views, layout, jp = self.planar, _lib.LAYOUT_PLANAR, case.J
        else:   # a refused request reads nothing: the fp32 views stand in where no bf16 ones exist
            views, layout, jp = self.packed.get(o["in_bf16"], self.packed[False]), _lib.LAYOUT_NHWC, case.jp
        flags = (_lib.HM_BF16 if o["in_bf16"] else 0) | (_lib.OUT_BF16 if o["out_bf16"] else 0) | (_lib.OUT_CHANNELS_LAST if o["form"] == "cl" else 0)
        so = self.sample_of[o["mode"]]
        shape = (case.P, case.V, o["Jc"], case.h, case.w, X, Y, Z, self.gs, case.img[0], case.img[1], _lib._stream(self.dev))
        gp = None if grids is None else grids.ptr
        if o["entry"] == "variant":
            assert so is None
            return lib.sp3d_unproject_fwd_variant(_lib._ptr_array(views), jp, self.cam.data_ptr(), self.centers.data_ptr(), self.valid.data_ptr(),
                                                  res.ptr, gp, *shape[:-1], o["word"] | (1 << 24), shape[-1])
        if o["entry"] == "strided":
            st = (C.c_int64 * 4)(*lay["strides"][:4])
            return lib.sp3d_unproject_fwd_strided(_lib._ptr_array(views), layout | flags, jp, self.cam.data_ptr(), _lib._opt(so),
                                                  self.centers.data_ptr(), self.valid.data_ptr(), res.ptr, st, *shape)
        return lib.sp3d_unproject_fwd_indexed(_lib._ptr_array(views), layout | flags, jp, self.cam.data_ptr(), _lib._opt(so),
                                              self.centers.data_ptr(), self.valid.data_ptr(), res.ptr, gp, *shape)


def sweep_pair(d, idx, o, failures, tally):
    case, dev = d.case, d.dev
    e = fs.expect(idx, o)
    where = (fs.case_id(idx), fs.option_id(o))
    runs = []
    for rep in range(2 if e["rc"] == fs.OK else 1):
        res, lay = result_buffer(case, o, dev)
        grids = grids_buffer(case, dev) if o["grids"] else None
        rc = d.launch(o, res, lay, grids)
        assert rc <= 0, where + ("HIP error", rc)            # a launch that failed: nothing more may run on this GPU
        if rc != e["rc"]:
            failures.append(where + ("return code", rc, e["rc"]))
            return
        runs.append((res, grids))
    res, grids = runs[0]
    if e["rc"] != fs.OK:
        tally["refused"] += 1
        if not res.all_sentinel() or (grids is not None and not grids.all_sentinel()):
            failures.append(where + ("a refused request wrote its result",))
        return
    tally["accepted"] += 1
    tally[e["family"] + " " + e["store"]] += 1
    ref_c, ref_g = d.reference(o)
    if not torch.equal(res.view, ref_c):
        bad = res.view != ref_c
        failures.append(where + ("cubes differ from the oracle", int(bad.sum()), [int(v) for v in bad.nonzero()[0]], e["names"], e["store"]))
    if not res.outside_untouched():
        failures.append(where + ("an element outside the result was written", e["names"], e["store"]))
    if grids is not None:
        if not torch.equal(grids.view, ref_g):
            failures.append(where + ("grids differ from the oracle", e["names"]))
        if not grids.outside_untouched():
            failures.append(where + ("a word outside the grids was written", e["names"]))
    if not torch.equal(res.bits, runs[1][0].bits) or (grids is not None and not torch.equal(grids.bits, runs[1][1].bits)):
        failures.append(where + ("a second launch gave other bits", e["names"]))


def report(failures):
    kinds = collections.Counter(f[2] for f in failures)
    return "\n".join(["%d failed checks: " % len(failures) + "; ".join("%d x %s" % (n, k) for k, n in kinds.items())] +
                     [repr(f) for f in failures[:40]])


@pytest.mark.parametrize("idx", range(len(fs.CASES)), ids=fs.case_id)
def test_every_option_of_the_case(idx):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    d = Device(fs.get(idx), dev)
    failures, tally = [], collections.Counter()
    for o in fs.options(idx):
        sweep_pair(d, idx, o, failures, tally)
    torch.cuda.synchronize(dev)
    print("fwd option sweep %s: %d pairs in %.1f s, %s" % (fs.case_id(idx), len(fs.options(idx)), time.perf_counter() - t0, dict(tally)))
    assert tally["accepted"] + tally["refused"] == len(fs.options(idx)) or failures
    assert not failures, report(failures)
