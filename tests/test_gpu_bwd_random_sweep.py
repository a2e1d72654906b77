"""Randomised sweep of the unprojection BACKWARD and of the pass mask of the training forward against the CPU oracle, on the
cases of tests/bwd_sweep_cases.py (random rigs, rotated / scaled / flipped crops, V = 1..16, J = 1..20, 2x2 to 480x256 maps,
cubes that are no multiple of the 8x8x4 block on any axis, P cubes over B samples, invalid cubes, samples that own no cube);
tests/test_bwd_sweep_reference.py pins the reference side on the CPU.

Per case and packed channel stride (the smallest of 4 / 8 / 12 / 16 that holds J, 16 as well on every third case):
  1  training forward, planar and channels-last: cubes bit-equal to the oracle, the pass-mask words EQUAL to the mask derived
     from the oracle's forward (bit j < J per voxel, nothing at or above J, zero rows for invalid cubes);
  2  deterministic MERGE and PER_TAP: the same integers as each other and run to run; pad channels and samples without a
     valid cube exactly zero; per pixel
         |got - ref| <= 2^-22 S + T 2^-40 2^ceil(log2 max|grad|)
     S = sum of the absolute contributions to the pixel (oracle, float64), T = 4 X Y Z (most cubes on one sample) the
     largest number of additions a pixel can receive.  Kernel and oracle form the same fp32 products g / den * w; one
     fixed-point step is 2^-40 2^ceil(log2 max|grad|), each addition rounds by at most half a step (the bound keeps a factor
     of 2), the conversion back rounds once; 2^-22 S allows one ulp of difference in a tap weight or in the division.  A
     dropped or misplaced tap is of the order S / (taps on the pixel): far above.  The fp32 forms share addressing, mask and
     weights with these two (the DET template flag), so this is the check that carries the sweep;
  3  fp32 forms (planar with sample_of, PER_TAP, MERGE, AUTO): per pixel |got - ref| <= (T + 4) 2^-24 S (any-order fp32
     summation of at most T terms: provable and loose), exactly zero where the reference is zero, and the project's own
     empirical tolerances (2e-5 of the largest gradient; per (view, channel) plane err(MERGE) <= max(2 err(PER_TAP), 2e-6),
     which is what catches a wrong per-block scale on the small channels).  AUTO passes the checks of the form the
     documented rule selects and agrees with it;
  4  J = 17 and 20: the planar form only; the training forward and the packed scatter refuse (unsupported combination)
     before any launch;
  5  one case replayed from a HIP graph (deterministic MERGE): the replay's integers are the eager ones.
No case skips and no pixel is filtered out.  Every figure is printed before it is asserted (pytest -s / -rP shows them).
"""
import numpy as np
import pytest
import torch

from tests import bwd_sweep_cases as sweep

pytestmark = pytest.mark.gpu

CASES = list(range(len(sweep.cases())))
GRAPH_CASE = 5          # P = 5 over B = 2, an invalid cube, ragged blocks on all axes

# The project's empirical fp32 tolerances were set on maps of 120x64 pixels and more; they hold on every case here, the 2x2
# and 9x7 maps with thousands of taps per pixel included (largest max error / tolerance 0.10, largest plane error / allowed
# 0.17), so no case falls back to the provable per-pixel bound alone.


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class OnDevice:
    def __init__(self, c, dev):
        self.c = c
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.cam, self.cen, self.val, self.grad = t(c.cam), t(c.centers), t(c.valid), t(c.grad)
        # identity sample_of: as an explicit index on even cases, as "no index" on odd ones
        self.so = None if (c.P == c.B and c.idx % 2 == 1) else t(c.sample_of)
        self.hms = [t(x) for x in c.hms]
        self.dev = dev

    def train_fwd(self, views, jp, channels_last, mask):
        from selfpose3d_amd import _lib
        c = self.c
        return _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, jp, self.cam, self.cen, self.val, c.P, c.J, c.h, c.w, c.cube,
                                  c.grid_size, c.img, False, channels_last=channels_last, sample_of=self.so, pass_mask=mask)[0]

    def packed_bwd(self, mask, jp, scatter, deterministic):
        """-> (V, B, h, w, jp) float32, pad channels included"""
        from selfpose3d_amd import _lib
        c = self.c
        return _lib.unproject_bwd_packed(self.cam, self.cen, self.val, self.grad, mask, c.B, c.V, c.J, jp, c.h, c.w, c.cube,
                                         c.grid_size, c.img, sample_of=self.so, deterministic=deterministic,
                                         return_packed=True, scatter=scatter)

    def planar_bwd(self):
        from selfpose3d_amd import _lib
        c = self.c
        return torch.stack(list(_lib.unproject_bwd(self.hms, self.cam, self.cen, self.val, self.grad, c.cube, c.grid_size,
                                                   c.img, sample_of=self.so)))


class Report:
    """collects every failed check of a case, so that one run shows all of them, and prints each figure"""

    def __init__(self, name):
        self.name, self.problems = name, []

    def check(self, ok, what, *figures):
        if not ok:
            self.problems.append("%s %s" % (what, " ".join(str(f) for f in figures)))

    def figure(self, what, **kv):
        print("sweep %s %s: %s" % (self.name, what, " ".join("%s=%.4g" % (k, v) for k, v in kv.items())))

    def done(self):
        assert not self.problems, "%s:\n  " % self.name + "\n  ".join(self.problems)


def _planes(packed, J):
    """(V, B, h, w, jp) device -> (V, B, J, h, w) float64 host"""
    return packed[..., :J].permute(0, 1, 4, 2, 3).contiguous().cpu().numpy().astype(np.float64)


def _mask_check(rep, what, mask, c):
    m = mask.cpu().numpy().view(np.uint16)
    exp = c.expected_mask
    if np.array_equal(m, exp):
        return
    diff = (m ^ exp).astype(np.uint32)
    low = diff & ((1 << c.J) - 1)
    unseen = np.broadcast_to((~c.seen).reshape(c.P, c.N), diff.shape)
    inval = np.broadcast_to((c.valid == 0)[:, None], diff.shape)
    rep.check(False, what + ": pass mask differs from the oracle's:", "words", int((diff != 0).sum()),
              "| bits < J on seen voxels", int((low != 0)[~unseen & ~inval].sum()),
              "| bits < J on unseen voxels", int((low != 0)[unseen & ~inval].sum()),
              "| bits >= J", int(((diff >> c.J) != 0).sum()), "| on invalid cubes", int((diff != 0)[inval].sum()))


def _fp32_checks(rep, what, got, c):
    """checks of one fp32 form against the reference; -> its error array"""
    err = np.abs(got - c.ref)
    bound = (c.T + 4) * 2.0 ** -24 * c.S
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    scale = max(1.0, float(np.abs(c.ref).max()))
    rep.figure(what, err_over_provable_bound=ratio, max_err=float(err.max()), project_tol=2e-5 * scale)
    rep.check(np.all(err <= bound), what + ": beyond (T + 4) 2^-24 S on", int((err > bound).sum()), "pixels, worst ratio", ratio)
    rep.check(not got[c.ref == 0].any(), what + ": non-zero where the reference is zero on", int((got[c.ref == 0] != 0).sum()))
    rep.check(not got[:, ~c.owns_valid].any(), what + ": gradient on a sample that owns no valid cube")
    rep.check(err.max() <= 2e-5 * scale, what + ": max error", float(err.max()), "> 2e-5 *", scale)
    return err


def _plane_errors(err, c):
    """(V, J): per (view, channel) plane the largest error relative to the plane's largest |ref|"""
    scale = np.maximum(1e-30, np.abs(c.ref).max(axis=(1, 3, 4)))
    return err.max(axis=(1, 3, 4)) / scale


def _packed_forms(rep, d, jp, dev):
    from selfpose3d_amd import _lib
    c = d.c
    tag = "jp=%d" % jp
    packed = _lib.pack_heatmaps(d.hms, jp=jp)
    views = [packed[v] for v in range(c.V)]
    own = torch.from_numpy(c.owns_valid).to(dev)

    # 1: training forward, planar and (J % 4 == 0) channels-last
    mask = None
    for cl in ((False, True) if c.J % 4 == 0 else (False,)):
        m = torch.full((c.P, c.N), 0x5a5a, dtype=torch.int16, device=dev)       # pre-filled: a word left over shows up as a difference
        cubes = d.train_fwd(views, jp, cl, m)
        what = "%s train fwd%s" % (tag, " channels-last" if cl else "")
        rep.check(np.array_equal(cubes.cpu().numpy(), c.fwd), what + ": cubes differ from the oracle's, max",
                  float(np.abs(cubes.cpu().numpy() - c.fwd).max()))
        _mask_check(rep, what, m, c)
        mask = m if mask is None else mask
    # the scatters below read the mask the device wrote (the planar training forward's), as a training step does

    # 2: deterministic forms
    det = {}
    for nm, s in (("merge", _lib.SCATTER_MERGE), ("per_tap", _lib.SCATTER_PER_TAP), ("auto", _lib.SCATTER_AUTO)):
        det[nm] = d.packed_bwd(mask, jp, s, True)
        rep.check(torch.equal(det[nm], d.packed_bwd(mask, jp, s, True)), "%s det %s: differs run to run" % (tag, nm))
    rep.check(torch.equal(det["merge"], det["per_tap"]), tag + " det: merge and per tap differ on",
              int((det["merge"] != det["per_tap"]).sum()), "elements, max", float((det["merge"] - det["per_tap"]).abs().max()))
    rep.check(torch.equal(det["auto"], det["merge"]), tag + " det: auto differs from merge")
    bound = 2.0 ** -22 * c.S + c.T * c.det_step
    for nm in ("merge", "per_tap"):
        what = "%s det %s" % (tag, nm)
        rep.check(not det[nm][..., c.J:].any(), what + ": pad channels not zero")
        rep.check(not det[nm][:, ~own].any(), what + ": gradient on a sample that owns no valid cube")
        err = np.abs(_planes(det[nm], c.J) - c.ref)
        ratio = float((err / bound).max())
        rep.figure(what, err_over_bound=ratio, max_err=float(err.max()))
        rep.check(np.all(err <= bound), what + ": beyond 2^-22 S + T step on", int((err > bound).sum()), "pixels, worst ratio", ratio)

    # 3: fp32 packed forms
    errs = {}
    got = {}
    for nm, s in (("per_tap", _lib.SCATTER_PER_TAP), ("merge", _lib.SCATTER_MERGE), ("auto", _lib.SCATTER_AUTO)):
        out = d.packed_bwd(mask, jp, s, False)
        what = "%s fp32 %s" % (tag, nm)
        rep.check(not out[..., c.J:].any(), what + ": pad channels not zero")
        got[nm] = _planes(out, c.J)
        errs[nm] = _fp32_checks(rep, what, got[nm], c)
    chosen = "merge" if sweep.auto_takes_merge(c.cube, c.grid_size) else "per_tap"
    e2 = _plane_errors(errs["per_tap"], c)
    for nm in ("merge",) + (("auto",) if chosen == "merge" else ()):
        e3 = _plane_errors(errs[nm], c)
        worst = float((e3 / np.maximum(2.0 * e2, 2e-6)).max())
        rep.figure("%s fp32 %s vs per tap" % (tag, nm), plane_err_over_allowed=worst, merge=float(e3.max()), per_tap=float(e2.max()))
        rep.check(np.all(e3 <= np.maximum(2.0 * e2, 2e-6)), "%s fp32 %s: plane error above max(2 per tap, 2e-6), worst ratio" % (tag, nm),
                  worst, "at (view, channel)", np.unravel_index(np.argmax(e3 / np.maximum(2.0 * e2, 2e-6)), e3.shape))
    # AUTO is the form the rule selects: two any-order fp32 sums of the same terms
    rep.check(np.all(np.abs(got["auto"] - got[chosen]) <= 2 * (c.T + 4) * 2.0 ** -24 * c.S), tag + " fp32 auto: not the sums of " + chosen)


def _wide_refuses(rep, d, dev):
    """J > 16: no pass mask and no packed scatter - refused before anything is launched (outputs untouched)"""
    from selfpose3d_amd import _lib
    c = d.c
    for jp in (16, 32):
        packed = _lib.pack_heatmaps(d.hms, jp=32)
        mask = torch.full((c.P, c.N), 0x5a5a, dtype=torch.int16, device=dev)
        with pytest.raises(_lib.Sp3dError, match="unsupported combination"):
            d.train_fwd([packed[v] for v in range(c.V)], jp, False, mask)
        with pytest.raises(_lib.Sp3dError, match="unsupported combination"):
            d.packed_bwd(mask, jp, _lib.SCATTER_AUTO, False)
        with pytest.raises(_lib.Sp3dError, match="unsupported combination"):
            d.packed_bwd(mask, jp, _lib.SCATTER_MERGE, True)
        torch.cuda.synchronize()
        rep.check(bool((mask == 0x5a5a).all()), "jp=%d: a refused call wrote the pass mask" % jp)


@pytest.mark.parametrize("idx", CASES, ids=sweep.case_id)
def test_backward_forms_and_pass_mask_vs_oracle(dev, idx):
    c = sweep.get(idx)
    d = OnDevice(c, dev)
    rep = Report(sweep.case_id(idx))
    rep.figure("case", T=c.T, mean_taps_per_pixel=4.0 * c.N * c.cubes_per_sample.max() * c.V / (c.h * c.w),
               max_ref=float(np.abs(c.ref).max()), det_step=c.det_step)
    errp = _fp32_checks(rep, "fp32 planar", d.planar_bwd().cpu().numpy().astype(np.float64), c)
    assert errp.shape == c.ref.shape
    strides = sweep.channel_strides(idx, c.J)
    if c.J > 16:
        assert not strides
        _wide_refuses(rep, d, dev)
    else:
        assert strides
        for jp in strides:
            _packed_forms(rep, d, jp, dev)
    rep.done()


def test_deterministic_merge_replayed_from_a_graph(dev):
    from selfpose3d_amd import _lib
    c = sweep.get(GRAPH_CASE)
    d = OnDevice(c, dev)
    jp = sweep.channel_strides(GRAPH_CASE, c.J)[0]
    packed = _lib.pack_heatmaps(d.hms, jp=jp)
    mask = torch.empty((c.P, c.N), dtype=torch.int16, device=dev)
    d.train_fwd([packed[v] for v in range(c.V)], jp, False, mask)
    assert np.array_equal(mask.cpu().numpy().view(np.uint16), c.expected_mask)
    eager = d.packed_bwd(mask, jp, _lib.SCATTER_MERGE, True).clone()
    assert torch.count_nonzero(eager) > 500
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d.packed_bwd(mask, jp, _lib.SCATTER_MERGE, True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            out = d.packed_bwd(mask, jp, _lib.SCATTER_MERGE, True)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
