"""Randomised sweep of the proposal stage on the device against the references of tests/proposal_sweep_cases.py
(tests/test_proposal_sweep_reference.py pins that side on the CPU): nms_chunk_topk_kernel + nms_merge_kernel<8|16>, the three
soft-argmax entry points and the training backward (selfpose3d_amd/csrc/sp3d_proposal.hip).

NMS, per case (signed, all-negative, plateau and non-finite volumes; ties at +-0 across tiles; 1 to 1600 tiles; candidate
counts at and one chunk above the merge kernel's pass sizes; k = 1..32; B up to 260; axes of one bin):
  * nms_topk: values bit for bit (-0.0 stays -0.0), indices equal, locs equal to the fp32 torch expression (NaN == NaN on an
    axis of one bin, where both sides are 0 / 0); a second call and the call without grid_size give the same bits;
  * nms_proposals: rows equal for five thresholds (one returned score exactly, the fp32 number below it, 0, -0.5, +inf).

Soft-argmax, exact, per case:
  * soft_argmax_grid == soft_argmax fed the grids that ProjectLayer.get_voxel writes for the same centres and cube, and those
    grids are the reference's; the training forward's out == soft_argmax_grid, its stats[..., 0] == the fp32 maximum of beta x;
  * one-hot rows return the fp32 voxel centre bit for bit (corners, last voxel, ragged tail, and the middle bin of odd axes of
    a cube at the origin, where the two forms of the fp32 linspace differ);
  * channels-last input gives the bits of planar input, the gradient comes back in the input's format; two runs are bit-equal.
Soft-argmax, bounded (S, T and the sum's scale: tests/proposal_sweep_cases.py):
  * |out - ref| <= C_FWD S;  |stats[..., 1] - sum exp| <= C_FWD u sum_n e_n (2 + |beta x_n| + |beta x_n - m|): a per-term
    scale in place of a sum of exp scaled by the accumulation depth - the depth-scaled form does not cover the rounding of
    the product at |beta x| near 5e4 (the shifted rows) and is loose by the depth everywhere else;
  * |dx - ref| <= C_BWD T element-wise, ref = float64 autograd of the torch graph.

The constants.  Rule: the smallest power of two at or above 4 x the worst measured ratio (the margin covers another reduction
order or another lowering of exp in a later compiler), and below the worst case of the accumulation: a term passes
ceil(N / 1024) additions in its lane, 6 across the wave and 16 across the block; numerator and denominator of the quotient
each cost at most that depth x u x sum p |g|, which S contains once, so the ceiling is 2 (ceil(N / 1024) + 22) = 556 at the
pose net's own 64^3 (more at 96^3; the small shapes are far from any accumulation effect: their ratios are below 1).
Measured on an MI355X (worst ratio per family over all shapes, then per shape over all families):
    family      fwd    sum    bwd   |  shape        fwd    sum    bwd   |  shape        fwd    sum    bwd
    soft        1.91   0.52   0.98  |  64x64x64     0.77   0.44   1.36  |  5x3x2        1.29   0.78   0.83
    flat        2.55   0.98   0.83  |  96x96x96     0      0.44   1.36  |  5x3x1        0.02   0      0.03
    peak        0      0.44   1.36  |  16x12x10     2.55   0.98   0.98  |  1x5x4        0      0.44   0.08
    two_peaks   0.21   0      0.04  |  5x11x31      0.25   0.44   1.17  |  1x1x1025     2.54   0.75   0.13
    one_hot     0      0      0.10  |  3x11x31      1.54   0.45   1.09  |  1x1x1        0      0.20   0.04
    constant    1.29   0.21   0.12  |  7x1x33       1.91   0.48   0.15  |
    shifted     1.54   0.45   1.09  |
Worst overall: forward 2.55, sum of exp 0.98 -> C_FWD = 16 (4 x 2.55 = 10.2); backward 1.36 with C_FWD = 16 inside T
-> C_BWD = 8 (4 x 1.36 = 5.4).  Both far below 556: the error does not grow with the accumulation depth (64^3 and 96^3 are
not the worst shapes), the strided lanes and the tree across wave and block keep it at a few u.
Every figure is printed before it is asserted (pytest -s / -rP shows them).  Each case is a handful of launches; nothing is
repeated to provoke anything, no graph is captured and no environment variable is read or set.
"""
import numpy as np
import pytest
import torch

from tests import proposal_sweep_cases as sweep

pytestmark = pytest.mark.gpu

NMS = list(range(len(sweep.nms_cases())))
SA = list(range(len(sweep.sa_cases())))

C_FWD = 16.0
C_BWD = 8.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


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


def _first_diff(got, exp):
    """where two arrays first differ bit for bit: (index, got, expected)"""
    d = np.argwhere(sweep.bits(got) != sweep.bits(exp))
    if not len(d):
        return ""
    i = tuple(d[0])
    return "first at %s: got %r expected %r (%d differ)" % (i, got[i], exp[i], len(d))


# ---------------------------------------------------------------------------------------------------------------------------
# NMS
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", NMS, ids=sweep.nms_case_id)
def test_nms_topk_and_proposal_rows_vs_reference(dev, idx):
    from selfpose3d_amd import _lib
    c = sweep.nms_get(idx)
    rep = Report(sweep.nms_case_id(idx))
    xd = torch.from_numpy(c.x).to(dev)
    exp_v, exp_i, exp_l = c.vals, c.idx3, c.locs
    rep.figure("case", tiles=sweep.num_tiles(c.shape), candidates=sweep.num_tiles(c.shape) * c.k,
               negative=float((exp_v < 0).sum()), zeros=float((exp_v == 0).sum()))
    vals, idx3, locs = _lib.nms_topk(xd, c.k, c.grid_size, c.grid_center)
    v, i3, lc = vals.cpu().numpy(), idx3.cpu().numpy(), locs.cpu().numpy()
    rep.check(v.shape == exp_v.shape and i3.shape == exp_i.shape and i3.dtype == np.int64 and lc.shape == exp_l.shape, "shapes")
    rep.check(np.array_equal(sweep.bits(v), sweep.bits(exp_v)), "values differ:", _first_diff(v, exp_v))
    bad = np.argwhere((i3 != exp_i).any(-1))
    rep.check(not len(bad), "indices differ in", len(bad), "slots, first", bad[:1].tolist(),
              "got", i3[tuple(bad[0])].tolist() if len(bad) else "", "expected", exp_i[tuple(bad[0])].tolist() if len(bad) else "")
    rep.check(np.array_equal(lc, exp_l, equal_nan=True), "locs differ, max", float(np.nanmax(np.abs(lc - exp_l), initial=0.0)))
    # a second call, and the call without grid_size
    v2, i2, l2 = _lib.nms_topk(xd, c.k, c.grid_size, c.grid_center)
    rep.check(torch.equal(v2.view(torch.int32), vals.view(torch.int32)) and torch.equal(i2, idx3)
              and torch.equal(l2.view(torch.int32), locs.view(torch.int32)), "a second call differs")
    v3, i3b, l3 = _lib.nms_topk(xd, c.k)
    rep.check(l3 is None and torch.equal(v3.view(torch.int32), vals.view(torch.int32)) and torch.equal(i3b, idx3),
              "the call without grid_size differs")
    for t in c.thresholds:
        rows = _lib.nms_proposals(xd, c.k, c.grid_size, c.grid_center, t).cpu().numpy()
        exp = c.rows(t)
        rep.check(rows.shape == exp.shape and sweep.rows_equal(rows, exp), "rows differ at threshold %r:" % t,
                  "flags", int((rows[..., 3] != exp[..., 3]).sum()), "scores", int((sweep.bits(rows[..., 4]) != sweep.bits(exp[..., 4])).sum()),
                  "mm", int((~np.isclose(rows[..., :3], exp[..., :3], rtol=0, atol=0, equal_nan=True)).sum()))
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------
# soft-argmax
# ---------------------------------------------------------------------------------------------------------------------------
def _device_grids(c, dev):
    """(P, N, 3): the voxel centres as the unprojection kernel writes them for the case's centres and cube"""
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer
    cfg = load_config(None, NETWORK__IMAGE_SIZE=[128, 96], NETWORK__HEATMAP_SIZE=[32, 24])
    meta = syn.make_meta(1, 2, (128, 96))
    hms = [h.to(dev) for h in syn.random_heatmaps(1, 2, 2, 24, 32, seed=4)]
    _, grids = ProjectLayer(cfg).get_voxel(hms, meta, list(c.grid_size), torch.from_numpy(c.centers).to(dev), list(c.cube),
                                           sample_of=torch.zeros(c.P, dtype=torch.int32))
    return grids


def _soft_argmax_case(dev, idx):
    """every check of one case -> (its Report, its worst ratios (forward, sum of exp, backward))"""
    from selfpose3d_amd import _lib
    c = sweep.sa_get(idx)
    rep = Report(sweep.sa_case_id(idx))
    P, J, cube, gs, beta = c.P, c.J, c.cube, c.grid_size, c.beta
    x0 = torch.from_numpy(c.x).to(dev)
    cen = torch.from_numpy(c.centers).to(dev)
    wgt = torch.from_numpy(c.wgt).to(dev)

    # exact: the three forward entry points, on the grids of the unprojection kernel
    grids = _device_grids(c, dev)
    rep.check(np.array_equal(grids.cpu().numpy().reshape(P, c.N, 3), c.grids), "get_voxel's grids differ from the reference's")
    out_grid = _lib.soft_argmax_grid(x0, cen, gs, cube, beta)
    out_mat = _lib.soft_argmax(x0, grids, beta)
    rep.check(torch.equal(out_mat.view(torch.int32), out_grid.view(torch.int32)), "in-kernel grid != materialised grid, max",
              float((out_mat - out_grid).abs().max()))
    rep.check(torch.equal(_lib.soft_argmax_grid(x0, cen, gs, cube, beta).view(torch.int32), out_grid.view(torch.int32)),
              "soft_argmax_grid differs run to run")
    out = out_grid.cpu().numpy()
    if c.family == "one_hot":
        want = c.grids[np.arange(P)[:, None], c.hot]
        bad = np.argwhere(sweep.bits(out) != sweep.bits(want))
        rep.check(not len(bad), "one-hot rows are not the voxel centre:", _first_diff(out, want),
                  "kind", c.hot_kind[int(bad[0][0]) * J + int(bad[0][1])] if len(bad) else "")

    # training pair, planar and channels-last
    dxs = {}
    for name, fmt in (("planar", torch.contiguous_format), ("channels-last", torch.channels_last_3d)):
        x = x0.clone().contiguous(memory_format=fmt).requires_grad_(True)
        o = _lib.soft_argmax_grid_autograd(x, cen, gs, cube, beta)
        (o * wgt).sum().backward()
        rep.check(torch.equal(o.detach().view(torch.int32), out_grid.view(torch.int32)), name + ": training out != soft_argmax_grid")
        rep.check(x.grad.shape == x.shape and x.grad.is_contiguous(memory_format=fmt), name + ": gradient not in the input's format")
        dxs[name] = x.grad.contiguous()
    rep.check(torch.equal(dxs["planar"].view(torch.int32), dxs["channels-last"].view(torch.int32)), "channels-last gradient differs")
    x = x0.clone().requires_grad_(True)
    (_lib.soft_argmax_grid_autograd(x, cen, gs, cube, beta) * wgt).sum().backward()
    rep.check(torch.equal(x.grad.view(torch.int32), dxs["planar"].view(torch.int32)), "gradient differs run to run")
    # the statistics the training forward keeps for the backward
    lib = _lib.load()
    stats = torch.full((P, J, 2), float("nan"), device=dev)
    o2 = torch.empty((P, J, 3), device=dev)
    _lib.check(lib.sp3d_soft_argmax_grid_train(x0.data_ptr(), cen.data_ptr(), _lib._f3(gs), cube[0], cube[1], cube[2], o2.data_ptr(),
                                               stats.data_ptr(), P, J, float(beta), _lib._stream(dev)), "sp3d_soft_argmax_grid_train")
    st = stats.cpu().numpy()
    rep.check(torch.equal(o2.view(torch.int32), out_grid.view(torch.int32)), "train out != soft_argmax_grid")
    rep.check(np.array_equal(sweep.bits(st[..., 0]), sweep.bits(c.max32)), "stats[..., 0] is not the fp32 maximum of beta x:",
              _first_diff(st[..., 0], c.max32))

    # bounded
    err = np.abs(out.astype(np.float64) - c.out)
    S = c.S
    r_fwd = float((err[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0
    rep.check((err <= C_FWD * S).all(), "forward beyond C_FWD S: worst ratio", r_fwd, "exact-zero scale missed", int((err[S == 0] != 0).sum()))
    se, scale = c.sumexp
    err_s = np.abs(st[..., 1].astype(np.float64) - se)
    r_sum = float((err_s / scale).max())
    rep.check((err_s <= C_FWD * scale).all(), "sum of exp beyond C_FWD scale: worst ratio", r_sum)
    T = c.T(C_FWD)
    err_b = np.abs(dxs["planar"].cpu().numpy().astype(np.float64) - c.dx)
    r_bwd = float((err_b / T).max())
    rep.check((err_b <= C_BWD * T).all(), "backward beyond C_BWD T on", int((err_b > C_BWD * T).sum()), "elements, worst ratio", r_bwd)
    rep.figure("ratios", fwd=r_fwd, sumexp=r_sum, bwd=r_bwd, max_err_mm=float(err.max()), depth=sweep.accumulation_depth(c.N))
    # the project's own tolerance on the shape and family it was set on
    if c.family == "soft" and beta == 100.0 and cube == (16, 12, 10):
        rep.check(err.max() <= 2e-3, "max error", float(err.max()), "> 2e-3 mm")
        rel = float(np.abs(err_b).max() / np.abs(c.dx).max())
        rep.check(rel <= 2e-4, "gradient error relative to its maximum", rel, "> 2e-4")
    return rep, (r_fwd, r_sum, r_bwd)


@pytest.fixture(scope="module")
def soft_argmax_results(dev):
    """idx -> (Report, ratios); every case runs once per module, whichever test asks for it first"""
    done = {}

    def get(idx):
        if idx not in done:
            done[idx] = _soft_argmax_case(dev, idx)
        return done[idx]
    return get


@pytest.mark.parametrize("idx", SA, ids=sweep.sa_case_id)
def test_soft_argmax_forms_vs_float64(soft_argmax_results, idx):
    soft_argmax_results(idx)[0].done()


def test_measured_ratios_and_the_constants(soft_argmax_results):
    """prints the worst measured ratio per family and per shape (the table of the module docstring) and how the constants stand
    to their rule on this device.  Asserted: the constants are below the accumulation's worst case.  The rule "4 x the worst
    measured ratio" is how they were SET and is only printed here: the bounds the suite enforces are C_FWD S and C_BWD T
    themselves, in the per-case test, so the 4 x margin stays available to a later compiler."""
    ratios = {idx: soft_argmax_results(idx)[1] for idx in SA}
    worst = np.array([ratios[i] for i in SA]).max(0)
    for key, label in ((4, "family"), (2, "shape")):
        for val in sorted({sweep.sa_cases()[i][key] for i in SA}, key=str):
            r = np.array([ratios[i] for i in SA if sweep.sa_cases()[i][key] == val]).max(0)
            print("sweep worst ratios %s %-14s fwd=%.3g sumexp=%.3g bwd=%.3g" % (label, val, r[0], r[1], r[2]))
    print("sweep worst ratios overall fwd=%.3g sumexp=%.3g bwd=%.3g  C_FWD=%g C_BWD=%g" % (worst[0], worst[1], worst[2], C_FWD, C_BWD))
    print("sweep margin left: C_FWD / worst = %.3g, C_BWD / worst = %.3g (4 when the constants were set)"
          % (C_FWD / max(worst[0], worst[1], 1e-30), C_BWD / max(worst[2], 1e-30)))
    ceiling = 2 * sweep.accumulation_depth(64 ** 3)
    assert C_FWD < ceiling and C_BWD < ceiling
