"""The 17..32-joint training pair on the device against the CPU oracle, on the cases of tests/wide_grad_cases.py
(tests/test_wide_grad_host.py pins the cases): sp3d_unproject_fwd_train with SP3D_HM_WIDE_MASK, both packed scatters with
SP3D_SCATTER_WIDE, and ProjectLayer.wide_grad on the Campus configuration.

The checks and bounds are those of tests/test_gpu_bwd_random_sweep.py (derived in its docstring, imported from it, not
tuned here):
  1  training forward: mask pre-filled with 0x5a5a, cubes bit-equal to the oracle's, both mask planes EQUAL to the planes
     derived from the oracle's forward;
  2  deterministic MERGE, PER_TAP and AUTO: the same integers as each other and run to run (AUTO those of the form the rule
     selects); channels J..31 and samples that own no valid cube exactly zero; per pixel
     |got - ref| <= 2^-22 S + T det_step;
  3  fp32 PER_TAP, MERGE, AUTO: per pixel |got - ref| <= (T + 4) 2^-24 S, zero where the reference is zero, max error
     <= 2e-5 max(1, max|ref|), plane error of the merge <= max(2 per tap, 2e-6);
  4  case 104 replayed from a HIP graph (deterministic MERGE, two sequential launches in one stream);
  5  the module: both hand-overs launch only NHWC / Jp = 32, cubes bit-equal to the no-grad forward, gradients within the
     fp32 bound of the oracle's.
No case skips and no pixel is filtered out.  Every figure is printed before it is asserted (pytest -s / -rP shows them).
"""
import types

import numpy as np
import pytest
import torch

from tests import bwd_sweep_cases as sweep
from tests import wide_grad_cases as wide
from tests.test_gpu_bwd_random_sweep import OnDevice, Report, _fp32_checks, _plane_errors, _planes

pytestmark = pytest.mark.gpu

JP = 32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class WideOnDevice(OnDevice):
    def views(self):
        from selfpose3d_amd import _lib
        packed = _lib.pack_heatmaps(self.hms, jp=JP)
        return [packed[v] for v in range(self.c.V)]

    def train_fwd_wide(self, views, mask):
        from selfpose3d_amd import _lib
        c = self.c
        return _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, JP, self.cam, self.cen, self.val, c.P, c.J, c.h, c.w, c.cube,
                                  c.grid_size, c.img, False, sample_of=self.so, pass_mask=mask, wide_mask=True)[0]

    def wide_bwd(self, mask, scatter, deterministic):
        """-> (V, B, h, w, 32) float32"""
        from selfpose3d_amd import _lib
        c = self.c
        return _lib.unproject_bwd_packed(self.cam, self.cen, self.val, self.grad, mask, c.B, c.V, c.J, JP, c.h, c.w, c.cube,
                                         c.grid_size, c.img, sample_of=self.so, deterministic=deterministic,
                                         return_packed=True, scatter=scatter, wide=True)


def _planes_check(rep, what, mask, expected, J):
    m = mask.cpu().numpy().view(np.uint16)
    if np.array_equal(m, expected):
        return
    diff = (m ^ expected).astype(np.uint32)
    rep.check(False, what + ": mask planes differ from the oracle's:", "plane 0 words", int((diff[0] != 0).sum()),
              "| plane 1 words", int((diff[1] != 0).sum()), "| plane 1 bits >= J - 16", int(((diff[1] >> max(J - 16, 0)) != 0).sum()))


@pytest.mark.parametrize("idx", wide.CASES, ids=wide.case_id)
def test_wide_forms_vs_oracle(dev, idx):
    from selfpose3d_amd import _lib
    c = wide.get(idx)
    d = WideOnDevice(c, dev)
    rep = Report(wide.case_id(idx))
    rep.figure("case", T=c.T, max_ref=float(np.abs(c.ref).max()), det_step=c.det_step)
    own = torch.from_numpy(c.owns_valid).to(dev)

    # 1: training forward with the two-plane mask
    mask = torch.full((2, c.P, c.N), 0x5a5a, dtype=torch.int16, device=dev)     # pre-filled: a word left over shows up as a difference
    cubes = d.train_fwd_wide(d.views(), mask).cpu().numpy()
    rep.check(np.array_equal(cubes, c.fwd), "train fwd: cubes differ from the oracle's, max", float(np.abs(cubes - c.fwd).max()))
    _planes_check(rep, "train fwd", mask, c.expected_mask_planes, c.J)
    # the scatters below read the mask the device wrote, as a training step does

    # 2: deterministic forms
    chosen = "merge" if sweep.auto_takes_merge(c.cube, c.grid_size) else "per_tap"
    det = {}
    for nm, s in (("merge", _lib.SCATTER_MERGE), ("per_tap", _lib.SCATTER_PER_TAP), ("auto", _lib.SCATTER_AUTO)):
        det[nm] = d.wide_bwd(mask, s, True)
        assert det[nm].shape == (c.V, c.B, c.h, c.w, JP)
        rep.check(torch.equal(det[nm], d.wide_bwd(mask, s, True)), "det %s: differs run to run" % nm)
    rep.check(torch.equal(det["merge"], det["per_tap"]), "det: merge and per tap differ on",
              int((det["merge"] != det["per_tap"]).sum()), "elements, max", float((det["merge"] - det["per_tap"]).abs().max()))
    rep.check(torch.equal(det["auto"], det[chosen]), "det: auto differs from " + chosen)
    bound = 2.0 ** -22 * c.S + c.T * c.det_step
    for nm in ("merge", "per_tap"):
        what = "det " + nm
        rep.check(not det[nm][..., c.J:].any(), what + ": channels J..31 not zero")
        rep.check(not det[nm][:, ~own].any(), what + ": gradient on a sample that owns no valid cube")
        err = np.abs(_planes(det[nm], c.J) - c.ref)
        ratio = float((err / bound).max())
        rep.figure(what, err_over_bound=ratio, max_err=float(err.max()))
        rep.check(np.all(err <= bound), what + ": beyond 2^-22 S + T step on", int((err > bound).sum()), "pixels, worst ratio", ratio)

    # 3: fp32 forms
    errs, got = {}, {}
    for nm, s in (("per_tap", _lib.SCATTER_PER_TAP), ("merge", _lib.SCATTER_MERGE), ("auto", _lib.SCATTER_AUTO)):
        out = d.wide_bwd(mask, s, False)
        what = "fp32 " + nm
        rep.check(not out[..., c.J:].any(), what + ": channels J..31 not zero")
        got[nm] = _planes(out, c.J)
        errs[nm] = _fp32_checks(rep, what, got[nm], c)
    e2 = _plane_errors(errs["per_tap"], c)
    for nm in ("merge",) + (("auto",) if chosen == "merge" else ()):
        e3 = _plane_errors(errs[nm], c)
        allowed = np.maximum(2.0 * e2, 2e-6)
        worst = float((e3 / allowed).max())
        rep.figure("fp32 %s vs per tap" % nm, plane_err_over_allowed=worst, merge=float(e3.max()), per_tap=float(e2.max()))
        rep.check(np.all(e3 <= allowed), "fp32 %s: plane error above max(2 per tap, 2e-6), worst ratio" % nm, worst,
                  "at (view, channel)", np.unravel_index(np.argmax(e3 / allowed), e3.shape))
    # AUTO is the form the rule selects: two any-order fp32 sums of the same terms
    rep.check(np.all(np.abs(got["auto"] - got[chosen]) <= 2 * (c.T + 4) * 2.0 ** -24 * c.S), "fp32 auto: not the sums of " + chosen)
    rep.done()


def test_wide_flag_at_16_joints_or_fewer(dev):
    """J <= 16 under the flags: one group, plane 1 written as zeros, and the same gradient as the 16-channel form's reference"""
    from selfpose3d_amd import _lib
    c = sweep.get(7)                    # (4, 4, 2, 9, (33, 17), (8, 8, 4), "space")
    assert c.J <= 16
    d = WideOnDevice(c, dev)
    mask = torch.full((2, c.P, c.N), 0x5a5a, dtype=torch.int16, device=dev)
    cubes = d.train_fwd_wide(d.views(), mask)
    assert np.array_equal(cubes.cpu().numpy(), c.fwd)
    m = mask.cpu().numpy().view(np.uint16)
    assert np.array_equal(m[0], c.expected_mask) and not m[1].any()
    a, b = d.wide_bwd(mask, _lib.SCATTER_MERGE, True), d.wide_bwd(mask, _lib.SCATTER_PER_TAP, True)
    assert torch.equal(a, b) and not a[..., c.J:].any()
    bound = 2.0 ** -22 * c.S + c.T * c.det_step
    assert np.all(np.abs(_planes(a, c.J) - c.ref) <= bound)


def test_wide_deterministic_merge_replayed_from_a_graph(dev):
    from selfpose3d_amd import _lib
    c = wide.get(wide.GRAPH_CASE)
    d = WideOnDevice(c, dev)
    mask = torch.empty((2, c.P, c.N), dtype=torch.int16, device=dev)
    d.train_fwd_wide(d.views(), mask)
    assert np.array_equal(mask.cpu().numpy().view(np.uint16), c.expected_mask_planes)
    eager = d.wide_bwd(mask, _lib.SCATTER_MERGE, True).clone()
    assert torch.count_nonzero(eager[..., :16]) > 500 and torch.count_nonzero(eager[..., 16:]) > 100
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d.wide_bwd(mask, _lib.SCATTER_MERGE, True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):      # the two group launches follow each other in this one stream: no parallel branches
            out = d.wide_bwd(mask, _lib.SCATTER_MERGE, True)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- the module: ProjectLayer.wide_grad on the Campus configuration ---------------------------------------------------
MOD_CUBE = (16, 16, 8)


@pytest.fixture(scope="module")
def campus():
    """Campus YAML at 17 joints, B = 2: inputs, and the oracle's forward / gradient of the root space on a 16x16x8 grid"""
    from oracle import oracle
    from tests.test_gpu_coco17 import rig_setup
    B, J = 2, 17
    cfg, img, hm, V, center, meta, hms, _, cam = rig_setup("campus_synthetic", B, J, seed=41)
    hms = [h * 1.6 - 0.3 for h in hms]                                  # the clamp blocks on both sides
    space = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE]
    rng = np.random.default_rng(41)
    grad = (rng.standard_normal((B, J) + MOD_CUBE) * np.exp(rng.uniform(-6, 3, (B, J, 1, 1, 1)))).astype(np.float32)
    centers = np.repeat(np.asarray([center], np.float32), B, 0)
    valid = np.ones(B, np.uint8)
    np_hms = [h.numpy() for h in hms]
    bwd = lambda g: np.stack(oracle.unproject_bwd(np_hms, cam, centers, valid, g, space, MOD_CUBE, img)).astype(np.float64)
    N = MOD_CUBE[0] * MOD_CUBE[1] * MOD_CUBE[2]
    ref = types.SimpleNamespace(ref=bwd(grad), S=bwd(np.abs(grad)), T=4 * N, owns_valid=np.ones(B, bool))
    return types.SimpleNamespace(cfg=cfg, meta=meta, hms=hms, space=space, center=[list(center)], grad=grad, ref=ref, B=B, J=J, V=V,
                                 h=hm[1], w=hm[0])


def _layer_grads(layer, heatmaps, s, grad):
    cubes, _ = layer(heatmaps, s.meta, s.space, s.center, list(MOD_CUBE))
    cubes.backward(grad)
    return cubes.detach()


def test_module_trains_through_the_nhwc_path(dev, campus, monkeypatch):
    from selfpose3d_amd import _lib
    from selfpose3d_amd.project_layer import ProjectLayer, nhwc_heatmap_views
    from tests.test_gpu_coco17 import wide_calls
    s = campus
    grad = torch.from_numpy(s.grad).to(dev)
    layer = ProjectLayer(s.cfg)
    assert layer.wide_grad is False
    layer.wide_grad = True
    with torch.no_grad():
        want_cubes, _ = layer([h.to(dev) for h in s.hms], s.meta, s.space, s.center, list(MOD_CUBE))
    calls = wide_calls(monkeypatch)
    packs = []
    real_pack = _lib.pack_heatmaps
    monkeypatch.setattr(_lib, "pack_heatmaps", lambda *a, **k: (packs.append(1), real_pack(*a, **k))[1])
    only_wide = lambda: bool(calls) and all(l == _lib.LAYOUT_NHWC and jp == 32 for l, jp in calls)

    # hand-over 1: planar (B, J, h, w) tensors, re-tiled to Jp = 32
    rep = Report("module")
    hg = [h.to(dev).requires_grad_(True) for h in s.hms]
    cubes = _layer_grads(layer, hg, s, grad)
    assert only_wide() and len(calls) == 1 and len(packs) == 1, (calls, packs)
    assert torch.equal(cubes, want_cubes)
    got = torch.stack([h.grad for h in hg]).cpu().numpy().astype(np.float64)
    _fp32_checks(rep, "planar hand-over", got, s.ref)

    # hand-over 2: views of a (V, B, h, w, 32) leaf - no re-tiling pass
    calls.clear()
    packs.clear()
    leaf = real_pack([h.to(dev) for h in s.hms], jp=32).requires_grad_(True)
    cubes = _layer_grads(layer, nhwc_heatmap_views(leaf, s.J), s, grad)
    assert only_wide() and len(calls) == 1 and not packs, (calls, packs)
    assert torch.equal(cubes, want_cubes)
    assert leaf.grad.shape == (s.V, s.B, s.h, s.w, 32) and not leaf.grad[..., s.J:].any()
    _fp32_checks(rep, "channels-last hand-over", _planes(leaf.grad, s.J), s.ref)
    rep.done()

    # deterministic backward: the same bits twice
    layer.deterministic_backward = True
    twice = []
    for _ in range(2):
        hg = [h.to(dev).requires_grad_(True) for h in s.hms]
        _layer_grads(layer, hg, s, grad)
        twice.append(torch.stack([h.grad for h in hg]))
    assert torch.equal(twice[0], twice[1]) and torch.count_nonzero(twice[0][:, :, 16]) > 100
    layer.deterministic_backward = False

    # an explicit NHWC request no longer raises under the switch ...
    calls.clear()
    nhwc = ProjectLayer(s.cfg, mode="nhwc")
    nhwc.wide_grad = True
    hg = [h.to(dev).requires_grad_(True) for h in s.hms]
    assert torch.equal(_layer_grads(nhwc, hg, s, grad), want_cubes) and only_wide()
    # ... and a layer with the switch off still takes the planar kernels
    calls.clear()
    off = ProjectLayer(s.cfg)
    hg = [h.to(dev).requires_grad_(True) for h in s.hms]
    _layer_grads(off, hg, s, grad)
    assert calls == [(_lib.LAYOUT_PLANAR, 0)]
    with pytest.raises(_lib.Sp3dError, match="16 joints"):
        ProjectLayer(s.cfg, mode="nhwc")(hg, s.meta, s.space, s.center, list(MOD_CUBE))
