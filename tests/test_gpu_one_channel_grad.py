"""The one-channel training pair on the GPU (sp3d_unproject_one_fwd_train, sp3d_unproject_one_bwd[_det]) on the cases of
tests/one_channel_grad_cases.py: every case of the backward sweep seen as a one-channel case (channel idx % J of its maps, the
J = 17 and 20 cases included) and one V = 12 case.

Per case, for both hand-overs - the channel's plane inside the planar (B,J,h,w) tensors, and the channel inside a packed
(V,B,h,w,jp) buffer with jp = ProjectLayer.jp_for(J) (32 included):
  1  training forward, results planar 1, planar 4 and channels-last 4: cubes bit-equal to the oracle channel, pad channels
     exactly zero; mask words EQUAL to the expected words (bit 0, nothing above, zero rows for invalid cubes) and to the words
     sp3d_unproject_fwd_train writes for the contiguous J = 1 slice at jp = 4;
  2  deterministic backward: equal run to run; bit-equal to channel 0 of unproject_bwd_packed(deterministic=True) at jp = 4
     on the contiguous slice, for SCATTER_PER_TAP and SCATTER_MERGE; within the sweep's 2^-22 S + T det_step of the oracle;
     exactly zero on samples that own no valid cube; the same integers with the packed forward's mask, and the packed backward
     the same with the new forward's mask; the same from a planar (P,4,..) gradient read at its stride;
  3  fp32 backward: the sweep's _fp32_checks (the provable (T + 4) 2^-24 S per pixel, zero where the reference is zero, the
     project's 2e-5 max(1, max|ref|)) - the existing numbers, none new;
  4  one case (the sweep's GRAPH_CASE): forward + deterministic backward replayed from a HIP graph equal the eager integers.
Then ProjectLayer (switch on vs off: no pack, equal cubes and gradients, the old switch untouched) and the ROOTNET_ROOTHM root
nets in train() mode.  No case skips, no pixel is filtered; every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import one_channel_grad_cases as cases
from tests.test_gpu_bwd_random_sweep import GRAPH_CASE, Report, _fp32_checks
from tests.test_gpu_one_channel import SMALL, _PackSpy, _small_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class OnDevice:
    def __init__(self, c, dev):
        from selfpose3d_amd import _lib
        from selfpose3d_amd.project_layer import ProjectLayer
        self.c, self.dev = c, dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.cam, self.cen, self.val, self.grad = t(c.cam), t(c.centers), t(c.valid), t(c.grad)
        # identity sample_of: as an explicit index on even cases, as "no index" on odd ones
        self.so = None if (c.P == c.B and c.idx % 2 == 1) else t(c.sample_of)
        hms = [t(x) for x in c.hms]                                                  # (B,Jt,h,w): the wider tensors
        r = c.rid
        jp = ProjectLayer.jp_for(c.Jt)
        packed = _lib.pack_heatmaps(hms, jp=jp)                                      # (V,B,h,w,jp): the wider buffer
        self.hand_overs = [("planar", _lib.LAYOUT_PLANAR, c.Jt, [x[:, r:r + 1] for x in hms]),
                           ("nhwc%d" % jp, _lib.LAYOUT_NHWC, jp, [packed[v].permute(0, 3, 1, 2)[:, r:r + 1] for v in range(c.V)])]
        # the old path's operands: the contiguous slice, re-tiled to 4 channels
        self.packed4 = _lib.pack_heatmaps([t(x) for x in c.hms_one], jp=4)
        self.own = torch.from_numpy(c.owns_valid).to(dev)

    def fresh_mask(self):
        return torch.full((self.c.P, self.c.N), 0x5a5a, dtype=torch.int16, device=self.dev)     # a word left over shows up

    def one_fwd(self, views, layout, jp, J, cl, mask):
        from selfpose3d_amd import _lib
        c = self.c
        return _lib.unproject_one_fwd_train(views, layout, jp, self.cam, self.cen, self.val, c.P, J, c.h, c.w, c.cube, c.grid_size,
                                            c.img, mask, False, channels_last=cl, sample_of=self.so)[0]

    def packed_fwd_mask(self):
        from selfpose3d_amd import _lib
        c = self.c
        m = self.fresh_mask()
        _lib.unproject_fwd([self.packed4[v] for v in range(c.V)], _lib.LAYOUT_NHWC, 4, self.cam, self.cen, self.val, c.P, 1, c.h,
                           c.w, c.cube, c.grid_size, c.img, False, sample_of=self.so, pass_mask=m)
        return m

    def one_bwd(self, mask, deterministic, grad=None):
        """-> (V, B, 1, h, w) float32"""
        from selfpose3d_amd import _lib
        c = self.c
        return torch.stack(_lib.unproject_one_bwd(self.cam, self.cen, self.val, self.grad if grad is None else grad, mask, c.B,
                                                  c.V, c.h, c.w, c.cube, c.grid_size, c.img, sample_of=self.so,
                                                  deterministic=deterministic))

    def packed_bwd(self, mask, scatter):
        """channel 0 of the deterministic packed scatter at jp = 4 -> (V, B, 1, h, w) float32, and its pad channels"""
        from selfpose3d_amd import _lib
        c = self.c
        out = _lib.unproject_bwd_packed(self.cam, self.cen, self.val, self.grad, mask, c.B, c.V, 1, 4, c.h, c.w, c.cube,
                                        c.grid_size, c.img, sample_of=self.so, deterministic=True, return_packed=True,
                                        scatter=scatter)
        return out[..., 0].unsqueeze(2), out[..., 1:]


def _words(mask):
    return mask.cpu().numpy().view(np.uint16)


def _forward_checks(rep, d, name, layout, jp, views, packed_words):
    c = d.c
    mask = None
    for form, J, cl in (("planar1", 1, False), ("planar4", 4, False), ("cl4", 4, True)):
        what = "%s fwd %s" % (name, form)
        m = d.fresh_mask()
        cubes = d.one_fwd(views, layout, jp, J, cl, m)
        g = cubes.cpu().numpy()
        rep.check(g.shape == (c.P, J) + tuple(c.cube), what + ": shape", g.shape)
        if cl:
            rep.check(cubes.is_contiguous(memory_format=torch.channels_last_3d), what + ": not channels-last")
        rep.check(np.array_equal(g[:, :1], c.fwd), what + ": cubes differ from the oracle's channel, max",
                  float(np.nanmax(np.abs(g[:, :1] - c.fwd))))
        rep.check(not g[:, 1:].any(), what + ": pad channels not zero")
        w = _words(m)
        diff = w != c.expected_mask
        rep.check(not diff.any(), what + ": mask differs from the expected words on", int(diff.sum()), "voxels | bits above 0:",
                  int((w > 1).sum()), "| on unseen voxels:", int(diff[~c.seen.reshape(c.P, c.N)].sum()))
        rep.check(np.array_equal(w, packed_words), what + ": mask differs from the packed training forward's on",
                  int((w != packed_words).sum()), "voxels")
        rep.check(not w[c.valid == 0].any(), what + ": words of an invalid cube not zero")
        mask = m if mask is None else mask
    return mask


def _backward_checks(rep, d, name, mask, packed_mask, packed_det):
    from selfpose3d_amd import _lib
    c = d.c
    det = d.one_bwd(mask, True)
    rep.check(tuple(det.shape) == (c.V, c.B, 1, c.h, c.w), name + " det: shape", tuple(det.shape))
    rep.check(torch.equal(det, d.one_bwd(mask, True)), name + " det: differs run to run")
    for nm, (ch0, pad) in packed_det.items():
        rep.check(torch.equal(det, ch0), name + " det: differs from channel 0 of the packed %s scatter on" % nm,
                  int((det != ch0).sum()), "pixels, max", float((det - ch0).abs().max()))
        rep.check(not pad.any(), name + ": packed %s pad channels not zero" % nm)
    got = det.cpu().numpy().astype(np.float64)
    err = np.abs(got - c.ref)
    bound = 2.0 ** -22 * c.S + c.T * c.det_step
    ratio = float((err / bound).max())
    rep.figure(name + " det", err_over_bound=ratio, max_err=float(err.max()), max_ref=float(np.abs(c.ref).max()))
    rep.check(np.all(err <= bound), name + " det: beyond 2^-22 S + T step on", int((err > bound).sum()), "pixels, worst ratio", ratio)
    rep.check(not det[:, ~d.own].any(), name + " det: gradient on a sample that owns no valid cube")
    # masks are interchangeable, in both directions
    rep.check(torch.equal(d.one_bwd(packed_mask, True), det), name + " det: another result with the packed forward's mask")
    rep.check(torch.equal(d.packed_bwd(mask, _lib.SCATTER_PER_TAP)[0], det), name + " det: packed scatter differs with the new mask")
    # a planar (P,4,X,Y,Z) gradient is read at its cube stride: channels 1-3 (noise) must not reach the result
    g4 = torch.randn((c.P, 4) + tuple(c.cube), device=d.dev)
    g4[:, 0] = d.grad[:, 0]
    rep.check(torch.equal(d.one_bwd(mask, True, grad=g4), det), name + " det: another result from a (P,4,..) gradient")
    cl = g4.contiguous(memory_format=torch.channels_last_3d)
    rep.check(torch.equal(d.one_bwd(mask, True, grad=cl), det), name + " det: another result from a channels-last gradient")
    # fp32
    _fp32_checks(rep, name + " fp32", d.one_bwd(mask, False).cpu().numpy().astype(np.float64), c)


@pytest.mark.parametrize("idx", cases.indices(), ids=cases.case_id)
def test_training_pair_vs_oracle_and_packed_path(dev, idx):
    from selfpose3d_amd import _lib
    c = cases.get(idx)
    d = OnDevice(c, dev)
    rep = Report(cases.case_id(idx) + "/ch%d" % c.rid)
    rep.figure("case", T=c.T, V=c.V, Jt=c.Jt, rid=c.rid, max_ref=float(np.abs(c.ref).max()), det_step=c.det_step,
               pass_share=float(c.expected_mask.mean()))
    packed_mask = d.packed_fwd_mask()
    packed_words = _words(packed_mask)
    rep.check(np.array_equal(packed_words, c.expected_mask), "the packed training forward's J = 1 mask differs from the expected words")
    packed_det = {nm: d.packed_bwd(packed_mask, s) for nm, s in (("per_tap", _lib.SCATTER_PER_TAP), ("merge", _lib.SCATTER_MERGE))}
    for name, layout, jp, views in d.hand_overs:
        mask = _forward_checks(rep, d, name, layout, jp, views, packed_words)
        _backward_checks(rep, d, name, mask, packed_mask, packed_det)
    rep.done()


def test_forward_and_deterministic_backward_replayed_from_a_graph(dev):
    c = cases.get(GRAPH_CASE)
    d = OnDevice(c, dev)
    name, layout, jp, views = d.hand_overs[1]
    mask = d.fresh_mask()
    cubes = d.one_fwd(views, layout, jp, 1, False, mask).clone()
    eager = d.one_bwd(mask, True).clone()
    assert np.array_equal(_words(mask), c.expected_mask) and torch.count_nonzero(eager) > 500
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    gmask = d.fresh_mask()
    with torch.cuda.stream(st):
        d.one_bwd(gmask, True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            gcubes = d.one_fwd(views, layout, jp, 1, False, gmask)
            out = d.one_bwd(gmask, True)
    for _ in range(3):
        out.zero_()
        gcubes.zero_()
        gmask.fill_(0x5a5a)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gcubes, cubes) and torch.equal(gmask, mask) and torch.equal(out, eager)


def test_cabi_refusals_with_real_tensors(dev):
    """the refusals of tests/test_one_channel_grad_host.py with device buffers large enough that a library which misses one
    (and launches) reads and writes in bounds"""
    from selfpose3d_amd import _lib
    lib = _lib.load()
    hm = torch.zeros(2, 32, 8, 8, device=dev)
    cam = torch.zeros(2, 2, 64, device=dev)
    cen, val = torch.zeros(2, 3, device=dev), torch.ones(2, dtype=torch.uint8, device=dev)
    cubes = torch.zeros(2, 16, 4, 4, 4, device=dev)
    mask = torch.full((2, 64), 0x5a5a, dtype=torch.int16, device=dev)
    grad, acc, scale = torch.ones(2, 4, 4, 4, 4, device=dev), torch.zeros(2, 2, 8, 8, dtype=torch.int64, device=dev), torch.ones(1, device=dev)
    views = (C.c_void_p * 2)(hm.data_ptr(), hm.data_ptr())
    gs = (C.c_float * 3)(8000, 8000, 2000)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = _lib._stream(dev)
    ft, fb, fd = lib.sp3d_unproject_one_fwd_train, lib.sp3d_unproject_one_bwd, lib.sp3d_unproject_one_bwd_det
    for layout, jp in ((_lib.LAYOUT_PLANAR, 15), (_lib.LAYOUT_NHWC, 16)):
        for J in (2, 3):
            assert ft(views, layout, jp, p(cam), None, p(cen), p(val), p(cubes), None, p(mask), 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, s) == -4
        assert ft(views, layout | _lib.OUT_CHANNELS_LAST, jp, p(cam), None, p(cen), p(val), p(cubes), None, p(mask), 1, 2, 1, 8, 8,
                  4, 4, 4, gs, 96, 72, s) == -4
        for bf in (_lib.OUT_BF16, _lib.HM_BF16):
            assert ft(views, layout | bf, jp, p(cam), None, p(cen), p(val), p(cubes), None, p(mask), 1, 2, 4, 8, 8, 4, 4, 4, gs, 96, 72, s) == -4
        assert ft(views, layout, jp, p(cam), None, p(cen), p(val), p(cubes), None, p(mask), 1, 2, 4, 8, 1, 4, 4, 4, gs, 96, 72, s) == -4
        assert ft(views, layout, jp, p(cam), None, p(cen), p(val), p(cubes), None, None, 1, 2, 4, 8, 8, 4, 4, 4, gs, 96, 72, s) == -2
    assert fb(p(cam), None, p(cen), p(val), p(grad), 256, p(mask), p(acc), 1, 1, 2, 8, 1, 4, 4, 4, gs, 96, 72, s) == -4
    assert fb(p(cam), None, p(cen), p(val), p(grad), 63, p(mask), p(acc), 1, 1, 2, 8, 8, 4, 4, 4, gs, 96, 72, s) == -1
    assert fb(p(cam), None, p(cen), p(val), None, 256, p(mask), p(acc), 1, 1, 2, 8, 8, 4, 4, 4, gs, 96, 72, s) == -2
    assert fd(p(cam), None, p(cen), p(val), p(grad), 256, None, p(acc), p(scale), 1, 1, 2, 8, 8, 4, 4, 4, gs, 96, 72, s) == -2
    assert fd(p(cam), None, p(cen), p(val), p(grad), 256, p(mask), p(acc), None, 1, 1, 2, 8, 8, 4, 4, 4, gs, 96, 72, s) == -2
    torch.cuda.synchronize(dev)
    assert not bool(cubes.any()) and not bool(acc.any()) and bool((mask == 0x5a5a).all())


# ---- ProjectLayer ----------------------------------------------------------------------------------------------------------
def _leaves(planar, nhwc, hand_over):
    """-> (leaf tensors that require a gradient, list[V] of (B,J,h,w) maps that are views of them, channel dim of a leaf).
    planar: the V tensors themselves; nhwc: ONE (V,B,h,w,jp) buffer, the maps being its channels-last views (a clone of such
    a view would be planar again)"""
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    if hand_over == "planar":
        src = [a.clone().requires_grad_(True) for a in planar]
        return src, src, 1
    buf = nhwc[0]._sp3d_packed[0].clone().requires_grad_(True)
    maps = nhwc_heatmap_views(buf, int(nhwc[0].shape[1]))
    assert maps[0].stride(1) == 1 and maps[0].stride(3) == buf.shape[-1]
    return [buf], maps, 4


def _only_channel(grad, rid, dim):
    """the gradient of a leaf is non-zero in channel rid and exactly zero in every other channel"""
    idx = [slice(None)] * grad.dim()
    idx[dim] = rid
    rest = grad.clone()
    rest[tuple(idx)] = 0
    return float(grad[tuple(idx)].abs().max()) > 0 and not bool(rest.any())


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
@pytest.mark.parametrize("B", [1, 2])
def test_project_layer_trains_through_the_slice_in_place(dev, monkeypatch, hand_over, B):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    cfg = load_config(None, **SMALL)
    meta, planar, nhwc = _small_scene(dev, B, 80 + B)
    rid = 2
    layer = ProjectLayer(cfg)
    layer.deterministic_backward = True
    spy = _PackSpy(monkeypatch)
    rng = np.random.default_rng(3)
    forms = [dict(), dict(want_grids=False, pad_channels=True), dict(want_grids=False, pad_channels=True, channels_last=True)]
    ws = [torch.from_numpy(rng.standard_normal((B, J, 24, 24, 8)).astype(np.float32)).to(dev) for J in (1, 4, 4)]
    grads, cubes = {}, {}
    for on in (True, False):
        layer.one_channel_grad = on
        grads[on], cubes[on] = [], []
        for kw, w in zip(forms, ws):
            clear_pack_cache()
            spy.calls = 0
            src, maps, chdim = _leaves(planar, nhwc, hand_over)
            c, _ = layer.get_voxel([a[:, rid:rid + 1] for a in maps], meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8], **kw)
            assert (spy.calls == 0) if on else (spy.calls >= 1), (on, kw, spy.calls)      # no re-tiling pass on the new path
            (c * w).sum().backward()
            assert not on or spy.calls == 0
            grads[on].append([a.grad.clone() for a in src])
            cubes[on].append(c.detach())
    for k in range(len(forms)):
        assert cubes[True][k].shape == cubes[False][k].shape and cubes[True][k].stride() == cubes[False][k].stride()
        assert torch.equal(cubes[True][k], cubes[False][k]), forms[k]
        for a, b in zip(grads[True][k], grads[False][k]):
            assert torch.equal(a, b), forms[k]
            assert _only_channel(a, rid, chdim), forms[k]                              # nothing outside the one channel
    print("one_channel_grad %s B=%d: max|grad| %.4g, nonzero pixels %d" % (hand_over, B, float(grads[True][0][0].abs().max()),
                                                                         int(torch.count_nonzero(grads[True][0][0]))))


@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
def test_the_inference_switch_alone_keeps_the_packed_gradient_path(dev, monkeypatch, hand_over):
    """one_channel on, one_channel_grad off: a heat-map gradient still re-tiles (the contract of
    tests/test_gpu_one_channel.py::test_project_layer_gradient_keeps_the_packed_path); and the new switch alone leaves the
    no-gradient call on the packed path"""
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache
    cfg = load_config(None, **SMALL)
    meta, planar, nhwc = _small_scene(dev, 2, 90)
    layer = ProjectLayer(cfg)
    spy = _PackSpy(monkeypatch)
    args = (meta, syn.SPACE_SIZE, [list(syn.SPACE_CENTER)], [24, 24, 8])
    layer.one_channel, layer.one_channel_grad = True, False
    clear_pack_cache()
    src, maps, chdim = _leaves(planar, nhwc, hand_over)
    c, _ = layer([a[:, 2:3] for a in maps], *args)
    assert spy.calls >= 1
    c.sum().backward()
    assert _only_channel(src[0].grad, 2, chdim)
    layer.one_channel, layer.one_channel_grad = False, True
    clear_pack_cache()
    spy.calls = 0
    with torch.no_grad():
        layer([a.detach()[:, 2:3] for a in maps], *args)
    assert spy.calls >= 1


# ---- the ROOTNET_ROOTHM root nets in train() mode ---------------------------------------------------------------------------
@pytest.mark.parametrize("hand_over", ["planar", "nhwc"])
def test_root_nets_train_switch_on_equals_off(dev, monkeypatch, hand_over):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
    from selfpose3d_amd.project_layer import clear_pack_cache
    B = 2
    cfg = load_config(None, **SMALL, NETWORK__ROOTNET_ROOTHM=True, NETWORK__ROOTNET_TRAIN_SYNTH=True)
    meta, planar, nhwc = _small_scene(dev, B, 95)
    soft = CuboidProposalNetSoft(cfg)
    syn.fill_parameters_deterministic(soft, seed=5, scale=0.05)
    soft.to(dev).train()
    plain = CuboidProposalNet(cfg)
    plain.load_state_dict(soft.state_dict())
    plain.to(dev).train()
    spy = _PackSpy(monkeypatch)
    w = torch.from_numpy(np.random.default_rng(4).standard_normal((B, 24, 24, 8)).astype(np.float32)).to(dev)
    for net in (plain, soft):
        net.project_layer.deterministic_backward = True
        got = {}
        for on in (True, False):
            net.project_layer.one_channel_grad = on
            net.zero_grad(set_to_none=True)
            clear_pack_cache()
            if net is soft:
                soft.generator = torch.Generator().manual_seed(7)
            src, maps, chdim = _leaves(planar, nhwc, hand_over)
            spy.calls = 0
            root_cubes = net(maps, meta)[0]
            calls = spy.calls
            (root_cubes * w).sum().backward()
            got[on] = (root_cubes.detach().clone(), [a.grad.clone() for a in src],
                       {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}, calls)
        name = type(net).__name__
        assert got[True][3] < got[False][3], (name, got[True][3], got[False][3])          # the root unprojection re-tiles no more
        assert torch.equal(got[True][0], got[False][0]), name
        rid = net.root_id
        for a, b in zip(got[True][1], got[False][1]):
            assert torch.equal(a, b), name
            assert _only_channel(a, rid, chdim), name
        assert got[True][2].keys() == got[False][2].keys() and len(got[True][2]) > 10
        for k in got[True][2]:
            assert torch.equal(got[True][2][k], got[False][2][k]), (name, k)
        print("root net %s %s: %d parameter gradients equal, max|d heat-map| %.4g" % (name, hand_over, len(got[True][2]),
                                                                                   float(got[True][1][0].abs().max())))
