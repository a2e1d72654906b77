"""The V2V inference plan (v2v_net._FoldedV2V), layer by layer and over whole volumes, against a float64 evaluation of the
MODULE's own math, at the configurations the project runs.

One real plan forward per configuration is captured: the plan's layer methods (_front_fft, _front_zspectrum, _res, _pool,
_up2x) and the head kernel are wrapped on the plan object, the _lib entry points are wrapped to record which kernel each
layer took, and the inputs (residuals and skips included) are cloned BEFORE each call - channel_shift_act_ and irfft3d_ work
in place and the FFT input buffer is reused between calls.  Each layer is then recomputed in float64 from the module's
parameters (not from the plan's BatchNorm-folded weights, so the folding is under test too), starting from the plan's own
fp32 input to that layer: errors do not pile up from layer to layer and each bound stays tight.  Where the opening conv
starts from the fused unprojection's z-spectrum, the referee's input is the CPU oracle's cubes for the same heat-maps.

Parameters: tests/golden_io.he_fill, BatchNorm statistics far from the identity (running_var in [0.1, 10], running_mean in
[-1, 1], gamma in [0.5, 2]), each conv rescaled once so that its output has unit spread on a small calibration input (the
activations then stay O(1) through the 20 layers).  Every layer's float64 output is asserted to be O(1) and 10-90 % positive
where it ends in a ReLU, so that the comparison has signal.  Before each captured forward the caching allocator's free
blocks are filled with NaN: a tile that a kernel never writes cannot pass by holding an earlier run's answer.

SP3D_V2V_F64_RECORD=<file.json>: write the measured per-layer and end-to-end errors (profiles/r07_v2v_plan_f64.json)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import golden_io as gio

pytestmark = pytest.mark.gpu

# ---- census: the kernel every layer takes, from the dispatch rules of v2v_net.py --------------------------------------------
# v2v_net.conv3_route on channels-last activations with the default switches: 16|32 -> 32 at full resolution ->
# conv3_split_; 32|64 -> 64 (16-column split) -> wino_fused_conv3d_ (split64); 64|128 -> 128 have no split, C >= 128 or
# 64*T*C*4 <= 160e6 at every shape below -> the quarter-resolution tier: conv3_split128_ where QUARTER_FORM says so, else
# wino_conv3d_ (the three launches, what TAIL names).  _FoldedV2V._pool: channels-last, C % 4 == 0, even sides ->
# maxpool2x.  _FoldedV2V._up2x: 64 output channels -> upsample2x_.  _FoldedV2V._tail: the 32-channel up-sampling + 1^3
# output conv -> upsample2x_head_.
# (layer, kernels in call order, input channels, resolution divisor of the input)
TAIL = [
    ("front_res", ("conv3_split_", "conv3_split_"), 16, 1),
    ("skip_res1", ("conv3_split_", "conv3_split_"), 32, 1),
    ("pool1", ("maxpool2x",), 32, 1),
    ("encoder_res1", ("wino_fused_conv3d_", "wino_fused_conv3d_"), 32, 2),
    ("skip_res2", ("wino_fused_conv3d_", "wino_fused_conv3d_"), 64, 2),
    ("pool2", ("maxpool2x",), 64, 2),
    ("encoder_res2", ("wino_conv3d_", "wino_conv3d_"), 64, 4),
    ("mid_res", ("wino_conv3d_", "wino_conv3d_"), 128, 4),
    ("decoder_res2", ("wino_conv3d_", "wino_conv3d_"), 128, 4),
    ("decoder_upsample2", ("upsample2x_",), 128, 4),
    ("decoder_res1", ("wino_fused_conv3d_", "wino_fused_conv3d_"), 64, 2),
    ("head", ("upsample2x_head_",), 64, 2),
]
# the opening 7^3 conv (_FoldedV2V._run, _front_zspectrum, _front_fft)
FRONTS = {
    "zspectrum": ("cfft2d_88_tiled", "freq_contract", "cfft2d_", "zdft_inv_cl"),          # TiledZSpectrum (fused unprojection)
    "zdft_cl": ("zdft_fwd_cl", "cfft2d_", "freq_contract", "cfft2d_", "zdft_inv_cl"),     # channels-last 16-channel cubes
    "rfft": ("rfft3d", "freq_contract", "irfft3d_", "crop_shift_act_cl"),               # padded planar buffer / generic
}
# the form of the quarter-resolution tier (encoder_res2, mid_res, decoder_res2) per configuration, written out: the direct
# kernel on grids of whole 5x5x5 blocks, at most 64 of them (_lib.quarter_direct_covers) - 20x20x5 at B = 1, 2 and 4 (16, 32
# and, on the boundary of the rule, 64 blocks); the three launches at 12x12x3 and 16^3 (ragged) and at 40x40x10, B = 2 (256 blocks)
QUARTER_LAYERS = ("encoder_res2", "mid_res", "decoder_res2")
QUARTER_FORM = {
    "R1_b4": "conv3_split128_", "R2_b1": "conv3_split128_", "R2_b2": "conv3_split128_", "R3_b1": "conv3_split128_",
    "R3_b4": "conv3_split128_", "R4_b2": "wino_conv3d_", "R5_b2": "wino_conv3d_",
    "P1_p1": "wino_conv3d_", "P1_p3": "wino_conv3d_", "P1_p8": "wino_conv3d_", "P1_p11": "wino_conv3d_",
}
LIB_ENTRIES = ("conv3_split_", "wino_fused_conv3d_", "wino_conv3d_", "conv3_split128_", "channel_shift_act_", "upsample2x_", "upsample2x_head_",
               "maxpool2x", "crop_shift_act_cl", "zdft_fwd_cl", "zdft_inv_cl", "freq_contract", "freq_contract_ty", "rfft3d",
               "irfft3d_", "cfft2d_", "cfft2d_88_tiled")

# id: (net, grid, batch, front kind, channels of the front's input tensor, seed).  What each runs, with the input shape of
# every layer (B, C, X, Y, Z) from TAIL (C, X/d, Y/d, Z/d):
#   R1  V2VNet(15,1) in CuboidProposalNet, 80x80x20, B=4: fused z-spectrum front (the bench's path); conv3_split_ at
#       80x80x20, split64 32->64 and 64->64 at 40x40x10, conv3_split128_ 64->128 and 128->128 at 20x20x5, upsample2x_
#       20x20x5 -> 40x40x10, head 40x40x10 -> 80x80x20 (J=1)
#   R2  the same with fuse_zdft=False, B=1 and B=2: channels-last 16-channel cubes -> zdft_fwd_cl
#   R3  NETWORK.ROOTNET_ROOTHM: V2VNet(1,1), cin=1, channels-last 4-channel cubes -> generic rFFT front + crop_shift_act_cl,
#       J=1 head, B=1 and B=4
#   R4  V2VNet(15,1), 48x48x12, B=2: padded planar input, quarter resolution 12x12x3
#   R5  V2VNet(15,1), 160x160x40, B=2: conv3_split_ at 160x160x40, split64 at 80x80x20, wino_conv3d_ at 40x40x10
#   P1  V2VNet(15,15) in PoseRegressionNet.forward_batched, 64^3 cubes, P = 1, 3 (one chunk padded to 4), 8 and 11 (8 + a
#       ragged tail of 3 padded to 4): conv3_split_ at 64^3, split64 at 32^3, wino_conv3d_ at 16^3, head 32^3 -> 64^3 (J=15)
ROOT_CONFIGS = {
    "R1_b4": dict(J=15, roothm=False, cube=(80, 80, 20), B=4, front="zspectrum", fc=15, fuse=True, seed=701),
    "R2_b1": dict(J=15, roothm=False, cube=(80, 80, 20), B=1, front="zdft_cl", fc=16, fuse=False, seed=702),
    "R2_b2": dict(J=15, roothm=False, cube=(80, 80, 20), B=2, front="zdft_cl", fc=16, fuse=False, seed=703),
    "R3_b1": dict(J=15, roothm=True, cube=(80, 80, 20), B=1, front="rfft", fc=4, fuse=True, seed=704),
    "R3_b4": dict(J=15, roothm=True, cube=(80, 80, 20), B=4, front="rfft", fc=4, fuse=True, seed=705),
    "R4_b2": dict(J=15, roothm=False, cube=(48, 48, 12), B=2, front="rfft", fc=15, fuse=True, seed=706),
    "R5_b2": dict(J=15, roothm=False, cube=(160, 160, 40), B=2, front="rfft", fc=15, fuse=True, seed=707),
}
POSE_CONFIGS = {"P1_p1": (1, 1, 711), "P1_p3": (2, 2, 712), "P1_p8": (2, 4, 713), "P1_p11": (3, 4, 714)}   # (B, K, seed)


def expected_census(cid, front, fc, B, cube):
    X, Y, Z = cube
    rows = [("front", FRONTS[front], (B, fc, X, Y, Z))]
    for name, kernels, c, d in TAIL:
        if name in QUARTER_LAYERS:
            kernels = (QUARTER_FORM[cid],) * 2
        rows.append((name, kernels, (B, c, X // d, Y // d, Z // d)))
    return rows


# ---- bounds: max|got - f64| / max(1, max|f64|), measured on the MI355X (profiles/r07_v2v_plan_f64.json) --------------------
# Worst measured over R1-R5 and P1 (the fp32 module through the library's convolutions, same inputs, in brackets):
#   opening conv 5.69e-7 (R3 B=4; 6.2e-7), conv3_split_ 1.57e-6 (P1 P=8 front_res; 2.0e-6), split64 7.67e-7 (R2 B=1 skip_res2;
#   1.6e-6), wino_conv3d_ 6.95e-7 (R3 B=4 decoder_res2; 2.6e-6), upsample2x_ 5.25e-7 (R5; 4.2e-7), head 3.05e-7 (P1 P=8;
#   3.9e-7), whole net 2.0e-6 (P1 P=8; 2.4e-6; the R1 graph replay 1.02e-6).  Each bound is <= 3x its measured worst: a wrong
#   tile, brick, channel scale or folded BatchNorm term is off by >= 1e-3 of the range (test_comparison_rejects_altered_outputs).
# With the quarter-resolution forms told apart (profiles/r17_v2v_plan_f64.json): conv3_split128_ 1.17e-6 (R3 B=4 decoder_res2),
# wino_conv3d_ 7.52e-7 (P1 P=11 mid_res).
BOUNDS = {
    "front": 1.7e-6,
    "conv3_split_": 4.7e-6,
    "wino_fused_conv3d_": 2.3e-6,
    "wino_conv3d_": 2.0e-6,
    "conv3_split128_": 2.0e-6,           # the bound of the other form of the same layers (tests/test_gpu_quarter_direct.py, tests/conv_sweep_cases.py)
    "upsample2x_": 1.5e-6,
    "upsample2x_head_": 9.0e-7,
}
E2E_BOUND = 6.0e-6


def bound_of(layer, kernels):
    if layer == "front":
        return BOUNDS["front"]
    return BOUNDS[kernels[0]]


# ---- parameters ---------------------------------------------------------------------------------------------------------
def fill_far_from_identity(net, seed):
    """he_fill, then BatchNorm statistics far from the identity, then each conv rescaled (weights and bias, one factor per
    output channel) so that its output has unit spread on a small calibration input - in one forward, in layer order"""
    from selfpose3d_amd.v2v_net import V2VNet
    assert isinstance(net, V2VNet)
    gio.he_fill(net, seed)
    rng = np.random.default_rng(seed + 1)
    with torch.no_grad():
        for _, m in sorted(net.named_modules()):
            if isinstance(m, torch.nn.modules.batchnorm._NormBase):
                c = m.num_features
                m.running_var.copy_(torch.from_numpy(10.0 ** rng.uniform(-1.0, 1.0, c)).float())
                m.running_mean.copy_(torch.from_numpy(rng.uniform(-1.0, 1.0, c)).float())
                m.weight.copy_(torch.from_numpy(2.0 ** rng.uniform(-1.0, 1.0, c)).float())
    net.eval()
    hooks = []

    def unit(m, _inp, out):
        s = out.std(dim=(0, 2, 3, 4)).clamp_min(1e-6)
        shape = (1, -1, 1, 1, 1) if isinstance(m, torch.nn.ConvTranspose3d) else (-1, 1, 1, 1, 1)
        m.weight.div_(s.view(shape))
        m.bias.div_(s)
        return out / s.view(1, -1, 1, 1, 1)
    for m in net.modules():
        if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
            hooks.append(m.register_forward_hook(unit))
    g = torch.Generator().manual_seed(seed)
    cin = net.front_layers[0].block[0].in_channels
    with torch.no_grad():
        net(torch.rand((2, cin, 16, 16, 8), generator=g) * 0.6)
    for h in hooks:
        h.remove()
    net.invalidate_plan()
    return net


# ---- allocator poisoning --------------------------------------------------------------------------------------------------
def poison_free_blocks(dev):
    """fill the caching allocator's free blocks with NaN (allocate, fill, free) without growing its reservation"""
    torch.cuda.synchronize(dev)
    keep = []
    size = 1 << 36
    while size >= (1 << 20) and len(keep) < 256:
        st = torch.cuda.memory_stats(dev)
        free = st["reserved_bytes.all.current"] - st["allocated_bytes.all.current"]
        if free < (1 << 20):
            break
        size = min(size, free)
        before = torch.cuda.memory_reserved(dev)
        t = torch.empty(size // 4, dtype=torch.float32, device=dev)
        if torch.cuda.memory_reserved(dev) > before:          # no free block this large: a fresh reservation, give it back
            del t
            torch.cuda.empty_cache()
            size //= 2
            continue
        t.fill_(float("nan"))
        keep.append(t)
    del keep
    torch.cuda.synchronize(dev)


# ---- capture ------------------------------------------------------------------------------------------------------------
class Capture:
    """records every layer of the plan's forwards: name, kernels, input shape, clones of inputs and output"""

    def __init__(self, mp, plan, lib, soft_argmax=False):
        self.calls = []            # one list of layer records per plan forward
        self.cur = None
        self.pool_n = 0
        self.soft = []
        for ent in LIB_ENTRIES:
            mp.setattr(lib, ent, self._kernel(ent, getattr(lib, ent)))
        mp.setattr(plan, "_front_fft", self._front(plan._front_fft))
        mp.setattr(plan, "_front_zspectrum", self._front(plan._front_zspectrum))
        mp.setattr(plan, "_res", self._res(plan._res))
        mp.setattr(plan, "_pool", self._pool(plan._pool))
        mp.setattr(plan, "_up2x", self._up(plan._up2x))
        if soft_argmax:
            inner = lib.soft_argmax_grid

            def sa(y, centers, *a, **k):
                self.soft.append((int(y.shape[0]), y.data_ptr(), int(centers.shape[0])))
                return inner(y, centers, *a, **k)
            mp.setattr(lib, "soft_argmax_grid", sa)

    def _open(self, name, shape, ins):
        rec = dict(layer=name, kernels=[], shape=tuple(int(v) for v in shape), ins=ins, out=None)
        assert self.cur is None, ("nested layer", name, self.cur["layer"])
        self.cur = rec
        self.calls[-1].append(rec)
        return rec

    def _close(self, rec, out):
        rec["out"] = out.clone()
        rec["ptr"] = out.data_ptr()
        self.cur = None
        return out

    def _kernel(self, ent, fn):
        def call(*a, **k):
            if ent == "upsample2x_head_" and self.cur is None:          # the head: a layer and a kernel in one call
                x, skip = a[0], a[3]
                rec = self._open("head", x.shape, dict(x=x.clone(), skip=skip.clone()))
                rec["kernels"].append(ent)
                return self._close(rec, fn(*a, **k))
            if self.cur is not None:
                self.cur["kernels"].append(ent)
            return fn(*a, **k)
        return call

    def _front(self, fn):
        def call(x, w0, s0):
            self.calls.append([])
            self.pool_n = 0
            cin = int(w0.shape[1])
            ins = dict(x=None if not torch.is_tensor(x) else x[:, :cin].clone())
            rec = self._open("front", x.shape, ins)
            return self._close(rec, fn(x, w0, s0))
        return call

    def _res(self, fn):
        def call(x, name):
            rec = self._open(name, x.shape, dict(x=x.clone()))
            return self._close(rec, fn(x, name))
        return call

    def _pool(self, fn):
        def call(x):
            self.pool_n += 1
            rec = self._open(f"pool{self.pool_n}", x.shape, dict(x=x.clone()))
            return self._close(rec, fn(x))
        return call

    def _up(self, fn):
        def call(x, name, skip):
            rec = self._open(name, x.shape, dict(x=x.clone(), skip=skip.clone()))
            return self._close(rec, fn(x, name, skip))
        return call


# ---- float64 referee ----------------------------------------------------------------------------------------------------
def conv3d_slabs(x, w, b, budget=1 << 30):
    """'same' float64 Conv3d (odd cubic kernel, stride 1) over x-slabs with a k//2 halo: the im2col of the library's
    float64 path holds C * k^3 values per output voxel of one sample, so each call sees at most `budget` bytes of it"""
    k = int(w.shape[2])
    p = k // 2
    B, C, X, Y, Z = x.shape
    xp = F.pad(x, (p, p, p, p, p, p))
    per_plane = C * k ** 3 * Y * Z * 8
    slab = max(1, min(X, budget // max(per_plane, 1)))
    out = torch.empty((B, int(w.shape[0]), X, Y, Z), dtype=x.dtype, device=x.device)
    for x0 in range(0, X, slab):
        x1 = min(X, x0 + slab)
        out[:, :, x0:x1] = F.conv3d(xp[:, :, x0:x1 + 2 * p], w, b)
    return out


class Referee:
    """float64 evaluation of the module's layers (a float64 copy of the fp32 net, eval mode)"""

    def __init__(self, net):
        from selfpose3d_amd.v2v_net import V2VNet
        cin = net.front_layers[0].block[0].in_channels
        cout = net.output_layer.out_channels
        r = V2VNet(cin, cout)
        r.load_state_dict(net.state_dict())
        self.r = r.double().to(net.output_layer.weight.device).eval()
        self.net = net

    def front(self, x):
        blk = self.r.front_layers[0].block
        return F.relu(blk[1](conv3d_slabs(x, blk[0].weight, blk[0].bias)))

    def res(self, name, x):
        m = self.r.front_layers[1] if name == "front_res" else getattr(self.r.encoder_decoder, name)
        rb = m.res_branch
        h = F.relu(rb[1](conv3d_slabs(x, rb[0].weight, rb[0].bias)))
        y = rb[4](conv3d_slabs(h, rb[3].weight, rb[3].bias))
        s = x if len(m.skip_con) == 0 else m.skip_con(x)
        return F.relu(y + s)

    def up(self, name, x, skip):
        return getattr(self.r.encoder_decoder, name)(x) + skip

    def head(self, x, skip):
        return self.r.output_layer(self.r.encoder_decoder.decoder_upsample1(x) + skip)

    def layer(self, rec, x=None):
        """float64 output of one captured layer, from `x` (float64) or from the plan's own input to it"""
        name = rec["layer"]
        ins = rec["ins"]
        x = ins["x"].double() if x is None else x
        if name == "front":
            return self.front(x)
        if name.startswith("pool"):
            return F.max_pool3d(x, 2, 2)
        if name == "head":
            return self.head(x, ins["skip"].double())
        if name.startswith("decoder_upsample"):
            return self.up(name, x, ins["skip"].double())
        return self.res(name, x)

    def chain(self, x):
        """the whole net in float64, layer by layer (v2v_net.py _EncDec.forward)"""
        x = self.front(x)
        x = self.res("front_res", x)
        s1 = self.res("skip_res1", x)
        x = self.res("encoder_res1", F.max_pool3d(x, 2, 2))
        s2 = self.res("skip_res2", x)
        x = self.res("encoder_res2", F.max_pool3d(x, 2, 2))
        x = self.res("decoder_res2", self.res("mid_res", x))
        x = self.up("decoder_upsample2", x, s2)
        x = self.res("decoder_res1", x)
        return self.head(x, s1)

    def eager32(self, rec, x=None):
        """the same layer through the fp32 module (library convolutions), for the yardstick"""
        n = self.net
        name, ins = rec["layer"], rec["ins"]
        x = ins["x"] if x is None else x
        with torch.no_grad():
            if name == "front":
                xc = x.contiguous(memory_format=torch.channels_last_3d)
                return n.front_layers[0](xc)
            if name.startswith("pool"):
                return F.max_pool3d(x, 2, 2)
            if name == "head":
                return n.output_layer(n.encoder_decoder.decoder_upsample1(x) + ins["skip"])
            if name.startswith("decoder_upsample"):
                return getattr(n.encoder_decoder, name)(x) + ins["skip"]
            m = n.front_layers[1] if name == "front_res" else getattr(n.encoder_decoder, name)
            return m(x)


def rel_err(got, ref):
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def check_layers(tag, calls, census, referee, front_inputs, records):
    """compare every captured layer of every forward with the float64 referee; census, signal and bound checks -> list of
    the layers over their bound (asserted by the caller once the measured errors are written)"""
    over = []
    assert len(calls) >= 1, tag
    for ci, layers in enumerate(calls):
        got_census = [(r["layer"], tuple(r["kernels"]), r["shape"]) for r in layers]
        want = census[ci]
        for g_row, w_row in zip(got_census, want):
            assert g_row == w_row, (tag, ci, "layer took another path than this file pins", g_row, w_row)
        assert len(got_census) == len(want), (tag, ci, got_census, want)
        for rec in layers:
            name = rec["layer"]
            x = front_inputs[ci] if (name == "front" and rec["ins"]["x"] is None) else None
            if name.startswith("pool"):
                assert torch.equal(rec["out"], F.max_pool3d(rec["ins"]["x"], 2, 2)), (tag, ci, name)
                continue
            ref = referee.layer(rec, None if x is None else x.double())
            out = rec["out"]
            assert out.shape == ref.shape, (tag, name, out.shape, ref.shape)
            assert bool(torch.isfinite(out).all()), (tag, ci, name, "non-finite output (a tile left unwritten?)")
            e = rel_err(out, ref)
            e32 = rel_err(referee.eager32(rec, x), ref)
            amax = float(ref.abs().max())
            pos = float((ref > 0).double().mean())
            records.append(dict(config=tag, call=ci, layer=name, kernels=list(rec["kernels"]), shape=list(rec["shape"]),
                                err=e, eager_fp32_err=e32, max_abs=amax, frac_pos=pos))
            # signal: O(1) outputs, and a ReLU that is neither dead nor the identity
            if not 0.3 <= amax <= 300.0:
                over.append((tag, ci, name, "output range", amax))
            if name != "head" and not 0.1 <= pos <= 0.9:
                over.append((tag, ci, name, "fraction of positive outputs", pos))
            b = bound_of(name, rec["kernels"])
            if not e <= b:
                over.append((tag, ci, name, rec["kernels"], e, b, e32))
            del ref
    return over


def write_records(records):
    path = os.environ.get("SP3D_V2V_F64_RECORD")
    if not path:
        return
    old = []
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    with open(path, "w") as f:
        json.dump(old + records, f, indent=1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _root_setup(dev, c):
    from oracle import oracle
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    kw = dict(MULTI_PERSON__INITIAL_CUBE_SIZE=list(c["cube"]))
    if c["roothm"]:
        kw["NETWORK__ROOTNET_ROOTHM"] = True
    cfg = load_config(None, **kw)
    net = CuboidProposalNet(cfg)
    assert tuple(net.cube_size) == tuple(c["cube"]) and net.rootnet_roothm == c["roothm"]
    fill_far_from_identity(net.v2v_net, c["seed"])
    net.eval().to(dev).use_channels_last(True)
    net.v2v_net.fuse_zdft = c["fuse"]
    img = [int(v) for v in cfg.NETWORK.IMAGE_SIZE]
    w, h = [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]
    V, B = int(cfg.DATASET.CAMERA_NUM), c["B"]
    meta = syn.make_meta(B, V, img)
    hms = syn.random_heatmaps(B, V, c["J"], h, w, seed=c["seed"])
    # the oracle's cubes of what the net's V2V reads (root-joint channel only under ROOTNET_ROOTHM)
    rh = [x[:, net.root_id:net.root_id + 1].contiguous() if c["roothm"] else x for x in hms]
    cam = pack_cameras(meta, B, img)
    centers = np.repeat(np.asarray([net.grid_center], np.float32), B, 0)
    cubes, _ = oracle.unproject_fwd([x.numpy() for x in rh], cam, centers, np.ones(B, np.uint8), net.grid_size, net.cube_size,
                                    img, want_grids=False)
    return net, [x.to(dev) for x in hms], meta, torch.from_numpy(cubes).to(dev)


def _capture_root(monkeypatch, net, hms, meta, dev):
    from selfpose3d_amd import _lib
    from selfpose3d_amd.v2v_net import _FoldedV2V
    v2v = net.v2v_net
    if v2v._plan is None:
        v2v._plan = _FoldedV2V(v2v)
    poison_free_blocks(dev)
    with monkeypatch.context() as mp:
        cap = Capture(mp, v2v._plan, _lib)
        with torch.no_grad():
            rc, gc = net(hms, meta)
        torch.cuda.synchronize(dev)
    return cap, rc.clone(), gc.clone()


@pytest.mark.parametrize("cid", list(ROOT_CONFIGS))
def test_root_net_plan_layers_vs_float64(dev, cid, monkeypatch):
    c = ROOT_CONFIGS[cid]
    net, hms, meta, cubes = _root_setup(dev, c)
    cap, rc, _ = _capture_root(monkeypatch, net, hms, meta, dev)
    assert len(cap.calls) == 1, len(cap.calls)
    census = [expected_census(cid, c["front"], c["fc"], c["B"], c["cube"])]
    ref = Referee(net.v2v_net)
    records = []
    # the fused front's referee input: the oracle's whole-volume cubes for the same heat-maps
    over = check_layers(cid, cap.calls, census, ref, [cubes], records)
    # end to end: the plan's whole output volume against the float64 net on the same input cubes
    front_in = cap.calls[0][0]["ins"]["x"]
    x_in = cubes if front_in is None else front_in
    if front_in is not None and c["front"] != "zspectrum":
        # the unprojection's cubes the plan read are the oracle's (whole volume, fp32 rounding of the same sums)
        assert float((front_in - cubes).abs().max()) <= 1e-5, cid
    want = ref.chain(x_in.double())
    with torch.no_grad():
        net.v2v_net.fused_inference = False
        eager = net.v2v_net(x_in.contiguous(memory_format=torch.channels_last_3d))
        net.v2v_net.fused_inference = True
    e, e32 = rel_err(rc, want.squeeze(1)), rel_err(eager, want)
    rec = dict(config=cid, call=0, layer="end_to_end", err=e, eager_fp32_err=e32, max_abs=float(want.abs().max()))
    if cid == "R1_b4":
        # the bench's replay of the same step
        from selfpose3d_amd.graphs import GraphedRootNet
        gr = GraphedRootNet(net, hms, meta)
        poison_free_blocks(dev)
        grc, _ = gr()
        torch.cuda.synchronize(dev)
        rec["graph_err"] = rel_err(grc, want.squeeze(1))
        del gr
    records.append(rec)
    write_records(records)
    assert not over, over
    assert e <= E2E_BOUND and rec.get("graph_err", 0.0) <= E2E_BOUND, rec
    del cap, ref, want
    torch.cuda.empty_cache()


@pytest.mark.parametrize("cid", list(POSE_CONFIGS))
def test_pose_net_plan_layers_vs_float64(dev, cid, monkeypatch):
    from selfpose3d_amd import _lib
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.pose_regression_net import PoseRegressionNet
    from selfpose3d_amd.v2v_net import _FoldedV2V
    B, K, seed = POSE_CONFIGS[cid]
    cfg = load_config(None)
    net = PoseRegressionNet(cfg)
    fill_far_from_identity(net.v2v_net, seed)
    net.eval().to(dev).use_channels_last(True)
    img = [int(v) for v in cfg.NETWORK.IMAGE_SIZE]
    w, h = [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]
    V, J = int(cfg.DATASET.CAMERA_NUM), int(cfg.NETWORK.NUM_JOINTS)
    meta = syn.make_meta(B, V, img)
    hms = [x.to(dev) for x in syn.random_heatmaps(B, V, J, h, w, seed=seed)]
    g = torch.Generator().manual_seed(seed)
    gc = torch.zeros(B, K, 5)
    gc[..., 0] = (torch.rand(B, K, generator=g) - 0.5) * 4000
    gc[..., 1] = (torch.rand(B, K, generator=g) - 0.5) * 4000
    gc[..., 2] = 800 + torch.rand(B, K, generator=g) * 400
    if B * K in (4, 12):
        gc[B - 1, K - 1, 3] = -1.0                               # P = 3 and P = 11: one invalid proposal
    P = int((gc[..., 3] >= 0).sum())
    v2v = net.v2v_net
    v2v._plan = _FoldedV2V(v2v)
    poison_free_blocks(dev)
    with monkeypatch.context() as mp:
        cap = Capture(mp, v2v._plan, _lib, soft_argmax=True)
        with torch.no_grad():
            pred = net.forward_batched(hms, meta, gc.to(dev), max_cubes_per_call=8)
        torch.cuda.synchronize(dev)
    X, Y, Z = net.cube_size
    sizes = [min(8, P - s) for s in range(0, P, 8)]
    padded = [1 << (n - 1).bit_length() for n in sizes]
    assert [r[0] for r in cap.soft] == sizes and [r[2] for r in cap.soft] == sizes, (cap.soft, sizes)
    census = [expected_census(cid, "rfft", J, m, (X, Y, Z)) for m in padded]
    assert len(cap.calls) == len(sizes)
    # the padding cube's output never reaches the caller: the soft-argmax reads the first n cubes of each chunk's output
    for (n, ptr, _), layers in zip(cap.soft, cap.calls):
        assert layers[-1]["layer"] == "head" and layers[-1]["ptr"] == ptr
        assert layers[-1]["out"].shape[0] >= n
    assert pred.shape == (B, K, J, 3)
    live = gc[..., 3] >= 0
    assert bool((pred[~live.to(dev)] == 0).all()) and bool(torch.isfinite(pred).all())
    ref = Referee(v2v)
    records = []
    over = check_layers(cid, cap.calls, census, ref, [None] * len(sizes), records)
    for ci, layers in enumerate(cap.calls):
        x_in = layers[0]["ins"]["x"]
        want = ref.chain(x_in.double())
        with torch.no_grad():
            v2v.fused_inference = False
            eager = v2v(x_in.contiguous(memory_format=torch.channels_last_3d))
            v2v.fused_inference = True
        e, e32 = rel_err(layers[-1]["out"], want), rel_err(eager, want)
        rec = dict(config=cid, call=ci, layer="end_to_end", err=e, eager_fp32_err=e32, max_abs=float(want.abs().max()))
        records.append(rec)
    write_records(records)
    assert not over, over
    for rec in records:
        if rec["layer"] == "end_to_end":
            assert rec["err"] <= E2E_BOUND, rec
    del cap, ref
    torch.cuda.empty_cache()


def test_comparison_rejects_altered_outputs(dev, monkeypatch):
    """teeth: the comparison with the bounds above rejects three altered copies of captured R2 outputs - one channel
    scaled by 1.01, the 4x4x4 brick at the far (x, y, z) corner zeroed, one channel shifted by 1e-3 of the range"""
    c = ROOT_CONFIGS["R2_b1"]
    net, hms, meta, cubes = _root_setup(dev, c)
    cap, _, _ = _capture_root(monkeypatch, net, hms, meta, dev)
    ref = Referee(net.v2v_net)
    seen = set()
    for rec in cap.calls[0]:
        if rec["layer"] not in ("front", "front_res", "encoder_res1", "mid_res", "decoder_upsample2", "head"):
            continue
        want = ref.layer(rec, cubes.double() if rec["ins"]["x"] is None else None)
        out = rec["out"]
        b = bound_of(rec["layer"], rec["kernels"])
        assert rel_err(out, want) <= b
        ch = int(want.abs().amax(dim=(0, 2, 3, 4)).argmax())
        rng = float(want[:, ch].max() - want[:, ch].min())
        a = out.clone()
        a[:, ch] *= 1.01
        bb = out.clone()
        bb[:, :, -4:, -4:, -4:] = 0.0
        cc = out.clone()
        cc[:, ch] += 1e-3 * rng
        for kind, alt in (("scaled", a), ("corner", bb), ("shift", cc)):
            assert not torch.equal(alt, out), (rec["layer"], kind)
            e = rel_err(alt, want)
            assert e > b, (rec["layer"], kind, e, b)
        seen.add(rec["layer"])
    assert seen == {"front", "front_res", "encoder_res1", "mid_res", "decoder_upsample2", "head"}, seen
