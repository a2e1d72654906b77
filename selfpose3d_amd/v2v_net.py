"""V2V 3D encoder-decoder as a plain PyTorch-ROCm module (MIOpen convolutions).

Architecture and ``state_dict`` key names follow the reference's
/root/reference/lib/models/v2v_net.py:10-144 so its checkpoints load unchanged
(``front_layers.0.block.0.weight``, ``encoder_decoder.encoder_res1.res_branch.0.weight`` ...):
7^3 conv(Cin->16) -> Res(16->32) -> [pool2, Res(32->64)] -> [pool2, Res(64->128)] -> Res(128)
-> Res(128) -> ConvT2(128->64) (+skip Res(64)) -> Res(64) -> ConvT2(64->32) (+skip Res(32))
-> 1^3 conv(32->Cout).  north_star keeps this stack on the framework's conv kernels; the
hand-written HIP work of this repo is the unprojection feeding it.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F


def _bn(c):
    # nn.BatchNorm3d (same parameters / buffers / state_dict keys) that can keep the statistics of GROUPS of samples apart
    # while a GroupSpec is attached in train mode: all candidate slots of the training pose net in one call (grouped_bn.py)
    from .grouped_bn import GroupedBatchNorm3d
    return GroupedBatchNorm3d(c)


def _grouped(bn, training: bool) -> bool:
    return training and getattr(bn, "groups", None) is not None


def fft_len(n: int) -> int:
    """smallest even m >= n whose prime factors are <= 13 (rocFFT radices) and that has at most ONE distinct odd prime
    factor: mixed odd radices are slow in rocFFT (72 beats 70 = 2*5*7 and 88 = 8*11 beats 90 = 2*9*5 by more than
    their size ratio, tools/exp_fftconv.py)"""
    m = n + (n & 1)
    while True:
        r, odd = m, 0
        for q in (2, 3, 5, 7, 11, 13):
            if q > 2 and r % q == 0:
                odd += 1
            while r % q == 0:
                r //= q
        if r == 1 and odd <= 1:
            return m
        m += 2


def is_cl(t) -> bool:
    """channels-last (and not also plain-contiguous, as a 1x1x1 weight or a one-channel tensor is in both formats)"""
    return t.is_contiguous(memory_format=torch.channels_last_3d) and not t.is_contiguous()


def pad_cin(x, w):
    """(x, w) of a conv with the input-channel count rounded up to a multiple of 4, or to what x already carries (zero
    input channels x zero weight slices: same math); see PadCinConv3d"""
    cin, have = w.shape[1], x.shape[1]
    target = have if have > cin else ((cin + 3) // 4 * 4 if cin >= 3 else cin)
    if target != cin:
        w = F.pad(w, (0, 0, 0, 0, 0, 0, 0, target - cin))
    if have < target:
        x = F.pad(x, (0, 0, 0, 0, 0, 0, 0, target - have))
    return x, w


def conv3_route(cin, cout, shape, winograd=True, wino_split=True, direct_conv=True, quarter_direct=True) -> str:
    """Which kernel a 3x3x3 layer (cin -> cout) of the plan takes on a channels-last input of ``shape`` = (B, X, Y, Z)
    with its weights on the GPU: the name of the _lib entry point, or "library" (the library's conv + channel_shift_act_).
    Wide layers on small grids (the 1/4- and 1/2-resolution blocks: a GEMM with few rows, where MIOpen's implicit-GEMM
    kernels drop to ~60 TFLOP/s) go through Winograd F(2x2x2,3x3x3): HIP input/output transforms around one batched
    rocBLAS GEMM, 2.1x faster at (4,128,20,20,5) and 1.2x at (4,64,40,40,10) (tools/exp_wino.py); the rule keeps the
    transformed tensor (64*T*C floats) within reach of the Infinity Cache, beyond which the transforms eat the gain.
    Each form of the quarter-resolution tier has its name: "conv3_split128_", the direct kernel, with ``quarter_direct`` on the
    grids _lib.quarter_direct_covers (41 instead of 49.5 us per 128 -> 128 layer at (4,128,20,20,5)), and
    "wino_conv3d_", the three Winograd launches, everywhere else.  Reads no environment: the switches are the caller's."""
    from . import _lib
    B, X, Y, Z = shape
    full = cout == 32 and cin in (16, 32)                  # the full-resolution layers
    if not winograd or not (cin >= 64 or full or (cout == 64 and cin == 32)):
        return "library"
    if wino_split and cout == 64 and cin in (32, 64):
        # half-resolution layers in one launch (16-column split): 80 us instead of 115 at (4,64,40,40,10), 44 instead of
        # 78 (MIOpen) at (4,32->64,40,40,10)
        return "wino_fused_conv3d_"
    T = B * ((X + 1) // 2) * ((Y + 1) // 2) * ((Z + 1) // 2)
    if cin >= 128 or (cin >= 64 and 64 * T * cin * 4 <= 160e6):
        return "conv3_split128_" if quarter_direct and _lib.quarter_direct_covers(B, cin, cout, X, Y, Z) else "wino_conv3d_"
    if full and wino_split and direct_conv:
        # implicit GEMM with exact three-piece bf16 splits: no Winograd transforms (which made the fused kernel
        # VALU-bound); 155 vs 163 us (ReLU), 159 vs 182 us (residual) at (4,32,80,80,20)
        return "conv3_split_"
    if full:
        # the transformed tensor would be hundreds of MB, so everything (transforms, v_mfma_f32_32x32x2_f32 products - or
        # their bf16 splits under wino_split -, epilogue) happens in one kernel: 225 us instead of 345 us at
        # (4,32,80,80,20), 0.99 instead of 1.34 ms for eight 64^3 pose cubes
        return "wino_fused_conv3d_"
    return "library"


def _zdft_front_ok(w0, w1, Z, SZ, channels=16) -> bool:
    """the static conditions of the direct z-DFT form of the opening conv (weight w0): cubes of ``channels`` channels and
    a (Z, SZ) the kernels are built for, 16 output channels, and a channels-last conv stack behind it (w1: a 3x3x3
    weight tells the layout the stack runs in)"""
    from . import _lib
    return bool((int(Z), int(SZ), int(channels)) in _lib.ZDFT_SHAPES and int(w0.shape[0]) == 16 and int(w0.shape[1]) <= 16
                and is_cl(w1))


def _wide_front_ok(w0, w1, Z, SZ) -> bool:
    """the static conditions of the z-spectrum form of the opening conv at 17..32 input channels (``V2VNet.wide_front``):
    the (Z, SZ) the z-DFT kernels are built for, 16 output channels and a channels-last conv stack behind it, as
    _zdft_front_ok asks - only the input side differs: the spectrum arrives from the unprojection (two channel groups), and
    the plane transforms and the contraction take any channel count.  Nothing else reads this predicate: cubes of 17..32
    channels keep the library transforms (_zdft_front_ok stays at <= 16)"""
    from . import _lib
    return bool((int(Z), int(SZ), 16) in _lib.ZDFT_SHAPES and int(w0.shape[0]) == 16 and 17 <= int(w0.shape[1]) <= 32
                and is_cl(w1))


def _one_front_ok(w0, w1, Z, SZ) -> bool:
    """the static conditions of the z-spectrum form of the opening conv at ONE input channel (``V2VNet.one_front``, the
    ROOTNET_ROOTHM root nets): as _wide_front_ok, with a 7x7x7 weight of one input channel - the spectrum arrives from the
    one-channel unprojection (SP3D_HM_ONE_ZSPECTRUM).  Nothing else reads this predicate: one-channel cubes keep the route
    they take today (_zdft_ok asks for 16-channel cubes, so they run the library's 3-D transforms)"""
    from . import _lib
    return bool((int(Z), int(SZ), 16) in _lib.ZDFT_SHAPES and int(w0.shape[0]) == 16 and int(w0.shape[1]) == 1
                and tuple(w0.shape[2:]) == (7, 7, 7) and is_cl(w1))


class _FreqConv3d(torch.autograd.Function):
    """Stride-1 'same' Conv3d (odd cubic kernel) in the frequency domain, forward AND backward, for the 7x7x7 opening
    conv of the V2V nets (v2v_net.py:113-117) on the GPU: zero-padded rFFT (rocFFT through torch.fft) -> channel
    contraction (sp3d_freq_contract_ex) -> irFFT.  With xp = x shifted by p = k//2 into an S-sized zero volume:
        y  = crop_[0,X)  irfft( sum_c  rfft(xp)[b,c] * conj(rfft(w)[o,c]) )
        dx = crop_[p,p+X) irfft( sum_o  rfft(gy)[b,o] * rfft(w)[o,c] )
        dw = crop_[0,k)  irfft( sum_b  conj(rfft(gy)[b,o]) * rfft(xp)[b,c] )
    (cross-correlation theorem; no wrap-around because S >= X + k - 1 per axis)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        from . import _lib
        B, C, X, Y, Z = x.shape
        O, k = int(w.shape[0]), int(w.shape[2])
        p = k // 2
        S = (fft_len(X + k - 1), fft_len(Y + k - 1), fft_len(Z + k - 1))
        xp = x.new_zeros((B, C) + S)
        xp[:, :, p:p + X, p:p + Y, p:p + Z] = x
        Wf = torch.fft.rfftn(w.float(), s=S, dim=(2, 3, 4))
        Yf = _lib.freq_contract_ex(torch.fft.rfftn(xp, dim=(2, 3, 4)), Wf, "fwd")
        y = torch.fft.irfftn(Yf, s=S, dim=(2, 3, 4))[:, :, :X, :Y, :Z]
        if bias is not None:
            y = y + bias.view(1, O, 1, 1, 1)
        cl = is_cl(x)
        ctx.save_for_backward(x, w)
        ctx.geom = (S, p, bias is not None, cl)
        return y.contiguous(memory_format=torch.channels_last_3d if cl else torch.contiguous_format)

    @staticmethod
    def backward(ctx, gy):
        from . import _lib
        x, w = ctx.saved_tensors
        S, p, has_bias, cl = ctx.geom
        B, C, X, Y, Z = x.shape
        O, k = int(w.shape[0]), int(w.shape[2])
        gp = gy.new_zeros((B, O) + S)
        gp[:, :, :X, :Y, :Z] = gy
        Gf = torch.fft.rfftn(gp, dim=(2, 3, 4))
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            Wf = torch.fft.rfftn(w.float(), s=S, dim=(2, 3, 4))
            gx = torch.fft.irfftn(_lib.freq_contract_ex(Gf, Wf, "dx"), s=S, dim=(2, 3, 4))[:, :, p:p + X, p:p + Y, p:p + Z]
            gx = gx.contiguous(memory_format=torch.channels_last_3d if cl else torch.contiguous_format)
        if ctx.needs_input_grad[1]:
            xp = x.new_zeros((B, C) + S)
            xp[:, :, p:p + X, p:p + Y, p:p + Z] = x
            Xf = torch.fft.rfftn(xp, dim=(2, 3, 4))
            gw = torch.fft.irfftn(_lib.freq_contract_ex(Gf, Xf, "dw"), s=S, dim=(2, 3, 4))[:, :, :k, :k, :k]
            gw = gw.contiguous().to(w.dtype)
        if has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum((0, 2, 3, 4))
        return gx, gw, gb


class PadCinConv3d(nn.Conv3d):
    """Conv3d whose input-channel count is rounded up to a multiple of 4 AT RUN TIME (zero input
    channels x zero weight slices: same math, parameters and state_dict unchanged).  MIOpen's
    7^3 kernels for Cin = 15 run 3.2x slower than for Cin = 16 on gfx950 (4.84 ms vs 1.51 ms at
    (4,15,80,80,20), tools/bench_cin.py); callers may also hand in an already padded tensor."""

    # 7^3 kernels on the GPU run through _FreqConv3d.  The weight spectrum (O*C volumes) has to be recomputed on every
    # call while the weights train - and once more, plus the O*C inverse transforms of the weight gradient, in the
    # backward - so under autograd it only pays for batches of at least `freq_domain_min_batch` cubes
    # (full-size training step, batch 2 per GPU: 102 ms direct vs 140 ms in the frequency domain, measured).
    freq_domain = True
    freq_domain_min_batch = 8

    def forward(self, x):
        cin = self.in_channels
        have = x.shape[1]
        if self.freq_domain and x.is_cuda and x.dtype == torch.float32 and self.kernel_size == (7, 7, 7) and \
                self.stride == (1, 1, 1) and self.padding == (3, 3, 3) and self.dilation == (1, 1, 1) and \
                self.groups == 1 and have >= cin and \
                (not torch.is_grad_enabled() or x.shape[0] >= self.freq_domain_min_batch):
            return _FreqConv3d.apply(x[:, :cin] if have > cin else x, self.weight, self.bias)
        xp, w = pad_cin(x, self.weight)
        if w is self.weight:
            return super().forward(x)
        return F.conv3d(xp, w, self.bias, self.stride, self.padding, self.dilation, self.groups)


class ConvBnRelu3d(nn.Module):
    """`.block` = Conv3d -> BN -> ReLU (v2v_net.py:10-20)"""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.block = nn.Sequential(PadCinConv3d(cin, cout, k, stride=1, padding=(k - 1) // 2), _bn(cout), nn.ReLU(True))

    def forward(self, x):
        if _grouped(self.block[1], self.training):          # BatchNorm + ReLU in one pass (the ReLU mask is recomputed
            return self.block[1].grouped_forward(self.block[0](x), relu=True)    # from the input in the backward)
        return self.block(x)


class Residual3d(nn.Module):
    """`.res_branch` (conv-bn-relu-conv-bn) + `.skip_con` (identity or 1^3 conv-bn) (v2v_net.py:23-45)"""

    def __init__(self, cin, cout):
        super().__init__()
        self.res_branch = nn.Sequential(
            nn.Conv3d(cin, cout, 3, 1, 1), _bn(cout), nn.ReLU(True), nn.Conv3d(cout, cout, 3, 1, 1), _bn(cout))
        self.skip_con = nn.Sequential() if cin == cout else nn.Sequential(nn.Conv3d(cin, cout, 1, 1, 0), _bn(cout))

    def forward(self, x):
        rb = self.res_branch
        if _grouped(rb[1], self.training):          # BatchNorm + ReLU, and the block's tail BatchNorm + add + ReLU, one pass each
            h = rb[3](rb[1].grouped_forward(rb[0](x), relu=True))
            return rb[4].grouped_forward(h, relu=True, residual=self.skip_con(x))
        return F.relu(self.res_branch(x) + self.skip_con(x), True)


class Up2x3d(nn.Module):
    """`.block` = ConvTranspose3d(k2,s2) -> BN -> ReLU (v2v_net.py:57-69)"""

    def __init__(self, cin, cout):
        super().__init__()
        self.block = nn.Sequential(nn.ConvTranspose3d(cin, cout, 2, stride=2, padding=0, output_padding=0), _bn(cout),
                                   nn.ReLU(True))

    def forward(self, x):
        if _grouped(self.block[1], self.training):
            return self.block[1].grouped_forward(self.block[0](x), relu=True)
        return self.block(x)


class _EncDec(nn.Module):
    """two-level U-shaped core (v2v_net.py:72-110); attribute names = checkpoint keys"""

    def __init__(self):
        super().__init__()
        self.encoder_res1 = Residual3d(32, 64)
        self.encoder_res2 = Residual3d(64, 128)
        self.mid_res = Residual3d(128, 128)
        self.decoder_res2 = Residual3d(128, 128)
        self.decoder_upsample2 = Up2x3d(128, 64)
        self.decoder_res1 = Residual3d(64, 64)
        self.decoder_upsample1 = Up2x3d(64, 32)
        self.skip_res1 = Residual3d(32, 32)
        self.skip_res2 = Residual3d(64, 64)

    def forward(self, x):
        s1 = self.skip_res1(x)
        x = self.encoder_res1(F.max_pool3d(x, 2, 2))
        s2 = self.skip_res2(x)
        x = self.encoder_res2(F.max_pool3d(x, 2, 2))
        x = self.decoder_res2(self.mid_res(x))
        x = self.decoder_upsample2(x) + s2
        x = self.decoder_upsample1(self.decoder_res1(x)) + s1
        return x


class TiledZSpectrum:
    """What the fused root-grid unprojection hands to the opening conv INSTEAD of cubes (ProjectLayer.get_voxel_zspectrum):
    the z-spectrum of the (B, cin, X, Y, Z) cubes, (B, cin, SZ//2+1, X/4, Y/4, 16) complex64 in 4 x 4 tiles.  Quacks like the
    cubes where the plan looks (shape / device / dtype)."""

    def __init__(self, spec: torch.Tensor, X: int, Y: int, Z: int, SZ: int):
        self.spec, self.X, self.Y, self.Z, self.SZ = spec, int(X), int(Y), int(Z), int(SZ)
        self.shape = (int(spec.shape[0]), int(spec.shape[1]), self.X, self.Y, self.Z)
        self.device, self.is_cuda, self.dtype = spec.device, spec.is_cuda, torch.float32


class _Conv(NamedTuple):
    """one BatchNorm-folded conv of the plan (the opening conv or a 3x3x3 layer) with every form of its weights it can run with"""
    w: torch.Tensor                            # folded weight (O, C, k, k, k)
    shift: torch.Tensor                        # what is left of bias and BatchNorm, per output channel
    u: Optional[torch.Tensor] = None           # Winograd-domain weights (_lib.wino_weights)
    split: Optional[torch.Tensor] = None       # ... in three bf16 pieces (_lib.wino_weights_split): the fused kernels
    direct: Optional[torch.Tensor] = None      # w in three bf16 pieces, 48-byte records: conv3_split_ (_lib.conv_weights_split)
    direct24: Optional[torch.Tensor] = None    # ... in 24-byte blocks: conv3_split128_ (_lib.conv_weights_split24)
    split_yz: Optional[torch.Tensor] = None    # G along y,z only, raw along x, the records of ``split``: the half-resolution
                                               # fused kernel's direct-in-x form (_lib.wino_yz_weights_split)


class _Res(NamedTuple):
    """a residual block: conv-ReLU-conv, + the input (or its folded 1x1x1 projection ``skip``), ReLU"""
    c1: _Conv
    c2: _Conv
    skip: Optional[torch.Tensor]
    # the projection in the record forms of the kernels that compute it on the second conv's accumulators (no GEMM, no
    # projected tensor): 16 -> 32 for conv3_split_ (_lib.conv_weights_split), 32 -> 64 for wino_fused_conv3d_ with split
    # weights (_lib.wino_weights_split, chunk 16)
    skip_direct: Optional[torch.Tensor] = None
    skip_split: Optional[torch.Tensor] = None
    # _tail max-pools this block's output (front_res, encoder_res1): where the skip is folded and _lib.pool_fold_covers, the
    # second conv writes the pooled tensor too and _pool hands it on without a launch
    pooled: bool = False


class _Up(NamedTuple):
    """a folded ConvTranspose3d(2, stride 2): weight (Cin, Cout, 2, 2, 2), shift, the weight in GEMM form (Cin, 8*Cout)
    and, for the shapes the one-kernel form covers, the GEMM form in three bf16 pieces (_lib.upconv_weights_split)"""
    wT: torch.Tensor
    shift: torch.Tensor
    wg: torch.Tensor
    split: Optional[torch.Tensor] = None


class _FoldedV2V:
    """Inference execution plan of a V2VNet: every BatchNorm3d (running statistics) is folded into the
    preceding (transposed) conv's weights, so a layer is one MIOpen conv (no bias) + ONE fused
    in-place epilogue (sp3d_channel_shift_act: shift [+ residual] [+ ReLU]) instead of conv + bias +
    BatchNorm + ReLU (+ add) kernels.  Same math as v2v_net.py:10-110 up to fp32 rounding of the
    folded weights.  Rebuilt whenever any parameter / buffer was replaced, moved or written through autograd-visible ops
    ((data_ptr, _version) of EVERY tensor), when the memory format of the 3x3x3 weights changes, after ``train()`` and
    after ``load_state_dict``.  Writes through ``.data`` leave no trace in tensor metadata: call
    ``V2VNet.invalidate_plan()`` after such weight surgery."""

    def __init__(self, net: "V2VNet"):
        self.net = net
        self.key = None
        self.layers = {}           # layer name -> _Conv ("front") | _Res | _Up
        self.spectra = {}          # ("Wf" | "Wz" | "Wty", FFT shape) -> the opening conv's weight spectrum in that form
        self.xpad = {}             # (cin, FFT shape, device) -> zero-padded input buffer of the frequency-domain front
        self.pooled = None         # (y, y_pooled) of the latest _res that also pooled its output, until the next _pool

    def graph_tensors(self):
        """everything a captured graph of this plan's forward may hold an address of (the layers' weights in all their
        forms, the weight spectra, the padded FFT buffers), as they are now: whoever replays the graph keeps this"""
        return dict(self.layers), dict(self.spectra), dict(self.xpad)

    @staticmethod
    def _key(net):
        ps = list(net.parameters()) + list(net.buffers())
        w3 = net.front_layers[1].res_branch[0].weight          # a 3x3x3 weight: its strides tell the memory format
        return (tuple((p.data_ptr(), p._version) for p in ps), str(w3.device), bool(is_cl(w3)))

    def _ensure_built(self):
        key = self._key(self.net)
        if key != self.key:
            self._build()
            self.key = key

    @staticmethod
    def _fold(conv, bn, transposed=False):
        s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shape = (1, -1, 1, 1, 1) if transposed else (-1, 1, 1, 1, 1)
        w = conv.weight * s.view(shape)
        fmt = torch.channels_last_3d if is_cl(conv.weight) else torch.contiguous_format
        b = conv.bias if conv.bias is not None else torch.zeros_like(bn.running_mean)
        return w.contiguous(memory_format=fmt), ((b - bn.running_mean) * s + bn.bias).contiguous()

    @staticmethod
    def _conv3_routes(cin, cout):
        """the routes of a cin -> cout layer: either side of the Infinity-Cache bound, a grid of whole 5x5x5 blocks, all switches"""
        return {conv3_route(cin, cout, s, True, ws, dc) for s in ((1, 2, 2, 2), (1 << 20, 2, 2, 2), (1, 5, 5, 5))
                for ws in (True, False) for dc in (True, False)}

    @staticmethod
    def _conv3_record(w, shift):
        """a folded 3x3x3 conv with the weight forms of every route conv3_route can give it (weights on the GPU)"""
        from . import _lib
        cout, cin = int(w.shape[0]), int(w.shape[1])
        routes = _FoldedV2V._conv3_routes(cin, cout)
        if not w.is_cuda or routes == {"library"}:
            return _Conv(w, shift)
        u = _lib.wino_weights(w)
        # layers of the fused kernels: weights split for the bf16 matrix pipe (lane quarters for 64 output channels)
        split = _lib.wino_weights_split(u, 16 if cout == 64 else 8) if "wino_fused_conv3d_" in routes else None
        # full-resolution (16 | 32 -> 32) and quarter-resolution layers (64 | 128 -> 128): direct convolution, three exact pieces
        direct = _lib.conv_weights_split(w) if "conv3_split_" in routes else None
        direct24 = _lib.conv_weights_split24(w) if "conv3_split128_" in routes else None
        # half-resolution layers (32 | 64 -> 64): the 48-point records of the fused kernel's y,z form
        split_yz = _lib.wino_yz_weights_split(w) if split is not None and cout == 64 else None
        return _Conv(w, shift, u, split, direct, direct24, split_yz)

    def _build(self):
        from . import _lib
        n, layers = self.net, {}
        layers["front"] = _Conv(*self._fold(n.front_layers[0].block[0], n.front_layers[0].block[1]))
        ed = n.encoder_decoder
        for name in ("front_res", "encoder_res1", "encoder_res2", "mid_res", "decoder_res2", "decoder_res1", "skip_res1",
                     "skip_res2"):
            blk = n.front_layers[1] if name == "front_res" else getattr(ed, name)
            w1, s1 = self._fold(blk.res_branch[0], blk.res_branch[1])
            w2, s2 = self._fold(blk.res_branch[3], blk.res_branch[4])
            ws = sd = sp = None
            if len(blk.skip_con) > 0:              # the skip's shift rides on the second conv's epilogue
                ws, ss = self._fold(blk.skip_con[0], blk.skip_con[1])
                s2 = (s2 + ss).contiguous()
                co, ci = int(ws.shape[0]), int(ws.shape[1])
                if ws.is_cuda and (co, ci) == (32, 16):
                    sd = _lib.conv_weights_split(ws)
                if ws.is_cuda and (co, ci) == (64, 32):
                    sp = _lib.wino_weights_split(ws.reshape(co, ci).t().reshape(1, ci, co).contiguous(), 16)
            layers[name] = _Res(self._conv3_record(w1, s1), self._conv3_record(w2, s2), ws, sd, sp,
                                pooled=name in ("front_res", "encoder_res1"))
        for name in ("decoder_upsample2", "decoder_upsample1"):
            blk = getattr(ed, name).block
            wT, sT = self._fold(blk[0], blk[1], transposed=True)
            # (Cin, Cout, 2,2,2) -> GEMM form (Cin, 8*Cout), columns ordered (i,j,k,o): see _up2x
            wg = wT.permute(0, 2, 3, 4, 1).reshape(wT.shape[0], 8 * wT.shape[1]).contiguous()
            # 128 -> 64 and 64 -> 32 (+ output conv): product and scatter in one kernel (sp3d_upconv2x_fused)
            fused = wg.is_cuda and (int(wT.shape[0]), int(wT.shape[1])) in ((128, 64), (64, 32))
            layers[name] = _Up(wT, sT, wg, _lib.upconv_weights_split(wg) if fused else None)
        # the spectra belong to the old weights; the padded buffers go with them, a caller's view of one is then copied
        self.layers, self.spectra, self.xpad = layers, {}, {}

    def _route(self, x, c: "_Conv") -> str:
        from . import _lib
        n = self.net
        if c.u is None or not is_cl(x):
            return "library"
        return conv3_route(int(c.w.shape[1]), int(c.w.shape[0]), (x.shape[0],) + tuple(x.shape[2:]), n.winograd,
                           getattr(n, "wino_split", True), getattr(n, "direct_conv", True),
                           quarter_direct=c.direct24 is not None and _lib.quarter_direct_enabled())

    def _conv3(self, x, c: "_Conv", mode, residual=None, xs=None, skip_w=None, pool=False):
        """3x3x3 conv + fused epilogue on the route conv3_route names (weights on the GPU and channels-last x); xs, skip_w:
        the block input and its projection records for the two kernels that fold the skip (_folded_skip chose them); pool:
        those kernels' pooled form, (y, y_pooled) instead of y (_pool_fold said the grid has one)"""
        from . import _lib
        route = self._route(x, c)
        split = getattr(self.net, "wino_split", True)
        # (the keyword only where it is asked for: callers that wrap the entries see the calls they saw before)
        kw = dict(pool=True) if pool else {}
        if route == "conv3_split_":
            return _lib.conv3_split_(x, c.direct, c.shift, mode, residual, xs=xs, skip_w=skip_w, **kw)
        if route == "wino_fused_conv3d_":
            return _lib.wino_fused_conv3d_(x, c.u, c.shift, mode, residual, c.split if split else None, xs=xs, skip_w=skip_w,
                                           U3yz=c.split_yz if split else None, **kw)
        assert xs is None and skip_w is None and not pool, route
        if route == "conv3_split128_":
            return _lib.conv3_split128_(x, c.direct24, c.shift, mode, residual)
        if route == "wino_conv3d_":
            return _lib.wino_conv3d_(x, c.u, c.shift, mode, residual)
        return _lib.channel_shift_act_(F.conv3d(x, c.w, None, 1, 1), c.shift, mode, residual)

    def _folded_skip(self, x, h, r: "_Res"):
        """the projection records of block r for the kernel its second conv takes on h, or None: that kernel has no folded
        form (other widths, the library, the three-launch Winograd, fp32 Winograd products), x is not a dense float32
        channels-last tensor of the projection's input width, or SP3D_FOLD_SKIP=0"""
        from . import _lib
        if r.skip is None or not _lib.skip_fold_enabled() or not (is_cl(x) and x.is_cuda and x.dtype == torch.float32):
            return None
        route, widths = self._route(h, r.c2), (int(r.c2.w.shape[1]), int(r.c2.w.shape[0]), int(x.shape[1]))
        if route == "conv3_split_" and widths == (32, 32, 16):
            return r.skip_direct
        if route == "wino_fused_conv3d_" and getattr(self.net, "wino_split", True) and widths == (64, 64, 32):
            return r.skip_split
        return None

    def _pool_fold(self, h, c: "_Conv") -> bool:
        """the kernel conv c takes on h has a pooled form on this grid (_lib.pool_fold_covers), and SP3D_FOLD_POOL is not 0"""
        from . import _lib
        return bool(_lib.pool_fold_enabled() and _lib.pool_fold_covers(self._route(h, c), *h.shape[2:]))

    def _res(self, x, name):
        r = self.layers[name]
        h = self._conv3(x, r.c1, 1)
        if r.skip is None:
            return self._conv3(h, r.c2, 2, x)
        rec = self._folded_skip(x, h, r)
        if rec is not None:                         # relu(conv3(h) + W . x + shift): neither the GEMM nor its product exists
            if r.pooled and self._pool_fold(h, r.c2):
                # ... and its MaxPool3d(2,2) from the same accumulators, kept for the _pool that is handed this very tensor
                y, yp = self._conv3(h, r.c2, 1, xs=x, skip_w=rec, pool=True)
                self.pooled = (y, yp)
                return y
            return self._conv3(h, r.c2, 1, xs=x, skip_w=rec)
        return self._conv3(h, r.c2, 2, self._conv1(x, r.skip))

    # -- library GEMM selection (OPT-IN) ---------------------------------------------------------------------------
    # The plan's GEMMs (batched Winograd products, transposed-conv and 1x1x1 GEMMs) are plain library calls; which
    # rocBLAS / hipBLASLt solution the library's heuristic picks matters: the 64 x (8000 x 64 x 64) batched product of a
    # half-resolution layer runs 85 us with the default solution and 47 us with the best one (tools/exp_blas.sh).
    # PyTorch's TunableOp can do that selection, but it is PROCESS-WIDE state and its choice comes from timing, so a
    # library forward must not switch it on behind the caller's back (round-2 advisor finding).  It is therefore off
    # unless the caller asks: ``V2VNet.tune_gemms(True)`` (what bench.py does, and says so in its JSON line) or
    # SP3D_TUNE_GEMM=1.  When on: the FIRST eager forward of each input shape runs with tuning enabled (a few ms per
    # GEMM shape, never during graph capture); later forwards only look the selection up.  TunableOp's enabled /
    # tuning flags are restored to the caller's values when the forward returns, its results file is neither renamed
    # nor written by this code: set PYTORCH_TUNABLEOP_FILENAME yourself to persist selections, and load the same
    # file on every rank (PYTORCH_TUNABLEOP_TUNING=0) for run-to-run / rank-to-rank identical kernels.
    _tuned_shapes: "set[tuple]" = set()
    _tune_gemms = None                 # None: follow SP3D_TUNE_GEMM (default off); True / False: explicit

    @staticmethod
    def _tunable():
        from . import _lib
        on = _FoldedV2V._tune_gemms
        if on is None:
            on = _lib.env_switch("SP3D_TUNE_GEMM", False)
        return getattr(torch.cuda, "tunable", None) if on else None

    def _run_tuned(self, x):
        tun = self._tunable()
        if tun is None or not x.is_cuda:
            return self._run(x)
        capturing = torch.cuda.is_current_stream_capturing()
        shape_key = (tuple(x.shape), str(x.device), bool(self.net.winograd), bool(self.net.fft_front))
        was_on, was_tuning = tun.is_enabled(), tun.tuning_is_enabled()
        try:
            tun.enable(True)
            first = shape_key not in _FoldedV2V._tuned_shapes and not capturing
            tun.tuning_enable(bool(first))
            if first:
                tun.set_max_tuning_duration(30)
            out = self._run(x)
            if first:
                _FoldedV2V._tuned_shapes.add(shape_key)
            return out
        finally:                       # the caller's process-wide settings come back; the selections stay in TunableOp's
            tun.tuning_enable(was_tuning)      # in-memory table and are found again by the next forward of this plan
            tun.enable(was_on)

    @torch.no_grad()
    def run(self, x):
        return self._run_tuned(x)

    def _run(self, x):
        from . import _lib
        self._ensure_built()
        w0, s0 = self.layers["front"][:2]
        if isinstance(x, TiledZSpectrum):
            return self._tail(self._front_zspectrum(x, w0, s0))
        if self.net.fft_front and w0.shape[2] == 7 and x.shape[1] >= w0.shape[1]:
            return self._tail(self._front_fft(x, w0, s0))
        x, w0 = pad_cin(x, w0)
        return self._tail(_lib.channel_shift_act_(F.conv3d(x, w0, None, 1, 3), s0, 1))

    def _zdft_ok(self, x, w0, S):
        """the direct z-DFT form of the opening conv applies: _zdft_front_ok, and x is channels-last 16-channel fp32 cubes"""
        if not (getattr(self.net, "zdft", True) and x.dim() == 5 and x.is_cuda and x.dtype == torch.float32):
            return False
        return bool(_zdft_front_ok(w0, self.layers["front_res"].c1.w, x.shape[4], S[2], x.shape[1])
                    and x.permute(0, 2, 3, 4, 1).is_contiguous())

    @staticmethod
    def _fft_shape(X, Y, Z, k):
        """padded transform lengths: >= n + k//2 zeros behind the signal, rocFFT-friendly factors, and a z length that
        is a multiple of 4 so that every row of the buffer starts 16-byte aligned"""
        sz = fft_len(Z + k - 1)
        while sz % 4:
            sz = fft_len(sz + 2)
        return (fft_len(X + k - 1), fft_len(Y + k - 1), sz)

    def _fft_buffer(self, B, cin, S, device):
        """zero-padded input buffer for B volumes: ONE buffer per (cin, S, device), grown when a larger batch shows
        up and sliced otherwise (the padding is never written, so any prefix of it is a valid padded buffer)"""
        bkey = (cin, S, str(device))
        buf = self.xpad.get(bkey)
        if buf is None or buf.shape[0] < B:
            buf = self.xpad[bkey] = torch.zeros((B, cin) + S, dtype=torch.float32, device=device)
        return buf[:B]

    def fft_input_view(self, B, X, Y, Z, device):
        """(B,cin,X,Y,Z) view of the zero-padded input buffer of the frequency-domain opening conv: a producer
        (ProjectLayer.get_voxel(out=...)) that fills it saves the pad/copy pass; `run` recognises the view."""
        self._ensure_built()
        w0 = self.layers["front"].w
        cin, k = int(w0.shape[1]), int(w0.shape[2])
        if not (self.net.fft_front and k == 7):
            return None
        return self._fft_buffer(B, cin, self._fft_shape(X, Y, Z, k), device)[:, :, :X, :Y, :Z]

    def _is_padded_view(self, x, cin, S):
        """is x the [:X,:Y,:Z] corner of whole samples of the zero-padded buffer this plan owns for (cin, S)?"""
        buf = self.xpad.get((cin, S, str(x.device)))
        vol = S[0] * S[1] * S[2]
        if buf is None or x.dim() != 5 or x.shape[1] != cin or x.dtype != buf.dtype or \
                tuple(x.stride()) != (cin * vol, vol, S[1] * S[2], S[2], 1):
            return False
        off = x.data_ptr() - buf.data_ptr()
        per = cin * vol * buf.element_size()
        return off >= 0 and off % per == 0 and off // per + x.shape[0] <= buf.shape[0]

    def _weights_f(self, w0, S):
        """the opening conv's weight spectrum conj(rfftn(taps)) / N, (O, C, SX, SY, SZ/2+1)"""
        if ("Wf", S) not in self.spectra:
            # the signal sits at the ORIGIN of the padded buffer (so a producer can write 16-byte aligned rows into it,
            # fft_input_view), hence the kernel is centred on the origin: taps -p..p wrap around to S-p..S-1
            k = int(w0.shape[2])
            wp = torch.zeros(tuple(w0.shape[:2]) + S, dtype=torch.float32, device=w0.device)
            wp[:, :, :k, :k, :k] = w0.float()
            wp = torch.roll(wp, shifts=(-(k // 2),) * 3, dims=(2, 3, 4))
            # correlation (conj); the inverse transform's 1/N is folded in here, so irfftn runs unnormalised
            self.spectra["Wf", S] = (torch.conj(torch.fft.rfftn(wp, dim=(2, 3, 4))).resolve_conj() /
                                     float(S[0] * S[1] * S[2])).contiguous()
        return self.spectra["Wf", S]

    def _weights_z(self, w0, S):
        """the opening conv's weight spectrum with kz as the slowest frequency index (what the direct z-DFT form contracts with)"""
        if ("Wz", S) not in self.spectra:
            self.spectra["Wz", S] = self._weights_f(w0, S).permute(0, 1, 4, 2, 3).contiguous()
            if not self.xpad:
                del self.spectra["Wf", S]              # nobody asked for the planar buffer: keep one spectrum only
        return self.spectra["Wz", S]

    def _weights_ty(self, w0, S):
        """(T, tw) of _lib.freq_contract_ty: the opening conv's taps transformed along z and x only (float64 on the host
        side of the plan build, stored fp32), as (G_p, S_1, D_1, ..., S_p, D_p) per (row = (kz, kx), o, c), and the
        (cos, sin)(2 pi ky u / SY) table.  W^[o,c,kz,kx,ky] = conj(rfftn(taps centred on the origin)) / N is what the kernel
        rebuilds from them per bin (csrc/sp3d_fftconv.hip)."""
        key = ("Wty", S)
        if key not in self.spectra:
            import math
            k = int(w0.shape[2])
            p = k // 2
            SX, SY, SZ = S
            w = w0.detach().double().cpu()                                       # (O, C, tx, ty, tz)
            t = torch.arange(k, dtype=torch.float64) - p
            ex = torch.exp(2j * math.pi * torch.arange(SX, dtype=torch.float64)[:, None] * t[None, :] / SX)            # (kx, tx)
            ez = torch.exp(2j * math.pi * torch.arange(SZ // 2 + 1, dtype=torch.float64)[:, None] * t[None, :] / SZ)   # (kz, tz)
            G = torch.einsum("ocxyz,kx,mz->mkocy", w.to(torch.complex128), ex, ez) / float(SX * SY * SZ)            # (kz,kx,O,C,ty)
            cols = [G[..., p]]
            for u in range(1, p + 1):
                cols += [G[..., p + u] + G[..., p - u], G[..., p + u] - G[..., p - u]]
            T = torch.view_as_real(torch.stack(cols, -1))                        # (kz,kx,O,C,1+2p,2)
            T = T.reshape(G.shape[0] * G.shape[1], G.shape[2], G.shape[3], 2 * (1 + 2 * p)).float().contiguous()
            ang = 2.0 * math.pi * torch.arange(SY, dtype=torch.float64)[:, None] * torch.arange(1, p + 1, dtype=torch.float64)[None, :] / SY
            tw = torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous()
            self.spectra[key] = (T.to(w0.device), tw.to(w0.device))
        return self.spectra[key]

    def _contract(self, Xs, w0, S):
        """channel contraction of the opening conv on the kz-slowest spectrum: with the weight spectrum's y transform rebuilt
        per bin (17.7 MB of table instead of 223 MB of spectrum on the root grid) when the kernel covers the shape"""
        from . import _lib
        # measured (profiles/r06_contract_ty.md): 12.6x fewer weight bytes, but no faster in the step (1.4512 vs 1.4507 ms) - the
        # rebuilt spectrum costs the VALU what the stream cost the HBM.  Opt-in: V2VNet.contract_ty = True / SP3D_CONTRACT_TY=1.
        on = getattr(self.net, "contract_ty", _lib.env_switch("SP3D_CONTRACT_TY", False))
        if on and int(w0.shape[2]) == 7 and int(w0.shape[1]) <= 16 and 4 * S[1] <= 384:
            T, tw = self._weights_ty(w0, S)
            return _lib.freq_contract_ty(Xs, T, tw)
        return _lib.freq_contract(Xs, self._weights_z(w0, S))

    def _front_zspectrum(self, z: "TiledZSpectrum", w0, s0):
        """opening conv when the unprojection already delivered the z-spectrum (round 6): x,y plane transforms (un-tiling
        on load) -> contraction -> inverse x,y -> inverse z-DFT + shift + ReLU.  Same kernels and bits as the cubes path of
        _front_fft minus zdft_fwd_cl_kernel (and minus the cubes' trip through HBM)."""
        from . import _lib
        k = int(w0.shape[2])
        S = self._fft_shape(z.X, z.Y, z.Z, k)
        if S[2] != z.SZ or S[0] != 88 or S[1] != 88 or int(w0.shape[1]) != z.shape[1] or int(w0.shape[0]) != 16:
            raise _lib.Sp3dError(f"TiledZSpectrum of {z.shape} (SZ {z.SZ}) does not fit this net's opening conv (FFT shape {S})")
        Xs = _lib.cfft2d_88_tiled(z.spec, z.X, z.Y)
        Ys = _lib.cfft2d_(self._contract(Xs, w0, S), True, rows_out=z.X)
        return _lib.zdft_inv_cl(Ys, z.X, z.Y, z.Z, S[2], s0, True)

    def _front_fft(self, x, w0, s0):
        """the 7x7x7 opening conv in the frequency domain: zero-padded rFFT (rocFFT via torch.fft) ->
        sp3d_freq_contract -> irFFT -> crop + shift + ReLU.  3.3x (80x80x20, B=4) to 4.7x (64^3) faster than the
        direct fp32 convolution and ~10x closer to the float64 result (tools/exp_fftconv.py)."""
        from . import _lib
        B, _, X, Y, Z = x.shape
        cin, k = int(w0.shape[1]), int(w0.shape[2])
        S = self._fft_shape(X, Y, Z, k)
        if self._zdft_ok(x, w0, S):
            # root grid: direct z-DFTs around dense 2-D complex transforms; the spectrum's slowest frequency index is kz,
            # the weight spectrum is stored in the same order (_weights_z).  x is the unprojection's channels-last result.
            Xs = _lib.cfft2d_(_lib.zdft_fwd_cl(x, cin, S), False, rows_in=X)          # rows x >= X are zero padding
            Ys = _lib.cfft2d_(self._contract(Xs, w0, S), True, rows_out=X)              # ... and not read on the way back
            return _lib.zdft_inv_cl(Ys, X, Y, Z, S[2], s0, True)
        if self._is_padded_view(x, cin, S):
            # x IS the signal corner of this plan's zero-padded buffer (fft_input_view / input_chunk_views): no pad/copy
            # pass.  Recognised by address and strides, not by a Python attribute: a tensor that went through an
            # autograd Function under no_grad comes back as a NEW Python object for the same memory (advisor, round 2)
            buf = x.as_strided((B, cin) + S, x.stride(), x.storage_offset())
        else:
            buf = self._fft_buffer(B, cin, S, x.device)
            buf[:, :, :X, :Y, :Z].copy_(x[:, :cin])                             # borders stay zero across calls
        # cached hipFFT plans behind the C ABI: same rocFFT kernels (bit-identical spectra) as torch.fft.rfftn / irfftn,
        # minus the defensive clones torch makes around every real transform on ROCm (3 x ~55 MB per root-net step)
        Yf = _lib.freq_contract(_lib.rfft3d(buf), self._weights_f(w0, S))
        y = _lib.irfft3d_(Yf, S[2])                                  # unnormalised (1/N is in Wf); Yf is scratch
        cl = is_cl(self.layers["front_res"].c1.w)       # a 3x3x3 weight tells the layout the conv stack runs in
        if cl and y.is_contiguous() and y.shape[1] % 4 == 0 and Z % 4 == 0 and 4 * Z * (y.shape[1] + 4) * 4 <= 65536:
            return _lib.crop_shift_act_cl(y, X, Y, Z, s0, True)     # crop + layout change + epilogue in one pass
        y = y[:, :, :X, :Y, :Z]
        y = y.contiguous(memory_format=torch.channels_last_3d if cl else torch.contiguous_format)
        return _lib.channel_shift_act_(y, s0, 1)

    def _tail(self, x):
        from . import _lib
        x = self._res(x, "front_res")
        skip1 = self._res(x, "skip_res1")
        x = self._res(self._pool(x), "encoder_res1")
        skip2 = self._res(x, "skip_res2")
        x = self._res(self._pool(x), "encoder_res2")
        x = self._res(self._res(x, "mid_res"), "decoder_res2")
        x = self._up2x(x, "decoder_upsample2", skip2)
        x = self._res(x, "decoder_res1")
        o = self.net.output_layer
        wT, sT, wg, w3 = self.layers["decoder_upsample1"]
        if self.net.winograd and is_cl(x) and wg.is_cuda and wT.shape[1] == 32 and x.dtype == torch.float32:
            # the last up-sampling layer's only consumer is the 1x1x1 output conv: one kernel, no 32-channel tensor
            return _lib.upsample2x_head_(x, wg, sT, skip1, o.weight, o.bias, w3)
        x = self._up2x(x, "decoder_upsample1", skip1)
        return self._conv1(x, o.weight, o.bias)

    def _pool(self, x):
        """MaxPool3d(2,2): own channels-last kernel (torch's also computes the arg-max indices: 2.4x the time)"""
        from . import _lib
        # what the _res before wrote next to its output - only for that very tensor; whatever is stashed is dropped here
        stash, self.pooled = self.pooled, None
        have = stash[1] if stash is not None and stash[0] is x else None
        if is_cl(x) and x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0 and \
                all(int(v) % 2 == 0 for v in x.shape[2:]):
            return _lib.maxpool2x(x, have=have) if have is not None else _lib.maxpool2x(x)
        return F.max_pool3d(x, 2, 2)

    def _up2x(self, x, name, skip):
        """ConvTranspose3d(2, stride 2) + BN + ReLU + skip: no overlapping taps, so on channels-last activations it is
        one product + a scatter with the epilogue instead of MIOpen's backward-data kernel - in one kernel
        (sp3d_upconv2x_fused) where the plan holds split weights, else a library GEMM + sp3d_upsample2x_scatter"""
        from . import _lib
        wT, sT, wg, w3 = self.layers[name]
        if self.net.winograd and is_cl(x) and wg.is_cuda and wT.shape[1] % 4 == 0:
            return _lib.upsample2x_(x, wg, sT, skip, w3)
        return _lib.channel_shift_act_(F.conv_transpose3d(x, wT, None, 2), sT, 3, skip)

    def _conv1(self, x, w, bias=None):
        """1x1x1 conv: on channels-last activations a plain (voxels, Cin) x (Cin, Cout) GEMM on the same memory"""
        if self.net.winograd and is_cl(x) and x.is_cuda:
            B, C, X, Y, Z = x.shape
            O = w.shape[0]
            x2 = x.permute(0, 2, 3, 4, 1).reshape(-1, C)
            y = torch.matmul(x2, w.reshape(O, C).t()) if bias is None else torch.addmm(bias, x2, w.reshape(O, C).t())
            return y.view(B, X, Y, Z, O).permute(0, 4, 1, 2, 3)
        return F.conv3d(x, w, bias, 1, 0)


class V2VNet(nn.Module):
    def __init__(self, input_channels: int, output_channels: int):
        super().__init__()
        self.front_layers = nn.Sequential(ConvBnRelu3d(input_channels, 16, 7), Residual3d(16, 32))
        self.encoder_decoder = _EncDec()
        self.output_layer = nn.Conv3d(32, output_channels, 1, 1, 0)
        self.fused_inference = True      # eval + no_grad + GPU: BatchNorm-folded plan with fused epilogues
        self.fft_front = True            # ... whose 7x7x7 opening conv runs in the frequency domain (rocFFT)
        self.winograd = True             # ... and whose wide low-resolution 3x3x3 convs run as Winograd F(2,3)
        self.zdft = True                 # ... root grid: direct z-DFTs + dense 2-D transforms instead of the 3-D real plans
        self.wino_split = True           # ... fused Winograd layers: exact 3-piece bf16 splits on the bf16 matrix pipe
        self.direct_conv = True          # ... full-resolution 3x3x3 layers: direct (implicit GEMM) split convolution
        # opt-in (SP3D_WIDE_FRONT=1): at 17..32 input channels the opening conv may start from the unprojection's z-spectrum too
        from . import _lib
        self.wide_front = _lib.env_switch("SP3D_WIDE_FRONT", False)
        # opt-in (SP3D_ONE_FRONT=1): at ONE input channel (ROOTNET_ROOTHM) the opening conv may start from the z-spectrum of the
        # one-channel unprojection instead of cubes through the library's 3-D transforms
        self.one_front = _lib.env_switch("SP3D_ONE_FRONT", False)
        self._plan = None
        self.reset_parameters()

    def reset_parameters(self):
        # N(0, 1e-3) weights, zero bias for every (transposed) conv (v2v_net.py:135-144)
        for m in self.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                nn.init.normal_(m.weight, 0.0, 0.001)
                nn.init.zeros_(m.bias)

    def invalidate_plan(self):
        """drop the folded inference plan (BatchNorm-folded / Winograd / frequency-domain weights); it is rebuilt from
        the current parameters on the next eval forward"""
        self._plan = None
        return self

    def train(self, mode: bool = True):
        # the folded plan is dropped when the module ENTERS training (weights are about to change); model.eval() on a
        # module that already is in eval mode - every validation pass calls it - keeps the plan (and its padded
        # buffers).  Weight edits while in eval mode are still caught by the plan's (data_ptr, version) key.
        if mode and not self.training:
            self._plan = None
        return super().train(mode)

    @staticmethod
    def tune_gemms(on: bool = True):
        """opt in (or out) of library-GEMM selection through PyTorch's TunableOp for the inference plan's GEMMs
        (process-wide TunableOp state is touched only inside the plan's forward and restored afterwards; see
        _FoldedV2V._run_tuned).  Default: off, or SP3D_TUNE_GEMM=1."""
        _FoldedV2V._tune_gemms = None if on is None else bool(on)

    def _load_from_state_dict(self, *args, **kwargs):
        self._plan = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _get_plan(self) -> _FoldedV2V:
        if self._plan is None:
            self._plan = _FoldedV2V(self)
        return self._plan

    def forward(self, x):
        if isinstance(x, TiledZSpectrum) or (
                self.fused_inference and not self.training and not torch.is_grad_enabled() and x.is_cuda
                and x.dtype == torch.float32 and x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0 and x.shape[4] % 4 == 0):
            return self._get_plan().run(x)
        return self.output_layer(self.encoder_decoder(self.front_layers(x)))

    def input_view(self, B, X, Y, Z, device):
        """where the next inference forward wants its (B,Cin,X,Y,Z) input written (a view of the FFT opening conv's
        padded buffer), or None when any tensor will do"""
        if not (self.wants_planar_input() and torch.device(device).type == "cuda" and X % 4 == 0 and Y % 4 == 0 and Z % 4 == 0):
            return None
        return self._get_plan().fft_input_view(B, X, Y, Z, device)

    def input_chunk_views(self, P, chunk, X, Y, Z, device):
        """for a caller that produces P inputs at once and feeds them in chunks of `chunk` (tail rounded up to a power
        of two): ONE zero-padded buffer for all of them -> (view of the first P inputs to write into, list of per-chunk
        views to pass to forward()).  None when the next forward does not take the FFT opening conv."""
        first = self.input_view(1, X, Y, Z, device)
        if first is None:
            return None
        cin = first.shape[1]
        S = _FoldedV2V._fft_shape(X, Y, Z, 7)          # input_view answers for the 7x7x7 FFT opening conv only
        sizes = []
        s0 = 0
        while s0 < P:
            n = min(chunk, P - s0)
            sizes.append((s0, n, 1 << (n - 1).bit_length()))
            s0 += n
        total = sizes[-1][0] + sizes[-1][2]
        buf = self._plan._fft_buffer(total, cin, S, device)
        whole = buf[:P, :, :X, :Y, :Z]
        chunks = [(n, buf[a:a + m, :, :X, :Y, :Z]) for a, n, m in sizes]
        return whole, chunks

    def wants_channels_last_cubes(self, X, Y, Z) -> bool:
        """True when the next inference forward's opening conv reads channels-last 16-channel cubes directly (direct
        z-DFT form, root grid): the caller should ask the unprojection for its channels-last result, not fill input_view"""
        if not (self.wants_planar_input() and getattr(self, "zdft", True) and self.front_layers[0].block[0].kernel_size == (7, 7, 7)):
            return False
        w0, w1 = self.front_layers[0].block[0].weight, self.front_layers[1].res_branch[0].weight
        return bool(w0.is_cuda and _zdft_front_ok(w0, w1, Z, _FoldedV2V._fft_shape(X, Y, Z, 7)[2]))

    def wants_zspectrum(self, X, Y, Z, cin: int):
        """SZ when the next inference forward can start from the cubes' z-spectrum (``TiledZSpectrum``: the unprojection
        fused with the opening conv's z pass, root grid), else None.  ``fuse_zdft`` (default on; SP3D_FUSE_ZDFT=0 turns it
        off for A/B) and the conditions of the direct z-DFT form + 88 x 88 planes + a float32 inference plan.  With
        ``wide_front`` (default off; SP3D_WIDE_FRONT=1) it also answers for 17 <= cin <= 32 (_wide_front_ok), with
        ``one_front`` (default off; SP3D_ONE_FRONT=1) for cin == 1 (_one_front_ok); without it cin == 1 is None - no
        unprojection delivers the spectrum of one channel otherwise."""
        from . import _lib
        if not getattr(self, "fuse_zdft", _lib.env_switch("SP3D_FUSE_ZDFT", True)):
            return None
        if self.training or torch.is_grad_enabled() or not self.fused_inference:
            return None
        w0 = self.front_layers[0].block[0].weight
        if 17 <= int(cin) <= 32:      # opt-in: the spectrum of 17..32 channels, one unprojection launch per channel group
            if not (getattr(self, "wide_front", False) and self.wants_planar_input() and getattr(self, "zdft", True) and w0.is_cuda
                    and tuple(w0.shape[2:]) == (7, 7, 7)
                    and _wide_front_ok(w0, self.front_layers[1].res_branch[0].weight, Z, _FoldedV2V._fft_shape(X, Y, Z, 7)[2])):
                return None
        elif int(cin) == 1:           # opt-in: the spectrum of the one channel of the ROOTNET_ROOTHM root nets, one launch
            if not (getattr(self, "one_front", False) and self.wants_planar_input() and getattr(self, "zdft", True) and w0.is_cuda
                    and _one_front_ok(w0, self.front_layers[1].res_branch[0].weight, Z, _FoldedV2V._fft_shape(X, Y, Z, 7)[2])):
                return None
        elif not self.wants_channels_last_cubes(X, Y, Z):
            return None
        S = _FoldedV2V._fft_shape(X, Y, Z, int(w0.shape[2]))
        if S[0] != 88 or S[1] != 88 or X % 4 or Y % 4 or int(w0.shape[1]) != int(cin) or w0.dtype != torch.float32:
            return None
        return int(S[2])

    def wants_planar_input(self) -> bool:
        """True when the next forward will take the FFT opening conv: it reads plain (B,C,X,Y,Z) cubes with the real
        channel count, so the caller need not pad channels or emit channels-last cubes."""
        return bool(self.fused_inference and self.fft_front and not self.training and not torch.is_grad_enabled())
