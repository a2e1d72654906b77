"""Cases, inputs, float64 referees and the comparison of the opening-conv sweep (tests/test_front_sweep_reference.py on the
CPU, tests/test_gpu_front_sweep.py on the GPU).  A plain helper: no pytest hooks, nothing here touches a GPU.

ROWS: one row per kernel of the frequency-domain 7x7x7 opening conv - the _lib entry, the rule its error is held to and
the factor of that rule.  cases(row): the boundary classes of that kernel's tiling (16-position tiles of zdft_fwd_cl, 16-row
y tiles of zdft_inv_cl, rows_in / rows_out of the 88 x 88 plane transform, the BB / OG instantiations of the contractions,
4-row blocks in groups of 8 of freq_contract_ty, ...) - for the contractions by pairwise coverage (pairwise()).
Inputs come from fixed seeds on the CPU; sample / plane b of a batch is 10^(3b) times larger than sample 0 (b < 2), so a read
from the neighbouring sample swamps sample 0, and errors are taken per sample as max|got - f64| / max(1, max|f64|).
Referees: float64 / complex128 torch.fft, einsum and slices; naive_*: the same by DFT matrices, loops or shift-and-add."""
import collections
import itertools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.test_gpu_v2v_plan_f64 import BOUNDS

Row = collections.namedtuple("Row", "name entries rule factor why")
# rule "library": no project bound exists for a stage of the opening conv, so the hand-written kernel is held to the library's
# fp32 form of the same operation on the same inputs, both measured against float64: e <= factor * e_library + 1e-7 (1.5: the
# project's rule for a hand-written form next to a library form, tests/test_gpu_parity.py; 1e-7: one fp32 rounding of a
# unit-range value, for the cases the library gets exactly).  A factor above 1.5 carries the measured ratio and the reason.
# rule "bound": the whole front, BOUNDS["front"] of tests/test_gpu_v2v_plan_f64.py.  rule "bits": bit-identity with the
# two-kernel form (+ the library rule for the spectrum, + the oracle for the cubes behind it).
F_HAND = 1.5
ROWS = (
    Row("zdft_fwd_cl", ("zdft_fwd_cl",), "library", F_HAND, None),
    Row("zdft_inv_cl", ("zdft_inv_cl",), "library", F_HAND, None),
    Row("cfft2d_88", ("cfft2d_",), "library", F_HAND, None),
    Row("cfft2d_88_tiled", ("cfft2d_88_tiled",), "library", F_HAND, None),
    Row("freq_contract", ("freq_contract", "freq_contract_ex"), "library", F_HAND, None),
    Row("freq_contract_ty", ("freq_contract_ty",), "library", F_HAND, None),
    Row("crop_shift_act_cl", ("crop_shift_act_cl",), "library", F_HAND, None),
    Row("unproject_fwd_zdft", ("unproject_fwd_zdft",), "bits", F_HAND, None),
    Row("front", (), "bound", None, None),
)
ROW = {r.name: r for r in ROWS}
OUT_ENTRIES = ("zdft_fwd_cl", "zdft_inv_cl", "cfft2d_88_tiled", "freq_contract", "freq_contract_ty", "freq_contract_ex",
               "crop_shift_act_cl", "unproject_fwd_zdft")
# the library form a stage row is compared with must itself be a sound yardstick: its own error stays under LIB_CAP, so that
# no rule lets more through than the 3e-6 x scale tests/test_gpu_parity.py allows the FFT kernels
PARITY_CAP = 3e-6
LIB_CAP = (PARITY_CAP - 1e-7) / F_HAND
Z, SZ, KZ, CH = 20, 28, 15, 16                    # the one shape the direct z-DFT kernels are built for
ZD_TILE = 16


def effective_bound(row):
    """the largest error a row's rule can let through"""
    if row.rule == "bound":
        return BOUNDS["front"]
    return row.factor * LIB_CAP + 1e-7


def pairwise(factors):
    """a small set of combinations of ``factors`` (name -> values) in which every pair of values of two different factors
    occurs together: greedy over the full product in its fixed order -> list of dicts"""
    names = list(factors)
    need = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in factors[a] for vb in factors[b]}
    product = [dict(zip(names, vs)) for vs in itertools.product(*factors.values())]
    out = []
    while need:
        def gain(c):
            return sum((a, c[a], b, c[b]) in need for a, b in itertools.combinations(names, 2))
        best = max(product, key=gain)
        out.append(best)
        need -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(names, 2)}
    return out


def covers_pairwise(cases, factors):
    names = list(factors)
    have = {(a, c[a], b, c[b]) for c in cases for a, b in itertools.combinations(names, 2)}
    return all((a, va, b, vb) in have for a, b in itertools.combinations(names, 2) for va in factors[a] for vb in factors[b])


# ---- case tables ----------------------------------------------------------------------------------------------------------
ZFWD_CLASSES = collections.OrderedDict([             # name -> (X, Y, SX, SY): the padded plane SX * SY against the 16-position tile
    ("below_tile", (1, 1, 2, 6)),                    # plane 12 < 16
    ("one_tile", (2, 3, 4, 4)),                      # plane == 16
    ("straddle", (20, 18, 22, 18)),                  # plane 396 = 16 * 24 + 12, SY = 18: every tile straddles two rows
    ("no_padding", (4, 6, 4, 6)),                    # X == SX and Y == SY
    ("run_small", (12, 10, 18, 16)),                 # the run shape's proportions
])
ZFWD_COUT = (1, 15, 16)
ZINV_CLASSES = (                                     # (X, Y, SX, SY): Y against the 16-row y tile, X == SX, SY == Y and SY > Y
    (1, 1, 2, 3), (3, 15, 3, 15), (3, 16, 5, 16), (1, 17, 1, 20), (3, 33, 4, 36),
    (1, 16, 1, 19), (3, 17, 3, 17), (1, 15, 2, 18), (3, 1, 3, 1), (1, 33, 1, 33),
)
F88 = 88
ROWS_88 = (1, 3, 75, 80, 82, 87, 88)
PAIRS_88 = ((1, 1), (80, 80), (88, 88), (87, 3), (3, 87), (75, 88), (88, 75), (82, 80), (80, 82))      # (rows_in, rows_out)
TILED_XY = ((4, 4), (4, 88), (88, 4), (76, 84), (80, 80), (88, 88))
CONTRACT_FACTORS = collections.OrderedDict([("I", (1, 2, 3, 4, 5)), ("J", (1, 8, 9, 16, 17)), ("K", (1, 15, 16)),
                                            ("F", (1, 255, 256, 257, 513)), ("form", ("plain", "fwd", "dx", "dw"))])
TY_FACTORS = collections.OrderedDict([("rows", (1, 3, 4, 5, 31, 32, 33, 36)), ("O", (1, 4, 5, 16)), ("C", (1, 15, 16)),
                                      ("SY", (8, 20, 88, 96)), ("B", (1, 4, 5))])
TY_PLAN = dict(S=(8, 20, 28), C=15, O=16, B=2)       # (T, tw) of _FoldedV2V._weights_ty instead of arbitrary tables
CROP_CLASSES = collections.OrderedDict([             # name -> (C, X, Y, Z, SX, SY, SZ); the kernel takes 4 y columns per block
    ("thin", (4, 1, 1, 4, 2, 3, 8)),
    ("ragged", (16, 3, 5, 8, 5, 7, 12)),
    ("no_crop", (8, 2, 4, 4, 2, 4, 4)),
])
UNPROJECT_CASES = (                                  # grid, views, valid flags of the B = 2 samples; heat-maps 32 x 24
    dict(cube=(4, 4, 20), V=1, valid=(1, 1)),
    dict(cube=(8, 12, 20), V=5, valid=(1, 0)),
    dict(cube=(76, 84, 20), V=5, valid=(1, 1)),
)
UNPROJECT_HM, UNPROJECT_IMG, UNPROJECT_J = (32, 24), (128, 96), 15           # (w, h)
FRONT_ROUTES = collections.OrderedDict([
    # name -> net input channels, channels of the input tensor, grid, B, channels-last input, contract_ty, the _lib entries
    # the route must call and those it must not
    ("zdft_library_planes", dict(cin=15, fc=16, grid=(12, 10, 20), B=2, cl=True, ty=False,
                                 calls=("zdft_fwd_cl", "cfft2d_", "freq_contract", "zdft_inv_cl"),
                                 never=("rfft3d", "irfft3d_", "freq_contract_ty", "crop_shift_act_cl", "channel_shift_act_"))),
    ("zdft_88_planes", dict(cin=15, fc=16, grid=(76, 82, 20), B=2, cl=True, ty=False,
                            calls=("zdft_fwd_cl", "cfft2d_", "freq_contract", "zdft_inv_cl"),
                            never=("rfft3d", "irfft3d_", "freq_contract_ty", "crop_shift_act_cl", "channel_shift_act_"))),
    ("zdft_88_planes_ty", dict(cin=15, fc=16, grid=(76, 82, 20), B=2, cl=True, ty=True,
                               calls=("zdft_fwd_cl", "cfft2d_", "freq_contract_ty", "zdft_inv_cl"),
                               never=("rfft3d", "irfft3d_", "freq_contract", "crop_shift_act_cl", "channel_shift_act_"))),
    # beyond the grids above: the same planes from the unprojection's tiled z-spectrum (_front_zspectrum), rows_in = 76
    ("zspectrum_88_planes", dict(cin=15, fc=16, grid=(76, 80, 20), B=2, cl=True, ty=False,
                                 calls=("cfft2d_88_tiled", "cfft2d_", "freq_contract", "zdft_inv_cl"),
                                 never=("rfft3d", "irfft3d_", "freq_contract_ty", "crop_shift_act_cl", "channel_shift_act_"))),
    ("rfft_cin15", dict(cin=15, fc=15, grid=(6, 5, 8), B=2, cl=False, ty=False,
                        calls=("rfft3d", "freq_contract", "irfft3d_", "crop_shift_act_cl"),
                        never=("zdft_fwd_cl", "zdft_inv_cl", "cfft2d_", "freq_contract_ty", "channel_shift_act_"))),
    ("rfft_cin1", dict(cin=1, fc=4, grid=(8, 8, 4), B=2, cl=True, ty=False,
                       calls=("rfft3d", "freq_contract", "irfft3d_", "crop_shift_act_cl"),
                       never=("zdft_fwd_cl", "zdft_inv_cl", "cfft2d_", "freq_contract_ty", "channel_shift_act_"))),
    ("rfft_z_not_4", dict(cin=15, fc=15, grid=(6, 5, 6), B=2, cl=False, ty=False,
                          calls=("rfft3d", "freq_contract", "irfft3d_", "channel_shift_act_"),
                          never=("zdft_fwd_cl", "zdft_inv_cl", "cfft2d_", "freq_contract_ty", "crop_shift_act_cl"))),
])


def cases(row):
    """every case of a row, a list of dicts (``kind`` tells the runner what to launch)"""
    n = row.name
    if n == "zdft_fwd_cl":
        return [dict(kind="zfwd", cls=c, dims=d, cout=co, B=B) for c, d in ZFWD_CLASSES.items() for co in ZFWD_COUT for B in (1, 2)]
    if n == "zdft_inv_cl":
        return [dict(kind="zinv", dims=d, relu=r, B=B) for d in ZINV_CLASSES for r in (True, False) for B in (1, 2)]
    if n == "cfft2d_88":
        out = [dict(kind="f88", rows=p, inverse=inv, planes=nb) for p in PAIRS_88 for inv in (False, True) for nb in (1, 3)]
        out.append(dict(kind="f88_unaligned", rows=(88, 88), inverse=False, planes=1))
        out.append(dict(kind="f_other", size=(48, 32), rows=(48, 48), inverse=False, planes=3))
        return out
    if n == "cfft2d_88_tiled":
        return [dict(kind="tiled", xy=xy, planes=nb) for xy in TILED_XY for nb in (1, 3)]
    if n == "freq_contract":
        return [dict(kind="contract", **c) for c in pairwise(CONTRACT_FACTORS)]
    if n == "freq_contract_ty":
        return [dict(kind="ty", **c) for c in pairwise(TY_FACTORS)] + [dict(kind="ty_plan", **TY_PLAN)]
    if n == "crop_shift_act_cl":
        return [dict(kind="crop", cls=c, dims=d, relu=r, B=2) for c, d in CROP_CLASSES.items() for r in (True, False)]
    if n == "unproject_fwd_zdft":
        return [dict(kind="unproject", **c) for c in UNPROJECT_CASES]
    if n == "front":
        return [dict(kind="front", route=r, **c) for r, c in FRONT_ROUTES.items()]
    raise KeyError(n)


def tag_of(case):
    return tuple((k, v) for k, v in case.items() if k not in ("calls", "never"))


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


def sample_scale(B, dims):
    """(B, 1, ..., 1): sample b is 10^(3b) times sample 0 for b < 2 (the third of three planes is as small as the first)"""
    return torch.tensor([10.0 ** (3 * b) if b < 2 else 1.0 for b in range(B)]).view((B,) + (1,) * (dims - 1))


def _randn(g, B, shape, cplx=False, scaled=True):
    """(B,) + shape, N(0,1) drawn sample by sample (sample 0 of a batch is the B = 1 case), times the sample scale"""
    if cplx:
        x = torch.cat([torch.view_as_complex(torch.randn((1,) + tuple(shape) + (2,), generator=g)) for _ in range(B)])
    else:
        x = torch.cat([torch.randn((1,) + tuple(shape), generator=g) for _ in range(B)])
    return x * sample_scale(B, x.dim()) if scaled else x


def tile44(planes):
    """(..., X, Y) -> (..., X/4, Y/4, 16): the 4 x 4-tiled plane layout of sp3d_unproject_fwd_zdft"""
    X, Y = planes.shape[-2:]
    lead = tuple(planes.shape[:-2])
    n = len(lead)
    t = planes.reshape(lead + (X // 4, 4, Y // 4, 4)).permute(*range(n), n, n + 2, n + 1, n + 3)
    return t.reshape(lead + (X // 4, Y // 4, 16)).contiguous()


def untile44(spec, X, Y):
    lead = tuple(spec.shape[:-3])
    n = len(lead)
    return spec.reshape(lead + (X // 4, Y // 4, 4, 4)).permute(*range(n), n, n + 2, n + 1, n + 3).reshape(lead + (X, Y))


def make_inputs(case):
    """the fp32 / complex64 CPU inputs of a case, name -> tensor"""
    k = case["kind"]
    g = _gen("front sweep", tag_of(case))
    if k == "zfwd":
        X, Y, _, _ = case["dims"]
        return dict(x=_randn(g, case["B"], (CH, X, Y, Z)))
    if k == "zinv":
        X, Y, SX, SY = case["dims"]
        v = _randn(g, case["B"], (CH, SX, SY, SZ)).double()                       # spectra of real volumes
        spec = torch.fft.rfft(v, dim=-1, norm="forward").permute(0, 1, 4, 2, 3).contiguous().to(torch.complex64)
        return dict(spec=spec, shift=0.5 * torch.randn(CH, generator=g))
    if k in ("f88", "f88_unaligned", "f_other"):
        SX, SY = case.get("size", (F88, F88))
        x = _randn(g, case["planes"], (SX, SY), cplx=True)
        x[:, case["rows"][0]:] = 0.0                                              # the GPU test puts NaN there
        return dict(x=x)
    if k == "tiled":
        X, Y = case["xy"]
        return dict(x=_randn(g, case["planes"], (X, Y), cplx=True))
    if k == "contract":
        I, J, K, Fn, form = (case[n] for n in ("I", "J", "K", "F", "form"))
        if form in ("plain", "fwd"):
            return dict(P=_randn(g, I, (K, Fn), cplx=True), Q=_randn(g, J, (K, Fn), True, False) / K ** 0.5)
        if form == "dx":
            return dict(P=_randn(g, I, (K, Fn), cplx=True), Q=_randn(g, K, (J, Fn), True, False) / K ** 0.5)
        P = _randn(g, I, (K, Fn), cplx=True).transpose(0, 1).contiguous()          # (K, I, F), output index i scaled
        return dict(P=P, Q=_randn(g, K, (J, Fn), True, False) / K ** 0.5)
    if k == "ty":
        rows, O, C, SY, B = (case[n] for n in ("rows", "O", "C", "SY", "B"))
        return dict(X=_randn(g, B, (C, 1, rows, SY), cplx=True), T=torch.randn((rows, O, C, 14), generator=g) / (7 * C) ** 0.5,
                    tw=torch.randn((SY, 3, 2), generator=g))
    if k == "ty_plan":
        S, C, O = case["S"], case["C"], case["O"]
        return dict(X=_randn(g, case["B"], (C, SZ // 2 + 1, S[0], S[1]), cplx=True),
                    w0=torch.randn((O, C, 7, 7, 7), generator=g) / (343 * C) ** 0.5 * S[0] * S[1] * S[2])
    if k == "crop":
        C, X, Y, Zc, SX, SY, SZc = case["dims"]
        return dict(src=_randn(g, case["B"], (C, SX, SY, SZc)), shift=0.5 * torch.randn(C, generator=g))
    if k == "front":
        X, Y, Zc = case["grid"]
        g = _gen("front", case["cin"], case["fc"], case["grid"], case["B"])      # the routes of one grid share their input
        return dict(x=_randn(g, case["B"], (case["fc"], X, Y, Zc)))
    raise KeyError(k)


def first_sample(ins, case):
    """the inputs of sample / plane 0 run alone"""
    k = case["kind"]
    if k == "contract":
        return dict(ins, P=ins["P"][:, :1].contiguous() if case["form"] == "dw" else ins["P"][:1].contiguous())
    keep = {"zfwd": ("x",), "zinv": ("spec",), "f88": ("x",), "tiled": ("x",), "ty": ("X",), "ty_plan": ("X",), "crop": ("src",),
            "front": ("x",)}[k]
    return {n: (v[:1].contiguous() if n in keep else v) for n, v in ins.items()}


def ty_plan_tables(w0, S):
    """(T, tw) of the plan for folded taps w0 on the FFT shape S, from _FoldedV2V._weights_ty itself (it needs no net)"""
    from selfpose3d_amd.v2v_net import _FoldedV2V
    return _FoldedV2V(None)._weights_ty(w0, tuple(S))


def unproject_inputs(case):
    """heat-maps, camera table, centres, valid flags of an unprojection case and the oracle's cubes (B, J, X, Y, Z)"""
    from oracle import oracle
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    B, V, J = len(case["valid"]), case["V"], UNPROJECT_J
    w, h = UNPROJECT_HM
    meta = syn.make_meta(B, V, UNPROJECT_IMG)
    hms = syn.random_heatmaps(B, V, J, h, w, seed=zlib.crc32(repr(tag_of(case)).encode()) % 1000)
    cam = pack_cameras(meta, B, UNPROJECT_IMG)
    centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), B, 0)
    centers[1, 0] += 250.0                                                          # the two samples see different voxels
    valid = np.asarray(case["valid"], np.uint8)
    cubes, _ = oracle.unproject_fwd([x.numpy() for x in hms], cam, centers, valid, syn.SPACE_SIZE, case["cube"], UNPROJECT_IMG,
                                    want_grids=False)
    return dict(hms=hms, cam=cam, centers=centers, valid=valid, cubes=torch.from_numpy(cubes), grid_size=syn.SPACE_SIZE)


def front_net(cin, channels_last):
    """a V2VNet (CPU, eval) whose opening conv and BatchNorm are far from the identity: unit-spread outputs, shifts of +-0.5"""
    from selfpose3d_amd.v2v_net import V2VNet
    g = _gen("front net", cin)
    net = V2VNet(cin, 1)
    conv, bn = net.front_layers[0].block[0], net.front_layers[0].block[1]
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (343 * cin) ** 0.5)
        conv.bias.copy_(0.1 * torch.randn(16, generator=g))
        bn.running_var.copy_(10.0 ** (2.0 * torch.rand(16, generator=g) - 1.0))
        bn.running_mean.copy_(2.0 * torch.rand(16, generator=g) - 1.0)
        bn.weight.copy_(bn.running_var.sqrt() * 2.0 ** (2.0 * torch.rand(16, generator=g) - 1.0))
        bn.bias.copy_(0.5 * torch.randn(16, generator=g))
    net.eval()
    if channels_last:
        net.to(memory_format=torch.channels_last_3d)
    return net


# ---- referees -------------------------------------------------------------------------------------------------------------
def pad_xy(x, SX, SY):
    """zero-pad the last two dims to (SX, SY)"""
    return F.pad(x, (0, SY - x.shape[-1], 0, SX - x.shape[-2]))


def ref_zfwd(x, cout, SX, SY):
    """(B,16,X,Y,20) real -> (B,cout,15,SX,SY) complex128: z-DFT of the rows zero-padded to 28, planes zero-padded"""
    s = torch.fft.rfft(x.double(), n=SZ, dim=-1)[:, :cout]                       # (B,cout,X,Y,15)
    return pad_xy(s.permute(0, 1, 4, 2, 3), SX, SY).contiguous()


def naive_zfwd(x, cout, SX, SY):
    z, k = torch.arange(Z, dtype=torch.float64), torch.arange(KZ, dtype=torch.float64)
    ang = -2.0 * math.pi * k[:, None] * z[None, :] / SZ
    M = torch.complex(torch.cos(ang), torch.sin(ang))                           # (15, 20)
    out = torch.zeros((x.shape[0], cout, KZ, SX, SY), dtype=torch.complex128)
    out[:, :, :, :x.shape[2], :x.shape[3]] = torch.einsum("kz,bcxyz->bckxy", M, x[:, :cout].to(torch.complex128))
    return out


def ref_zinv(spec, shift, X, Y, relu):
    """the kernel's formula in float64: shift[o] + f0.re + (-1)^z f14.re + 2 sum_{k=1..13} (re cos - im sin), optional ReLU
    (B,16,15,SX,SY) complex -> (B,16,X,Y,20) real"""
    f = spec.to(torch.complex128)[:, :, :, :X, :Y]
    z, k = torch.arange(Z, dtype=torch.float64), torch.arange(1, KZ - 1, dtype=torch.float64)
    ang = 2.0 * math.pi * k[:, None] * z[None, :] / SZ                           # (13, 20)
    y = 2.0 * (torch.einsum("bokxy,kz->boxyz", f[:, :, 1:KZ - 1].real, torch.cos(ang))
               - torch.einsum("bokxy,kz->boxyz", f[:, :, 1:KZ - 1].imag, torch.sin(ang)))
    sign = torch.where(torch.arange(Z) % 2 == 0, 1.0, -1.0).double()
    y = y + f[:, :, 0].real.unsqueeze(-1) + f[:, :, KZ - 1].real.unsqueeze(-1) * sign + shift.double().view(1, -1, 1, 1, 1)
    return y.clamp_min(0) if relu else y


def naive_zinv(spec, shift, X, Y, relu):
    """the unnormalised C2R of torch.fft (equal to the formula on a Hermitian spectrum), cropped, + shift, optional ReLU"""
    f = spec.to(torch.complex128).permute(0, 1, 3, 4, 2)
    y = torch.fft.irfft(f, n=SZ, dim=-1, norm="forward")[:, :, :X, :Y, :Z] + shift.double().view(1, -1, 1, 1, 1)
    return y.clamp_min(0) if relu else y


def ref_fft2(x, inverse):
    """unnormalised 2-D transform of complex planes in complex128 (inverse: the e^{+i} kernel)"""
    x = x.to(torch.complex128)
    return torch.fft.ifft2(x, norm="forward") if inverse else torch.fft.fft2(x)


def naive_fft2(x, inverse):
    SX, SY = x.shape[-2:]
    sgn = 1.0 if inverse else -1.0

    def dft(n):
        i = torch.arange(n, dtype=torch.float64)
        ang = sgn * 2.0 * math.pi * ((i[:, None] * i[None, :]) % n) / n
        return torch.complex(torch.cos(ang), torch.sin(ang))
    return torch.einsum("ux,bxy,vy->buv", dft(SX), x.to(torch.complex128), dft(SY))


def ref_contract(P, Q, form):
    P, Q = P.to(torch.complex128), Q.to(torch.complex128)
    if form == "plain":
        return torch.einsum("ikf,jkf->ijf", P, Q)
    if form == "fwd":
        return torch.einsum("ikf,jkf->ijf", P, Q.conj())
    if form == "dx":
        return torch.einsum("ikf,kjf->ijf", P, Q)
    return torch.einsum("kif,kjf->ijf", P.conj(), Q)


def naive_contract(P, Q, form):
    P, Q = P.to(torch.complex128).numpy(), Q.to(torch.complex128).numpy()
    if form in ("plain", "fwd"):
        I, K, Fn = P.shape
        J = Q.shape[0]
    elif form == "dx":
        I, K, Fn = P.shape
        J = Q.shape[1]
    else:
        K, I, Fn = P.shape
        J = Q.shape[1]
    out = np.zeros((I, J, Fn), np.complex128)
    for i in range(I):
        for j in range(J):
            for k in range(K):
                if form == "plain":
                    out[i, j] += P[i, k] * Q[j, k]
                elif form == "fwd":
                    out[i, j] += P[i, k] * np.conj(Q[j, k])
                elif form == "dx":
                    out[i, j] += P[i, k] * Q[k, j]
                else:
                    out[i, j] += np.conj(P[k, i]) * Q[k, j]
    return torch.from_numpy(out)


def ty_weights(T, tw, dtype=torch.float64):
    """W^[o,c,row,ky] = G + sum_u S_u cos_u + i D_u sin_u of the kernel's header, from T (rows,O,C,14) and tw (SY,3,2)
    -> (O, C, rows, SY) complex"""
    T, tw = T.to(dtype), tw.to(dtype)
    c = torch.view_as_complex(T.reshape(T.shape[:3] + (7, 2)).contiguous())      # (rows,O,C,7): G, S1, D1, S2, D2, S3, D3
    W = c[..., 0].unsqueeze(-1).expand(c.shape[:3] + (tw.shape[0],)).clone()
    for u in range(3):
        W = W + c[..., 1 + 2 * u].unsqueeze(-1) * tw[:, u, 0] + 1j * c[..., 2 + 2 * u].unsqueeze(-1) * tw[:, u, 1]
    return W.permute(1, 2, 0, 3)


def ref_ty(X, T, tw):
    """(B,C,KZ,SX,SY) x tables -> (B,O,KZ,SX,SY) complex128"""
    B, C, K, SX, SY = X.shape
    W = ty_weights(T, tw)
    return torch.einsum("bcrf,ocrf->borf", X.to(torch.complex128).reshape(B, C, K * SX, SY), W).reshape(B, -1, K, SX, SY)


def naive_ty(X, T, tw):
    B, C, K, SX, SY = X.shape
    x, t, w = X.to(torch.complex128).numpy().reshape(B, C, K * SX, SY), T.double().numpy(), tw.double().numpy()
    rows, O = t.shape[:2]
    out = np.zeros((B, O, rows, SY), np.complex128)
    for r in range(rows):
        for ky in range(SY):
            for o in range(O):
                for c in range(C):
                    p = t[r, o, c]
                    wr, wi = p[0], p[1]
                    for u in range(3):
                        cs, sn = w[ky, u]
                        wr += p[2 + 4 * u] * cs - p[2 + 4 * u + 3] * sn
                        wi += p[2 + 4 * u + 1] * cs + p[2 + 4 * u + 2] * sn
                    out[:, o, r, ky] += x[:, c, r, ky] * complex(wr, wi)
    return torch.from_numpy(out.reshape(B, O, K, SX, SY))


def plan_spectrum(w0, S):
    """conj(rfftn(taps centred on the origin)) / N in complex128, kz slowest: (O, C, SZ/2+1, SX, SY)"""
    k = int(w0.shape[2])
    wp = torch.zeros(tuple(w0.shape[:2]) + tuple(S), dtype=torch.float64)
    wp[:, :, :k, :k, :k] = w0.double()
    wp = torch.roll(wp, shifts=(-(k // 2),) * 3, dims=(2, 3, 4))
    return (torch.fft.rfftn(wp, dim=(2, 3, 4)).conj() / float(S[0] * S[1] * S[2])).permute(0, 1, 4, 2, 3).contiguous()


def ref_ty_plan(X, w0, S):
    return torch.einsum("bckxy,ockxy->bokxy", X.to(torch.complex128), plan_spectrum(w0, S))


def ref_crop(src, shift, X, Y, Zc, relu):
    y = src.double()[:, :, :X, :Y, :Zc] + shift.double().view(1, -1, 1, 1, 1)
    return y.clamp_min(0) if relu else y


def naive_crop(src, shift, X, Y, Zc, relu):
    s, sh = src.double().numpy(), shift.double().numpy()
    out = np.zeros((s.shape[0], s.shape[1], X, Y, Zc))
    for c in range(s.shape[1]):
        for x in range(X):
            for y in range(Y):
                v = s[:, c, x, y, :Zc] + sh[c]
                out[:, c, x, y] = np.maximum(v, 0.0) if relu else v
    return torch.from_numpy(out)


def ref_unproject_spectrum(cubes, J):
    """oracle cubes (B,J,X,Y,20) -> their z-spectrum (B,J,15,X,Y) complex128"""
    return torch.fft.rfft(cubes.double()[:, :J], n=SZ, dim=-1).permute(0, 1, 4, 2, 3).contiguous()


def ref_front(x, w0, s0, conv=None):
    """float64 F.conv3d(padding = 3) of the folded taps + the folded shift + ReLU; x may carry more channels than w0 reads"""
    cin = int(w0.shape[1])
    xd, wd = x.double()[:, :cin], w0.double()
    c = F.conv3d(xd, wd, padding=3) if conv is None else conv(xd, wd)
    return (c + s0.double().view(1, -1, 1, 1, 1)).clamp_min(0)


def naive_front(x, w0, s0):
    """the same by shift-and-add in NumPy"""
    cin = int(w0.shape[1])
    xd, w = x.double().numpy()[:, :cin], w0.double().numpy()
    B, _, X, Y, Zc = xd.shape
    xp = np.zeros((B, cin, X + 6, Y + 6, Zc + 6))
    xp[:, :, 3:-3, 3:-3, 3:-3] = xd
    y = np.zeros((B, w.shape[0], X, Y, Zc))
    for i in range(7):
        for j in range(7):
            for k in range(7):
                y += np.einsum("bcxyz,oc->boxyz", xp[:, :, i:i + X, j:j + Y, k:k + Zc], w[:, :, i, j, k])
    return torch.from_numpy(np.maximum(y + s0.double().numpy().reshape(1, -1, 1, 1, 1), 0.0))


def referee(case, ins, naive=False):
    """the float64 result of a case from its CPU inputs (every kind but "unproject" and "front", which need more than ins)"""
    k = case["kind"]
    if k == "zfwd":
        _, _, SX, SY = case["dims"]
        return (naive_zfwd if naive else ref_zfwd)(ins["x"], case["cout"], SX, SY)
    if k == "zinv":
        X, Y, _, _ = case["dims"]
        return (naive_zinv if naive else ref_zinv)(ins["spec"], ins["shift"], X, Y, case["relu"])
    if k in ("f88", "f88_unaligned", "f_other"):
        return (naive_fft2 if naive else ref_fft2)(ins["x"], case["inverse"])[:, :case["rows"][1]]
    if k == "tiled":
        return (naive_fft2 if naive else ref_fft2)(pad_xy(ins["x"], F88, F88), False)
    if k == "contract":
        return (naive_contract if naive else ref_contract)(ins["P"], ins["Q"], case["form"])
    if k == "ty":
        return (naive_ty if naive else ref_ty)(ins["X"], ins["T"], ins["tw"])
    if k == "ty_plan":
        if naive:                                       # the kernel's formula on the plan's fp32 tables
            return ref_ty(ins["X"], *ty_plan_tables(ins["w0"], case["S"]))
        return ref_ty_plan(ins["X"], ins["w0"], case["S"])
    if k == "crop":
        _, X, Y, Zc, _, _, _ = case["dims"]
        return (naive_crop if naive else ref_crop)(ins["src"], ins["shift"], X, Y, Zc, case["relu"])
    raise KeyError(k)


# ---- comparison -----------------------------------------------------------------------------------------------------------
def compare(got, ref):
    """per sample (index of dim 0): err = max|got - ref| / max(1, max|ref|), abs = max|got - ref|, range = max|ref|, pos = the
    share of positive reference values (real results; None for spectra) -> dict of lists.  A NaN in ``got`` gives err = nan,
    which fails every ``<=``."""
    B = ref.shape[0]
    cd = torch.complex128 if ref.is_complex() else torch.float64
    d = (got.to(cd) - ref).abs().reshape(B, -1).amax(1)                         # amax propagates NaN
    amax = ref.abs().reshape(B, -1).amax(1)
    pos = None if ref.is_complex() else (ref > 0).double().reshape(B, -1).mean(1).tolist()
    return dict(err=(d / amax.clamp_min(1.0)).tolist(), abs=d.tolist(), range=amax.tolist(), pos=pos)


def has_signal(case, cmp):
    """ReLU cases: 10-90 % positive outputs in every sample; every other case: a result that is not all zero"""
    if case.get("relu") or case["kind"] == "front":
        return all(0.1 <= p <= 0.9 for p in cmp["pos"])
    return all(r > 0.0 for r in cmp["range"])


def within(rule_factor, e, e_lib):
    """the library rule, per sample"""
    return all(a <= rule_factor * b + 1e-7 for a, b in zip(e, e_lib))
