"""Cases, inputs, float64 referees and the comparison of the conv / up-conv sweep (tests/test_conv_sweep_reference.py on
the CPU, tests/test_gpu_conv_sweep.py on the GPU).  A plain helper: no pytest hooks, nothing here touches a GPU.

ROWS: one row per kernel instantiation family of the V2V inference plan - the _lib entry, its (C, O) widths, the output
block it tiles with, its epilogue modes and the rule its error is held to.
grids(block): the grid classes of a block - degenerate, thinner than a block, exactly one, one + a voxel in every axis,
ragged x / y, interior, interior + ragged.  upconv_grids(): the same idea for the 128-voxel tiles of the up-conv kernels,
which run over the voxels of the whole batch.  walk_grids(cus): grids on which the persistent workgroups of
conv3_split_kernel walk two and three blocks, computed from the CU count as conv3_split_launch computes its launch.
make_weights / make_inputs: everything from fixed seeds on the CPU.  Sample b of a batch is 10^(3b) times larger (x,
residual, skip), so a read from the neighbouring sample swamps sample 0; errors are therefore taken per sample.
referee: float64 F.conv3d / F.conv_transpose3d + the epilogue; naive_referee: the same by shift-and-add in NumPy."""
import collections
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.test_gpu_v2v_plan_f64 import BOUNDS

Row = collections.namedtuple("Row", "name entry widths block modes bound rule kw")
# rule: "bound" - the per-sample error is held to `bound`; "three_launch" - no plan bound: the parity-test rule against the
# three-launch form on the same inputs, e <= 1.5 e_three + 1e-7 (absolute errors; tests/test_gpu_parity.py); "gemm" - the
# up-conv entries: the GEMM + scatter form is held to `bound`, the fused form to it and to 1.5x the GEMM + scatter form's
# error (tests/test_gpu_upconv_fused.py)
ALL_MODES = (0, 1, 2, 3)
ROWS = (
    Row("conv3_split", "conv3_split_", ((16, 32), (32, 32)), (16, 8, 4), ALL_MODES, BOUNDS["conv3_split_"], "bound", dict(walk=True)),
    Row("conv3_split_skip", "conv3_split_", ((32, 32),), (16, 8, 4), (1,), BOUNDS["conv3_split_"], "bound", dict(walk=True, skip=16)),
    Row("wino_fused_fp32", "wino_fused_conv3d_", ((16, 32), (32, 32)), (8, 8, 4), ALL_MODES, None, "three_launch", dict()),
    Row("wino_fused_split8", "wino_fused_conv3d_", ((16, 32), (32, 32)), (8, 8, 4), ALL_MODES, None, "three_launch", dict(chunk=8)),
    Row("wino_fused_split16", "wino_fused_conv3d_", ((32, 64), (64, 64)), (8, 8, 2), ALL_MODES, BOUNDS["wino_fused_conv3d_"], "bound",
        dict(chunk=16)),
    Row("wino_fused_split16_skip", "wino_fused_conv3d_", ((64, 64),), (8, 8, 2), (1,), BOUNDS["wino_fused_conv3d_"], "bound",
        dict(chunk=16, skip=32)),
    Row("conv3_split128", "conv3_split128_", ((64, 128), (128, 128)), (5, 5, 5), ALL_MODES, 2.0e-6, "bound", dict()),
    Row("wino_three_launch", "wino_conv3d_", ((8, 4), (64, 128), (128, 128)), (2, 2, 2), ALL_MODES, BOUNDS["wino_conv3d_"], "bound",
        dict(library_gemm=True)),
    Row("upsample2x", "upsample2x_", ((128, 64),), None, (None,), BOUNDS["upsample2x_"], "gemm", dict()),
    Row("upsample2x_head", "upsample2x_head_", ((64, 32, 1), (64, 32, 15)), None, (None,), BOUNDS["upsample2x_head_"], "gemm", dict()),
)
ROW = {r.name: r for r in ROWS}
UPCONV_TILE = 128


def effective_bound(row):
    """the largest error a row's rule can let through when the form it is compared with keeps its own bound"""
    if row.rule == "three_launch":
        return 1.5 * BOUNDS["wino_conv3d_"] + 1e-7
    return row.bound


def grids(block):
    """the grid classes of a (bx, by, bz) output block, name -> (X, Y, Z)"""
    bx, by, bz = block
    return collections.OrderedDict([
        ("unit", (1, 1, 1)),
        ("thin", (1, 2, 3)),
        ("one_block", (bx, by, bz)),
        ("one_block_plus_1", (bx + 1, by + 1, bz + 1)),
        ("ragged_xy", (2 * bx - 1, by + 1, bz)),
        ("interior", (3 * bx, 3 * by, 3 * bz)),
        ("interior_ragged", (2 * bx + 3, 2 * by + 1, 2 * bz + 1)),
    ])


def upconv_grids():
    """name -> (B, (X, Y, Z)) of the up-conv rows: the kernels tile the B*X*Y*Z input voxels of the whole batch by 128"""
    g = collections.OrderedDict([
        ("unit", (1, (1, 1, 1))),
        ("below_tile", (1, (5, 5, 2))),                 # 50 voxels
        ("below_tile_b2", (2, (3, 4, 5))),              # 120 voxels, the sample boundary inside the only tile
        ("one_tile", (1, (8, 8, 2))),
        ("one_tile_b2", (2, (8, 4, 2))),                # exactly one tile made of two samples
        ("tile_plus_ragged", (2, (6, 5, 3))),           # 180 voxels: a full tile that ends inside sample 1 + a ragged one
        ("tile_plus_one", (1, (43, 3, 1))),             # 129 voxels: a ragged tile of one voxel
        ("multi", (1, (32, 24, 20))),                   # 120 tiles: the *_multi grid of tests/test_gpu_upconv_fused.py
    ])
    for name, (B, (X, Y, Z)) in g.items():
        n = B * X * Y * Z
        assert {"unit": n < UPCONV_TILE, "below": n < UPCONV_TILE, "one": n == UPCONV_TILE,
                "tile": UPCONV_TILE < n < 2 * UPCONV_TILE, "multi": n > 100 * UPCONV_TILE}[name.split("_")[0]], (name, n)
    return g


def launch_of(blocks, cus):
    """(rounds, workgroups) conv3_split_launch gives `blocks` output blocks on `cus` compute units"""
    rounds = (blocks + cus - 1) // cus
    return rounds, (blocks + rounds - 1) // rounds


def walked(blocks, nwg):
    """blocks each workgroup walks: conv3_split_kernel's my_blocks"""
    return [(blocks - 1 - i) // nwg + 1 if i < blocks else 0 for i in range(nwg)]


def _factor(n):
    """n = a * b with a <= b and a as large as possible"""
    a = int(n ** 0.5)
    while n % a:
        a -= 1
    return a, n // a


def walk_grids(cus):
    """name -> (B, (X, Y, Z)) for the two conv3_split_ rows on a device of `cus` compute units.  X = 16 (one block along x);
    two_rounds: B = 1, an odd number of blocks in (cus, 2 cus] - the last workgroup walks one block, the others two;
    three_rounds: B = 2, blocks in (2 cus, 3 cus] and no multiple of 3 - workgroups walk two or three blocks and every
    walk crosses the sample boundary.  Each with whole blocks only and with a ragged last block in y and in z."""
    bx, by, bz = ROW["conv3_split"].block
    out = collections.OrderedDict()

    def first(lo, hi, ok):
        for n in range(lo, hi + 1):
            a, b = _factor(n)
            if ok(n) and a >= 5:                        # at least 5 x 5 blocks in (y, z): interior and edge blocks
                return a, b
        raise ValueError(f"no walk grid for {cus} compute units")
    nbz, nby = first(cus + 1, 2 * cus, lambda n: n % 2 == 1)
    out["two_rounds_whole"] = (1, (bx, by * nby, bz * nbz))
    out["two_rounds_ragged"] = (1, (bx, by * nby - 3, bz * nbz - 1))
    nbz, nby = first(nby * nbz + 1, (3 * cus) // 2, lambda n: (2 * n) % 3 != 0)          # another grid than the two-round one
    out["three_rounds_whole"] = (2, (bx, by * nby, bz * nbz))
    out["three_rounds_ragged"] = (2, (bx, by * nby - 3, bz * nbz - 1))
    return out


def block_count(B, grid, block):
    return B * int(np.prod([(g + b - 1) // b for g, b in zip(grid, block)]))


def cases(row, cus=None):
    """every (class name, B, grid) a row runs: its grid classes at B = 2 (sample 0 alone is the B = 1 run of the batch
    position check), the up-conv tile classes, and the walk grids for `cus` compute units where the row walks"""
    if row.block is None:
        return [(name, B, grid) for name, (B, grid) in upconv_grids().items()]
    out = [(name, 2, grid) for name, grid in grids(row.block).items()]
    if cus is not None and row.kw.get("walk"):
        out += [(name, B, grid) for name, (B, grid) in walk_grids(cus).items()]
    return out


def at_least_one_block(row, B, grid):
    if row.block is None:
        return B * int(np.prod(grid)) >= UPCONV_TILE
    return all(g >= b for g, b in zip(grid, row.block))


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


def make_weights(row, width):
    """fp32 CPU weights of a (row, width): w ~ N(0,1) / sqrt(taps C), shift ~ 0.5 N(0,1); skip / head weights alike"""
    g = _gen("weights", row.name, width)
    C, O = width[:2]
    if row.block is None:
        w = dict(wT=torch.randn(C, O, 2, 2, 2, generator=g) / C ** 0.5, shift=0.5 * torch.randn(O, generator=g))
        if len(width) == 3:
            J = width[2]
            w["wo"] = torch.randn(J, O, 1, 1, 1, generator=g) / O ** 0.5
            w["bo"] = 0.5 * torch.randn(J, generator=g)
        return w
    w = dict(w=torch.randn(O, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5, shift=0.5 * torch.randn(O, generator=g))
    if row.kw.get("skip"):
        CS = row.kw["skip"]
        w["ws"] = torch.randn(O, CS, 1, 1, 1, generator=g) / CS ** 0.5
    return w


def sample_scale(B):
    return torch.tensor([10.0 ** (3 * b) if b < 2 else 1.0 for b in range(B)]).view(B, 1, 1, 1, 1)


def make_inputs(row, width, B, grid):
    """fp32 CPU activations of a case: x ~ N(0,1) times a per-channel factor 2^U(-3,3), residual / skip ~ N(0,1), sample b
    times 10^(3b).  Sample 0 of a batch is the B = 1 case of the same grid (the generator draws sample by sample)."""
    C, O = width[:2]
    X, Y, Z = grid
    g = _gen("inputs", row.name, width, grid)
    chan = 2.0 ** (6.0 * torch.rand(C, generator=g) - 3.0)
    up = 2 if row.block is None else 1
    xs, rs, ss = [], [], []
    for _ in range(B):
        xs.append(torch.randn(1, C, X, Y, Z, generator=g) * chan.view(1, C, 1, 1, 1))
        rs.append(torch.randn(1, O, up * X, up * Y, up * Z, generator=g))
        if row.kw.get("skip"):
            ss.append(torch.randn(1, row.kw["skip"], X, Y, Z, generator=g))
    s = sample_scale(B)
    ins = dict(x=torch.cat(xs) * s, res=torch.cat(rs) * s)
    if ss:
        ins["xs"] = torch.cat(ss) * s
    return ins


def first_sample(ins):
    return {k: v[:1].clone() for k, v in ins.items()}


# ---- referees -------------------------------------------------------------------------------------------------------------
def conv3d_f64(x, w, budget=1 << 28):
    """'same' float64 3x3x3 convolution over x-slabs with a halo (the library's float64 path unfolds C * 27 values per
    output voxel: each call sees at most `budget` bytes of that)"""
    B, C, X, Y, Z = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    slab = max(1, min(X, budget // max(1, B * C * 27 * Y * Z * 8)))
    out = torch.empty((B, int(w.shape[0]), X, Y, Z), dtype=x.dtype, device=x.device)
    for x0 in range(0, X, slab):
        x1 = min(X, x0 + slab)
        out[:, :, x0:x1] = F.conv3d(xp[:, :, x0:x1 + 2], w)
    return out


def referee_core(row, weights, ins):
    """the float64 part every mode of a case shares: the convolution (+ the folded skip projection), before the epilogue"""
    d = {k: v.double() for k, v in weights.items()}
    x = ins["x"].double()
    if row.block is None:
        return F.conv_transpose3d(x, d["wT"], None, 2)
    c = conv3d_f64(x, d["w"])
    if "ws" in d:
        c = c + F.conv3d(ins["xs"].double(), d["ws"])
    return c


def epilogue(row, weights, ins, core, mode):
    """float64 epilogue as the existing tests spell it: mode 0 c + shift; 1 relu(c + shift); 2 relu(c + shift + res);
    3 relu(c + shift) + res; the up-conv rows relu(c + shift) + skip (+ the 1x1x1 output conv)"""
    O = core.shape[1]
    y = core + weights["shift"].double().to(core.device).view(1, O, 1, 1, 1)
    res = ins["res"].double()
    if row.block is None:
        y = y.clamp_min(0) + res
        if "wo" in weights:
            y = F.conv3d(y, weights["wo"].double().to(core.device), weights["bo"].double().to(core.device))
        return y
    if mode == 2:
        y = y + res
    if mode >= 1:
        y = y.clamp_min(0)
    if mode == 3:
        y = y + res
    return y


def referee(row, weights, ins, mode):
    return epilogue(row, weights, ins, referee_core(row, weights, ins), mode)


def naive_referee(row, weights, ins, mode):
    """the same layer in NumPy float64 without any library convolution: one shifted multiply-add per tap"""
    w = {k: v.double().numpy() for k, v in weights.items()}
    x, res = ins["x"].double().numpy(), ins["res"].double().numpy()
    B, C, X, Y, Z = x.shape
    if row.block is None:
        O = w["wT"].shape[1]
        y = np.zeros((B, O, 2 * X, 2 * Y, 2 * Z))
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    y[:, :, i::2, j::2, k::2] = np.einsum("bcxyz,co->boxyz", x, w["wT"][:, :, i, j, k])
        y = np.maximum(y + w["shift"].reshape(1, O, 1, 1, 1), 0.0) + res
        if "wo" in w:
            y = np.einsum("boxyz,jo->bjxyz", y, w["wo"][:, :, 0, 0, 0]) + w["bo"].reshape(1, -1, 1, 1, 1)
        return torch.from_numpy(y)
    O = w["w"].shape[0]
    xp = np.zeros((B, C, X + 2, Y + 2, Z + 2))
    xp[:, :, 1:-1, 1:-1, 1:-1] = x
    y = np.zeros((B, O, X, Y, Z))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                y += np.einsum("bcxyz,oc->boxyz", xp[:, :, i:i + X, j:j + Y, k:k + Z], w["w"][:, :, i, j, k])
    if "ws" in w:
        y += np.einsum("bcxyz,oc->boxyz", ins["xs"].double().numpy(), w["ws"][:, :, 0, 0, 0])
    y += w["shift"].reshape(1, O, 1, 1, 1)
    if mode == 2:
        y += res
    if mode >= 1:
        y = np.maximum(y, 0.0)
    if mode == 3:
        y += res
    return torch.from_numpy(y)


# ---- comparison -----------------------------------------------------------------------------------------------------------
def compare(got, ref):
    """per sample: err = max|got - ref| / max(1, max|ref|), abs = max|got - ref|, range = max|ref|, pos = the share of
    positive reference values (the signal figures of tests/test_gpu_v2v_plan_f64.py) -> dict of lists"""
    B = ref.shape[0]
    d = (got.double() - ref).abs().reshape(B, -1).amax(1)
    amax = ref.abs().reshape(B, -1).amax(1)
    pos = (ref > 0).double().reshape(B, -1).mean(1)
    return dict(err=(d / amax.clamp_min(1.0)).tolist(), abs=d.tolist(), range=amax.tolist(), pos=pos.tolist())


def has_signal(row, mode, B, grid, cmp):
    """10-90 % positive outputs in the ReLU modes (the head's outputs follow no ReLU), on grids of at least one block"""
    relu = (mode is None and "head" not in row.name) or (mode is not None and mode >= 1)
    if not relu or not at_least_one_block(row, B, grid):
        return True
    return all(0.1 <= p <= 0.9 for p in cmp["pos"])
