"""The conv / up-conv sweep's own parts, without a GPU (tests/conv_sweep_cases.py): the table covers what it says, the walk
grids make persistent workgroups walk what they say, the float64 referee agrees with a naive shift-and-add convolution,
the comparison rejects altered outputs at every row's bound, and the referee's outputs have signal on every case."""
import inspect
import itertools

import pytest
import torch

from tests import conv_sweep_cases as sw

ROW_WIDTHS = [(r.name, w) for r in sw.ROWS for w in r.widths]
_ids = [f"{n}-{'x'.join(str(v) for v in w)}" for n, w in ROW_WIDTHS]


def test_table_covers_every_entry_width_mode_and_grid_class():
    """the rows are the kernel instantiation families of the inference plan; every (row, width, mode) meets every grid class"""
    want = {
        "conv3_split": ("conv3_split_", {(16, 32), (32, 32)}, (16, 8, 4), 4),
        "conv3_split_skip": ("conv3_split_", {(32, 32)}, (16, 8, 4), 1),
        "wino_fused_fp32": ("wino_fused_conv3d_", {(16, 32), (32, 32)}, (8, 8, 4), 4),
        "wino_fused_split8": ("wino_fused_conv3d_", {(16, 32), (32, 32)}, (8, 8, 4), 4),
        "wino_fused_split16": ("wino_fused_conv3d_", {(32, 64), (64, 64)}, (8, 8, 2), 4),
        "wino_fused_split16_skip": ("wino_fused_conv3d_", {(64, 64)}, (8, 8, 2), 1),
        "conv3_split128": ("conv3_split128_", {(64, 128), (128, 128)}, (5, 5, 5), 4),
        "wino_three_launch": ("wino_conv3d_", {(8, 4), (64, 128), (128, 128)}, (2, 2, 2), 4),
        "upsample2x": ("upsample2x_", {(128, 64)}, None, 1),
        "upsample2x_head": ("upsample2x_head_", {(64, 32, 1), (64, 32, 15)}, None, 1),
    }
    assert {r.name: (r.entry, set(r.widths), r.block, len(r.modes)) for r in sw.ROWS} == want
    for r in sw.ROWS:
        cs = sw.cases(r, cus=256)
        names = [c[0] for c in cs]
        assert len(set(names)) == len(names)
        if r.block is None:
            assert names == list(sw.upconv_grids()) and len(names) == 8
            continue
        bx, by, bz = r.block
        classes = dict((n, (B, g)) for n, B, g in cs)
        assert [classes[n] for n in sw.grids(r.block)] == [
            (2, (1, 1, 1)), (2, (1, 2, 3)), (2, (bx, by, bz)), (2, (bx + 1, by + 1, bz + 1)), (2, (2 * bx - 1, by + 1, bz)),
            (2, (3 * bx, 3 * by, 3 * bz)), (2, (2 * bx + 3, 2 * by + 1, 2 * bz + 1))]
        assert (len(cs) == 11) == bool(r.kw.get("walk")) and len(cs) in (7, 11)
        # the full product: nothing in the enumeration depends on the width or the mode
        assert len(list(itertools.product(r.widths, r.modes, cs))) == len(r.widths) * len(r.modes) * len(cs)
    assert [r.name for r in sw.ROWS if r.kw.get("walk")] == ["conv3_split", "conv3_split_skip"]


def test_every_entry_of_the_table_takes_out():
    """the sweep hands every entry a guarded buffer: ``out`` is keyword-only and defaults to a fresh tensor"""
    from selfpose3d_amd import _lib
    for entry in sorted({r.entry for r in sw.ROWS}):
        p = inspect.signature(getattr(_lib, entry)).parameters["out"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, entry
        assert list(inspect.signature(getattr(_lib, entry)).parameters)[-1] == "out", entry


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_walk_grids_make_workgroups_walk_two_and_three_blocks(cus):
    """rounds and workgroups re-derived from conv3_split_launch: rounds = ceil(blocks / cus), nwg = ceil(blocks / rounds)"""
    bx, by, bz = sw.ROW["conv3_split"].block
    g = sw.walk_grids(cus)
    assert list(g) == ["two_rounds_whole", "two_rounds_ragged", "three_rounds_whole", "three_rounds_ragged"]
    for name, (B, (X, Y, Z)) in g.items():
        nbx, nby, nbz = -(-X // bx), -(-Y // by), -(-Z // bz)
        blocks = B * nbx * nby * nbz
        assert blocks == sw.block_count(B, (X, Y, Z), (bx, by, bz))
        rounds = (blocks + cus - 1) // cus
        nwg = (blocks + rounds - 1) // rounds
        assert (rounds, nwg) == sw.launch_of(blocks, cus) and nwg <= cus
        walk = sw.walked(blocks, nwg)
        assert sum(walk) == blocks
        assert X == bx and B * X * Y * Z <= 330_000
        if name.startswith("two_rounds"):
            assert B == 1 and rounds == 2 and blocks % 2 == 1
            assert walk.count(1) == 1 and walk.count(2) == nwg - 1 and walk[-1] == 1
        else:
            assert B == 2 and rounds == 3 and blocks % 3 != 0
            assert set(walk) == {2, 3}
            per_sample = blocks // 2
            # every workgroup's first block lies in sample 0 and its last in sample 1
            assert all(i < per_sample <= i + (n - 1) * nwg for i, n in enumerate(walk))
        if name.endswith("whole"):
            assert Y % by == 0 and Z % bz == 0
        else:
            assert Y % by != 0 and Z % bz != 0 and nby >= 5 and nbz >= 5
    assert g["two_rounds_whole"][1][1:] == tuple(a + b for a, b in zip(g["two_rounds_ragged"][1][1:], (3, 1)))
    assert g["three_rounds_whole"][1][1:] == tuple(a + b for a, b in zip(g["three_rounds_ragged"][1][1:], (3, 1)))


def test_walk_grids_for_256_compute_units():
    g = sw.walk_grids(256)
    assert g["two_rounds_whole"] == (1, (16, 296, 28)) and sw.launch_of(259, 256) == (2, 130)
    assert g["three_rounds_ragged"] == (2, (16, 157, 51)) and sw.launch_of(520, 256) == (3, 174)
    # two grids of other proportions meet the same conditions: 13 x 21 blocks, and 2 x 13 x 20
    assert sw.launch_of(sw.block_count(1, (16, 101, 83), (16, 8, 4)), 256) == (2, 137)
    assert sw.launch_of(sw.block_count(2, (16, 104, 80), (16, 8, 4)), 256) == (3, 174)


def _small(row):
    """the classes up to one block (B as the sweep runs them)"""
    if row.block is None:
        return [c for c in sw.cases(row) if c[0] in ("unit", "below_tile", "below_tile_b2", "one_tile", "one_tile_b2")]
    return [c for c in sw.cases(row) if c[0] in ("unit", "thin", "one_block")]


@pytest.mark.parametrize("name,width", ROW_WIDTHS, ids=_ids)
def test_referee_equals_naive_convolution(name, width):
    row = sw.ROW[name]
    weights = sw.make_weights(row, width)
    for cname, B, grid in _small(row):
        ins = sw.make_inputs(row, width, B, grid)
        for mode in row.modes:
            ref, naive = sw.referee(row, weights, ins, mode), sw.naive_referee(row, weights, ins, mode)
            assert ref.shape == naive.shape and ref.dtype == torch.float64
            e = sw.compare(naive, ref)["err"]
            assert max(e) <= 1e-12, (cname, mode, e)


def test_sample_zero_of_a_batch_is_the_single_sample_case():
    row = sw.ROW["conv3_split_skip"]
    two, one = sw.make_inputs(row, (32, 32), 2, (5, 4, 3)), sw.make_inputs(row, (32, 32), 1, (5, 4, 3))
    for k in ("x", "res", "xs"):
        assert torch.equal(two[k][:1], one[k]) and torch.equal(sw.first_sample(two)[k], one[k])
        assert 300.0 < float(two[k][1].abs().max() / two[k][0].abs().max()) < 3000.0


@pytest.mark.parametrize("name,width", ROW_WIDTHS, ids=_ids)
def test_compare_rejects_altered_outputs_and_referee_has_signal(name, width):
    """signal: 10-90 % positive outputs on every case of at least one block, in every ReLU mode.  Teeth, on the class with
    interior and ragged blocks (the up-conv rows: a full tile + a ragged one): the row's bound rejects one voxel of one
    channel off by 1e-3 of the range, the far-corner block zeroed, and sample 0 contaminated by 1e-6 of sample 1."""
    row = sw.ROW[name]
    weights = sw.make_weights(row, width)
    bound = sw.effective_bound(row)
    teeth_class = "tile_plus_ragged" if row.block is None else "interior_ragged"
    bitten = 0
    for cname, B, grid in sw.cases(row, cus=256):              # with the walk grids of a 256-CU device where the row walks
        ins = sw.make_inputs(row, width, B, grid)
        core = sw.referee_core(row, weights, ins)
        for mode in row.modes:
            ref = sw.epilogue(row, weights, ins, core, mode)
            cmp = sw.compare(ref.float(), ref)
            assert max(cmp["err"]) <= 1.2e-7 and max(cmp["err"]) <= bound / 10          # fp32 rounding of the exact answer passes
            assert sw.has_signal(row, mode, B, grid, cmp), (cname, mode, cmp["pos"])
            if cname != teeth_class or mode not in (1, None):
                continue
            assert B == 2
            ch = int(ref[0].abs().amax(dim=(1, 2, 3)).argmax())
            rng = float(ref[0, ch].max() - ref[0, ch].min())
            a = ref.clone()
            a[0, ch, -1, 0, -1] += 1e-3 * rng
            b = ref.clone()
            bx, by, bz = (4, 4, 4) if row.block is None else row.block
            b[:, :, -(ref.shape[2] % bx or bx):, -(ref.shape[3] % by or by):, -(ref.shape[4] % bz or bz):] = 0.0
            c = ref.clone()
            c[0] += 1e-6 * ref[1]
            for kind, alt in (("voxel", a), ("corner", b), ("neighbour", c)):
                e = sw.compare(alt, ref)["err"]
                assert max(e) > bound, (kind, e, bound)
                assert e[0] > bound, (kind, e, bound)              # each alteration shows in sample 0, the small one
            bitten += 1
    assert bitten == 1
