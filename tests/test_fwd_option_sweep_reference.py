"""The forward option sweep (tests/fwd_option_sweep_cases.py) proved without a GPU:

* plan: for every (case, option) the library's own launch plan (sp3d_unproject_fwd_plan, host arithmetic) answers the code the
  table names, launches exactly the kernels it names, with the brick stack and the second group's byte offsets it restates;
* table coverage: the kernels of the sweep's plans are every row of the planar, tile, pipe and brick tables (read from the
  SP3D_ROW tables of the sources) but the rows fs.excluded_rows() lists by name with a reason - and none of those is reached;
* class coverage: every store-path, brick, cube-count, channel and heat-map class the sweep is there for is entered by a pair
  the library accepts, asserted on the restated predicates;
* signal, from the oracle alone: something to compare in every case, unseen voxels, values clamped at 0 and at 1, skipped cubes;
* no silent skips: accepted + refused pairs = the table;
* the oracle on one-pixel maps."""
import collections

import numpy as np
import pytest

from selfpose3d_amd import _lib, build as sbuild
from tests import fwd_option_sweep_cases as fs

FAMILY = {"unproject_planar_kernel": "planar", "unproject_nhwc_kernel": "tile", "unproject_pipe_kernel": "pipe",
          "unproject_brick_kernel": "brick", "unproject_brick_h_kernel": "brick_h"}


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def plan_of(idx, o):
    c = fs.CASES[idx]
    flags = (_lib.HM_BF16 if o["in_bf16"] else 0) | (_lib.OUT_BF16 if o["out_bf16"] else 0) | (_lib.OUT_CHANNELS_LAST if o["form"] == "cl" else 0)
    layout, jp = (_lib.LAYOUT_PLANAR, 0) if o["layout"] == "planar" else (_lib.LAYOUT_NHWC, fs.jp_of(c["J"]))
    strides = fs.result_layout(o["form"], c["P"], o["Jc"], c["cube"], o["out_bf16"])["strides"][:4] if o["entry"] == "strided" else None
    word = (o["word"] | (1 << 24)) if o["entry"] == "variant" else 0
    w, h = c["wh"]
    return _lib.unproject_fwd_plan(o["entry"], layout | flags, jp, c["P"], c["V"], o["Jc"], h, w, c["cube"], word, strides)


@pytest.fixture(scope="module")
def plans(lib):
    return [(idx, o, fs.expect(idx, o), plan_of(idx, o)) for idx, o in fs.pairs()]


def test_table_limits():
    """the shapes the sweep is allowed: axes <= 24 but z of 32 / 33 / 64 on cubes of at most 6 x 6, maps <= 40 px but the 5 x 64 and
    the 96 x 72 one, 16 and 40 cubes at most 6 x 6 x 6"""
    for c in fs.CASES:
        X, Y, Z = c["cube"]
        assert max(X, Y) <= 24 and (Z <= 24 or (Z in (32, 33, 64) and max(X, Y) <= 6)), c
        assert max(c["wh"]) <= 40 or c["wh"] in ((5, 64), (96, 72)), c
        assert c["P"] < 16 or max(c["cube"]) <= 6, c
    assert sum(c["wh"] == (96, 72) for c in fs.CASES) == 1
    assert {c["P"] for c in fs.CASES} == {1, 2, 3, 4, 5, 8, 9, 16, 40}
    for cube in ((1, 1, 1), (3, 3, 3), (4, 4, 4), (5, 5, 5), (7, 6, 1), (6, 5, 20), (5, 3, 33), (6, 5, 32), (5, 6, 64)):
        assert any(c["cube"] == cube for c in fs.CASES), cube
    assert {c["J"] for c in fs.CASES} >= {17, 20, 21, 24, 25, 28, 29, 32}


def test_plan_answers_what_the_table_names(plans):
    wrong = []
    for idx, o, e, (rc, launches, _) in plans:
        where = (fs.case_id(idx), fs.option_id(o))
        if e.get("by_entry"):                        # refused by the entry point itself, before the plan is asked
            continue
        if rc != e["rc"]:
            wrong.append(where + ("code", rc, e["rc"]))
            continue
        names = [l["name"] for l in launches]
        if names != e["names"] or any(FAMILY[n.split("<")[0]] != e["family"] for n in names):
            wrong.append(where + ("kernels", names, e["names"]))
            continue
        if [l["J"] for l in launches] != [g[1] for g in e["groups"]] and e["family"] != "planar":
            wrong.append(where + ("channels written", [l["J"] for l in launches], e["groups"]))
        if e["stack"]:
            nwz, nzc, zw = e["stack"]
            for l in launches:
                if (l["s2"], l["s3"], l["block"]) != (nzc, zw, 64 * zw) or nzc * zw < nwz or (nzc - 1) * zw >= nwz:
                    wrong.append(where + ("brick stack", (l["s2"], l["s3"], l["block"]), e["stack"]))
        if len(launches) == 2:
            got = [(l["view_off"], l["out_off"], l["grids"]) for l in launches]
            if got != [(0, 0, 1), fs.group_offsets(idx, o) + (0,)]:
                wrong.append(where + ("second group", got, fs.group_offsets(idx, o)))
    assert not wrong, (len(wrong), wrong[:20])


def test_every_table_row_is_reached_or_excluded_by_name(plans):
    rows, excluded = fs.table_rows(), fs.excluded_rows()
    assert collections.Counter(rows.values()) == {"planar": 3, "tile": 24, "pipe": 51, "brick": 22}, collections.Counter(rows.values())
    reached = {l["name"] for _, _, _, (rc, launches, _) in plans for l in launches}
    assert reached <= set(rows), reached - set(rows)
    assert set(excluded) <= set(rows), set(excluded) - set(rows)
    assert not reached & set(excluded), reached & set(excluded)          # an excluded row the sweep does reach is excluded wrongly
    assert not set(rows) - reached - set(excluded), sorted(set(rows) - reached - set(excluded))
    assert fs.ZD_ROW in excluded and len(set(excluded.values())) == 3


def test_every_class_is_entered(plans):
    """by a pair the library accepts; predicates on the restated plan, not on names of cases"""
    ok = [(fs.CASES[i], o, e) for i, o, e, _ in plans if e["rc"] == fs.OK]

    def entered(what, pred):
        assert any(pred(c, o, e) for c, o, e in ok), what

    def own_bricks(c, o, e):
        return e["family"] in ("brick", "brick_h") and o["form"] == "cl"

    def planar_bricks(c, o, e):
        return e["family"] in ("brick", "brick_h") and o["form"] != "cl"
    N = lambda c: c["cube"][0] * c["cube"][1] * c["cube"][2]            # noqa: E731
    # channels-last bricks, one per workgroup
    entered("a cube inside one brick", lambda c, o, e: own_bricks(c, o, e) and max(c["cube"]) < 4)
    entered("exactly one brick", lambda c, o, e: own_bricks(c, o, e) and c["cube"] == (4, 4, 4))
    entered("ragged on all three axes", lambda c, o, e: own_bricks(c, o, e) and all(n > 4 and n % 4 for n in c["cube"]))
    entered("Z < 4 under whole bricks in x or y", lambda c, o, e: own_bricks(c, o, e) and c["cube"][2] < 4 and max(c["cube"][:2]) > 4)
    entered("X % 4 == 0, Y and Z ragged", lambda c, o, e: own_bricks(c, o, e) and c["cube"][0] % 4 == 0 and c["cube"][1] % 4 and c["cube"][2] % 4)
    entered("more than 8 bricks along z, the last ragged", lambda c, o, e: own_bricks(c, o, e) and e["stack"][0] > 8 and c["cube"][2] % 4)
    for n in (1, 2, 3, 4, 5, 8, 9, 16, 40):                             # block map at 1, 2, 4; chunk map beyond; XCD classes above 8
        entered("%d cubes, channels-last" % n, lambda c, o, e: own_bricks(c, o, e) and c["P"] == n)
        entered("%d cubes, planar" % n, lambda c, o, e: e["family"] == "pipe" and o["form"] == "dense" and c["P"] == n)
        entered("%d cubes, planar-input kernel" % n, lambda c, o, e: e["family"] == "planar" and c["P"] == n)
    # brick stacks
    for nzc in (1, 2):
        for store in ("vec16", "scalar"):
            entered("stacks, nzc %d, %s" % (nzc, store), lambda c, o, e: planar_bricks(c, o, e) and e["stack"][1] == nzc and e["store"] == store)
    entered("stacks, strided, 16-byte pieces", lambda c, o, e: planar_bricks(c, o, e) and not e["dense"] and e["store"] == "vec16")
    entered("stacks, bf16 maps", lambda c, o, e: planar_bricks(c, o, e) and e["family"] == "brick_h")
    # pipe store path
    pipe = lambda c, o, e: e["family"] == "pipe" and o["form"] != "cl"  # noqa: E731
    entered("N % 64 == 0", lambda c, o, e: pipe(c, o, e) and N(c) % 64 == 0 and e["store"] == "vec16" and not e["tail"])
    entered("N % 4 == 0, a last tile below 64", lambda c, o, e: pipe(c, o, e) and N(c) % 4 == 0 and e["store"] == "vec16" and e["tail"])
    entered("N % 4 != 0", lambda c, o, e: pipe(c, o, e) and N(c) % 4 and N(c) > 64 and e["store"] == "scalar")
    entered("N < 64", lambda c, o, e: pipe(c, o, e) and N(c) < 64)
    entered("strided, Z % 4 == 0", lambda c, o, e: pipe(c, o, e) and not e["dense"] and e["vec4"] and c["cube"][2] % 4 == 0 and e["store"] == "vec16")
    entered("strided, Z % 4 != 0, aligned rows", lambda c, o, e: pipe(c, o, e) and not e["dense"] and e["vec4"] and c["cube"][2] % 4 and
            N(c) % 4 == 0 and N(c) >= 64 and e["store"] == "scalar")
    entered("strided, unaligned rows", lambda c, o, e: pipe(c, o, e) and o["form"] == "strided_unaligned" and not e["vec4"] and N(c) % 64 == 0)
    entered("strided, aligned rows, base 4 bytes off", lambda c, o, e: pipe(c, o, e) and o["form"] == "strided_offbase" and not e["vec4"] and
            N(c) % 64 == 0 and c["cube"][2] % 4 == 0)
    entered("bf16 cubes, strided, 16-byte pieces", lambda c, o, e: pipe(c, o, e) and o["out_bf16"] and not e["dense"] and e["store"] == "vec16")
    # channels, storage, sample_of, valid
    for jp in (4, 8, 12, 16):
        for fam in ("pipe", "brick"):
            entered("Jp %d, J == Jp, %s" % (jp, fam), lambda c, o, e: e["family"] == fam and c["J"] == jp)
            entered("Jp %d, J < Jp, %s" % (jp, fam), lambda c, o, e: e["family"] == fam and jp - 4 < c["J"] < jp)
    for J in (17, 20, 21, 24, 25, 28, 29, 32):
        for storage in fs.STORAGE:
            for dense in (True, False):
                entered("J %d, storage %s, dense %s" % (J, storage, dense), lambda c, o, e: c["J"] == J and len(e["groups"]) == 2 and
                        (o["in_bf16"], o["out_bf16"]) == storage and e["dense"] == dense and any(n % 4 for n in c["cube"]))
    for width in (4, 8, 12, 16):
        for fam in ("pipe", "brick"):
            entered("second group of %d, %s" % (width, fam), lambda c, o, e: len(e["groups"]) == 2 and e["groups"][1][0] == width and e["family"] == fam)
    for storage in fs.STORAGE[1:]:
        for form in fs.FORMS:
            for mode in ("none", "perm", "repeat", "subset"):
                entered("storage %s, %s, sample_of %s" % (storage, form, mode), lambda c, o, e: (o["in_bf16"], o["out_bf16"]) == storage and
                        o["form"] == form and o["mode"] == mode)
    for how in ("first0", "mid0", "last0", "only"):
        for fam in ("planar", "pipe", "brick", "brick_h"):
            entered("valid %s, %s" % (how, fam), lambda c, o, e: c["valid"] == how and e["family"] == fam)
    # heat-maps
    entered("2 x 2", lambda c, o, e: c["wh"] == (2, 2) and e["family"] == "pipe")
    entered("1 x N", lambda c, o, e: c["wh"][0] == 1 and e["family"] == "tile")
    entered("N x 1", lambda c, o, e: c["wh"][1] == 1 and e["family"] == "tile")
    entered("5 x 64", lambda c, o, e: c["wh"] == (5, 64))
    entered("a row that is no multiple of 32 floats", lambda c, o, e: (c["wh"][0] * fs.jp_of(c["J"])) % 32 and e["family"] in ("pipe", "brick"))
    for word in (8, 24):                                                 # the channels-last rows of the pipe table
        for jp in (4, 8, 12, 16):
            entered("word %d, Jp %d" % (word, jp), lambda c, o, e: o["word"] == word and e["family"] == "pipe" and fs.jp_of(c["J"]) == jp)
    # refusals the header documents
    no = [(fs.CASES[i], o) for i, o, e, _ in plans if e["rc"] == fs.EUNSUPPORTED]
    for what, pred in (("bf16 on a one-pixel map", lambda c, o: min(c["wh"]) == 1 and (o["in_bf16"] or o["out_bf16"]) and fs.jp_of(c["J"]) == 16),
                       ("channels-last on a one-pixel map", lambda c, o: min(c["wh"]) == 1 and o["form"] == "cl" and not o["in_bf16"]),
                       ("strided on a one-pixel map", lambda c, o: min(c["wh"]) == 1 and o["entry"] == "strided"),
                       ("Jp = 32 on a one-pixel map", lambda c, o: min(c["wh"]) == 1 and c["J"] > 16 and o["form"] == "dense"),
                       ("channels-last, J % 4 != 0", lambda c, o: o["form"] == "cl" and o["Jc"] % 4 and c["J"] <= 16 and min(c["wh"]) > 1),
                       ("channels-last at Jp = 32", lambda c, o: o["form"] == "cl" and c["J"] > 16 and min(c["wh"]) > 1),
                       ("bf16 below 16 channels", lambda c, o: o["in_bf16"] and fs.jp_of(c["J"]) < 16 and min(c["wh"]) > 1),
                       ("the tile kernel has no channels-last form", lambda c, o: o["word"] in (0, 1, 2) and c["J"] <= 16)):
        assert any(pred(c, o) for c, o in no), what
    for idx in range(len(fs.CASES)):                                     # the sample_of of a case reads every class it is there for
        so = fs.get(idx).sample_of
        c = fs.CASES[idx]
        if c["P"] > c["B"]:
            assert len(set(so["repeat"])) < c["P"] and so["repeat"].max() < c["B"]
        elif c["P"] < c["B"]:
            assert len(set(so["subset"])) == c["P"] and not np.array_equal(so["subset"], np.arange(c["P"]))
        elif c["B"] > 1:
            assert sorted(so["perm"]) == list(range(c["B"])) and not np.array_equal(so["perm"], np.arange(c["B"]))


def test_no_pair_is_skipped(plans):
    """every pair either compares on the GPU or asserts its refusal: tests/test_gpu_fwd_option_sweep.py takes fs.options(idx)
    whole and branches on expect()['rc'] alone"""
    accepted = sum(e["rc"] == fs.OK for _, _, e, _ in plans)
    refused = sum(e["rc"] == fs.EUNSUPPORTED for _, _, e, _ in plans)
    assert accepted + refused == len(plans) == len(fs.pairs()) == sum(len(fs.options(i)) for i in range(len(fs.CASES)))
    assert accepted > 1000 and refused > 100, (accepted, refused)
    print("fwd option sweep: %d cases, %d pairs, %d accepted, %d refused" % (len(fs.CASES), len(plans), accepted, refused))


def test_signal_from_the_oracle_alone():
    lo = hi = unseen = skipped = False
    for idx in range(len(fs.CASES)):
        case = fs.get(idx)
        for mode in fs.modes_of(fs.CASES[idx]):
            for in_bf16 in (False, True):
                cubes, grids = case.oracle(mode, in_bf16)
                assert np.isfinite(cubes).all() and np.isfinite(grids).all()
                share = [(cubes[p] != 0).mean() for p in range(case.P) if case.valid[p]]
                assert share and max(share) >= 0.10, (fs.case_id(idx), mode, share)          # something to get wrong
                assert all(not cubes[p].any() and not grids[p].any() for p in range(case.P) if not case.valid[p])
                v = cubes[case.valid > 0]
                lo, hi = lo or bool((v == 0).any()), hi or bool((v == 1).any())              # clamped at 0 and at 1
                unseen = unseen or bool((v == 0).all(axis=1).any())                          # a voxel no view sees: zero in every channel
        skipped = skipped or not case.valid.all()
    assert lo and hi and unseen and skipped, (lo, hi, unseen, skipped)


def test_bf16_referee_is_the_parity_definition():
    """the rounded maps are bf16 values, differ from the fp32 maps, and so do the two oracle results"""
    case = fs.get(3)
    assert all(np.array_equal(fs.bf16_round(x), x) for x in case.hms_bf16)
    assert any((a != b).any() for a, b in zip(case.hms, case.hms_bf16))
    assert all((a.view(np.uint32) & 0xffff == 0).all() for a in case.hms_bf16)
    assert (case.oracle("none", False)[0] != case.oracle("none", True)[0]).any()
    o = dict(fs.options(3)[0], out_bf16=True)
    assert (case.reference(o)[0].view(np.uint32) & 0xffff == 0).all()


def test_oracle_on_one_pixel_maps():
    """1 x N and N x 1 maps: the oracle takes them, and samples the one column (row) for every voxel as the kernels' rw1 = 0
    (rh1 = 0) does - its result does not depend on where a voxel falls along that axis: the same cubes come out when the image
    is 1000 times as wide (tall), which moves every sample position along the axis and nothing else"""
    from oracle import oracle
    seen = set()
    for idx, c in enumerate(fs.CASES):
        w, h = c["wh"]
        if min(w, h) > 1:
            continue
        case = fs.get(idx)
        ref, _ = case.oracle(fs.modes_of(c)[0], False)
        assert np.isfinite(ref).all() and (ref[case.valid > 0] != 0).mean() > 0.1
        hms, cam = case.gathered(fs.modes_of(c)[0], False)
        img = (case.img[0] * 1000, case.img[1]) if w == 1 else (case.img[0], case.img[1] * 1000)
        other, _ = oracle.unproject_fwd(hms, cam, case.centers, case.valid, case.grid_size, case.cube, img)
        assert np.array_equal(ref, other), fs.case_id(idx)
        seen.add("1xN" if w == 1 else "Nx1")
    assert seen == {"1xN", "Nx1"}
