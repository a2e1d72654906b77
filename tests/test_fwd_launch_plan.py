"""The forward unprojection's launch decision, read from the library itself without a GPU (sp3d_unproject_fwd_plan: the
resolve function every forward entry point goes through, asked with shapes instead of device pointers).

* census: kernel, workgroups, workgroup size and LDS of every request of tests/fwd_launch_cases.py equal
  tests/golden/fwd_launch_census.json, recorded from the library of the commit BEFORE the plan existed, so the table is what
  the old dispatcher did, not what this one says.  The committed table was taken on the host: the same requests issued to
  that library with dummy pointers and hipLaunchKernel interposed, writing down the kernel symbol, grid, block and dynamic
  LDS of each launch (static LDS added as below).  tools/record_fwd_launch_census.py records the same table from a
  kernel trace on a GPU, in the same format;
* the downgrades and refusals no GPU memory could hold (one-pixel-wide and 2^24 + 1 pixel images), the Jp = 32 limits and
  the one-channel refusals, as the code before the plan answered them;
* tests/test_xcd_block_map.py's numpy replay of the brick launch geometry equals the real one, field by field;
* every documented bit of the tuning word has exactly one field of the decoded tuning."""
import json
import os
import re

import pytest

from selfpose3d_amd import _lib, build as sbuild
from tests import test_xcd_block_map as replay
from tests.fwd_launch_cases import requests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NHWC, PLANAR = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def plan(entry="indexed", layout=NHWC, jp=16, B=2, V=3, J=15, h=18, w=24, cube=(24, 16, 20), word=0, flags=0, strides=None):
    return _lib.unproject_fwd_plan(entry, layout | flags, jp, B, V, J, h, w, cube, word, strides)


def plan_of(r):
    """a request of tests/fwd_launch_cases.py -> (rc, launches, tuning)"""
    flags = (_lib.HM_BF16 if r.get("in_bf16") else 0) | (_lib.OUT_BF16 if r.get("out_bf16") else 0) | \
        (_lib.OUT_CHANNELS_LAST if r.get("cl") else 0) | (_lib.HM_ONE_CHANNEL if r.get("one") else 0)
    X, Y, Z = r["cube"]
    strides = None
    if r["entry"] == "strided":
        px, py, pz = r.get("pad", (0, 0, 0))
        sy = Z + pz
        sx = (Y + py) * sy
        sj = (X + px) * sx
        strides = (r["J"] * sj, sj, sx, sy)
    word = r.get("word", 0) | ((1 << 24) if r["entry"] == "variant" and r.get("cl") else 0)
    return plan(r["entry"], NHWC if r["layout"] == "nhwc" else PLANAR, r["jp"], r["B"], r["V"], r["J"], r["h"], r["w"], r["cube"],
                word, flags, strides)


def static_lds(name):
    """LDS a kernel declares itself, which a trace adds to the launch's dynamic bytes: only the pipe kernel has any -
    NW * max(JP * WOSTR, WREC) floats (sp3d_unproject_host.h: WOSTR = 68, WREC = 640)"""
    m = re.match(r"unproject_pipe_kernel<(\d+), (?:true|false), (\d+),", name)
    return int(m.group(2)) * max(int(m.group(1)) * 68, 640) * 4 if m else 0


def test_census_equals_the_previous_dispatcher(lib):
    with open(os.path.join(ROOT, "tests", "golden", "fwd_launch_census.json")) as fh:
        census = json.load(fh)
    rq = requests()
    assert sorted(census) == sorted(r["id"] for r in rq)
    seen = set()
    for r in rq:
        rc, launches, _ = plan_of(r)
        assert rc == 0, (r["id"], rc)
        got = [dict(name=l["name"], workgroups=l["workgroups"], block=l["block"], lds=l["lds"] + static_lds(l["name"])) for l in launches]
        assert got == census[r["id"]], (r["id"], got, census[r["id"]])
        seen.update(l["name"].split("<")[0] for l in launches)
    assert seen == {"unproject_planar_kernel", "unproject_nhwc_kernel", "unproject_pipe_kernel", "unproject_brick_kernel",
                    "unproject_brick_h_kernel", "unproject_one_kernel"}


@pytest.mark.parametrize("h,w", [(18, 1), (1, 24), (4097, 4096)])
def test_images_the_pipelined_kernels_cannot_index_take_the_tile_kernel(lib, h, w):
    """below 2 x 2 pixels (the clamped 2 x 2 block) and above 2^24 pixels (24-bit multiplies): the tile kernel, whatever the
    default or the word says; bf16 storage, which only the pipelined kernels have, is refused"""
    for kw in (dict(), dict(cube=(24, 16, 32)), dict(entry="variant", word=120), dict(entry="variant", word=56 | (1 << 22))):
        rc, launches, _ = plan(h=h, w=w, **kw)
        assert rc == 0 and [l["name"] for l in launches] == ["unproject_nhwc_kernel<16, true, 1>"], (kw, rc, launches)
        tiles = -(-24 * 16 * kw.get("cube", (0, 0, 20))[2] // 256)
        assert (launches[0]["block"], launches[0]["s0"], launches[0]["s1"]) == (256, tiles, 2 * tiles)
    for entry in ("strided", "train"):      # sp3d_unproject_fwd_strided and _fwd_train refuse an image below 2 x 2; above 2^24 pixels they
        rc, launches, _ = plan(h=h, w=w, entry=entry)                                     # answer as the indexed entry does
        assert (rc, launches) == (EUNSUPPORTED, []) if min(h, w) < 2 else [l["name"] for l in launches] == ["unproject_nhwc_kernel<16, true, 1>"]
    assert plan(h=h, w=w, entry="variant", word=6)[1][0]["name"] == "unproject_nhwc_kernel<16, false, 4>"
    for flags in (_lib.HM_BF16, _lib.OUT_BF16, _lib.HM_BF16 | _lib.OUT_BF16):
        assert plan(h=h, w=w, flags=flags)[0] == EUNSUPPORTED
        assert plan(h=h, w=w, J=16, flags=flags | _lib.OUT_CHANNELS_LAST)[0] == EUNSUPPORTED
    assert plan(h=h, w=w, J=16, flags=_lib.OUT_CHANNELS_LAST)[0] == EUNSUPPORTED          # the tile kernel writes planar results
    assert plan(h=h, w=w, jp=32, J=17)[0] == EUNSUPPORTED


def test_wide_pixels_take_the_planar_defaults_only(lib):
    """Jp = 32: two channel groups through the pipe kernel or the brick stacks; no channels-last result, no pass mask, no
    z-spectrum, no word but the two planar defaults"""
    for cube, family in (((24, 16, 20), "unproject_pipe_kernel"), ((24, 16, 32), "unproject_brick_kernel")):
        rc, launches, _ = plan(jp=32, J=21, cube=cube)
        assert rc == 0 and [l["name"].split("<")[0] for l in launches] == [family] * 2
        assert [(l["J"], l["view_off"], l["out_off"], l["grids"]) for l in launches] == \
            [(16, 0, 0, 1), (5, 64, 16 * 24 * 16 * cube[2] * 4, 0)]
        assert launches[1]["name"].startswith(family + "<8, ") and launches[1]["name"].endswith(", 32>")
    assert len(plan(jp=32, J=16)[1]) == 1
    assert plan(jp=32, J=33)[0] == EUNSUPPORTED
    assert plan(jp=32, J=20, flags=_lib.OUT_CHANNELS_LAST)[0] == EUNSUPPORTED
    assert plan("train", jp=32, J=17)[0] == EUNSUPPORTED
    assert plan("zdft", jp=32, J=17, B=1, cube=(80, 80, 20))[0] == EUNSUPPORTED
    for word in (24, 56):                                        # either default, whatever the grid's own default is
        for cube in ((24, 16, 20), (24, 16, 32)):
            assert plan("variant", jp=32, J=17, cube=cube, word=word)[0] == 0
    for word in (0, 8, 28, 120, 56 | 64, 56 | 256, 56 | (1 << 10), 56 | (1 << 11), 24 | (1 << 17), 24 | (1 << 21), 56 | (1 << 22), 24 | (1 << 24)):
        assert plan("variant", jp=32, J=20 if word >> 24 else 17, word=word)[0] == EUNSUPPORTED, word


def test_one_channel_refusals(lib):
    """SP3D_HM_ONE_CHANNEL: every refusal of the one-channel read, in the order the entry points gave them"""
    one = _lib.HM_ONE_CHANNEL
    ok = dict(jp=5, J=1, flags=one)
    for layout in (PLANAR, NHWC):
        assert plan(layout=layout, **ok)[0] == 0
        assert plan(layout=layout, jp=5, J=4, flags=one | _lib.OUT_CHANNELS_LAST)[0] == 0
        assert plan("strided", layout=layout, **ok)[0] == 0
        assert plan(layout=layout, jp=0, J=1, flags=one)[0] == EINVAL                   # no channel to read
        for J in (2, 3, 5, 16):                                                         # 1 or 4 channels written
            assert plan(layout=layout, jp=5, J=J, flags=one)[0] == EUNSUPPORTED
        assert plan(layout=layout, jp=5, J=1, flags=one | _lib.OUT_CHANNELS_LAST)[0] == EUNSUPPORTED   # channels-last: 4
        for bf in (_lib.HM_BF16, _lib.OUT_BF16):                                        # fp32 storage only
            assert plan(layout=layout, jp=5, J=1, flags=one | bf)[0] == EUNSUPPORTED
        assert plan("train", layout=layout, **ok)[0] == EUNSUPPORTED                    # no pass mask
        for h, w in ((18, 1), (1, 24), (4097, 4096)):                                   # 2 x 2 .. 2^24 pixels
            assert plan(layout=layout, h=h, w=w, **ok)[0] == EUNSUPPORTED
    for layout in (2, 7):                                                               # unknown layout: before everything else
        assert plan(layout=layout, jp=5, J=2, flags=one | _lib.HM_BF16)[0] == EINVAL
    # a pixel row of 2^24 elements or more, a sample beyond 32-bit byte offsets (NHWC: the pixel stride counts)
    assert plan(layout=NHWC, jp=1 << 22, J=1, h=2, w=4, flags=one)[0] == EUNSUPPORTED
    assert plan(layout=NHWC, jp=(1 << 22) - 1, J=1, h=2, w=4, flags=one)[0] == 0
    assert plan(layout=NHWC, jp=64, J=1, h=4096, w=2048, flags=one)[0] == EUNSUPPORTED
    assert plan(layout=PLANAR, jp=64, J=1, h=4096, w=2048, flags=one)[0] == 0
    rc, (l,), _ = plan(layout=NHWC, jp=5, J=1, V=9, flags=one)
    assert rc == 0 and l["name"] == "unproject_one_kernel<10, 8, false>" and (l["nscalars"], l["s0"], l["s1"], l["s2"]) == (3, 18 * 24 * 5, 24 * 5, 5)


def _geom_of(launch, keys):
    return {k: launch[k] for k in keys}


@pytest.mark.parametrize("B", [1, 2, 3, 4, 8])
def test_numpy_replay_of_the_brick_launch_is_the_real_one(lib, B):
    """launch_geom of tests/test_xcd_block_map.py against the plan: every grid of 1..40 x 1..40 brick columns and 1..3
    z-chunks, block map (the default of channels-last results) and chunk map (tuning bit 22)"""
    for nzc in (1, 2, 3):
        Z = 32 * nzc - 12                                        # nwz = 8 nzc - 3 bricks: nzc chunks of 8, 8, 5
        for nbx in range(1, 41):
            for nby in range(1, 41):
                for chunks in (False, True):
                    want, grid = replay.launch_geom(B, nbx, nby, nzc, chunks)
                    rc, (l,), _ = plan("variant", jp=4, J=4, B=B, cube=(4 * nbx, 4 * nby, Z), word=56 | ((1 << 22) if chunks else 0))
                    where = (B, nbx, nby, nzc, chunks)
                    assert rc == 0 and l["workgroups"] == grid, (where, l["workgroups"], grid)
                    assert (l["s0"], l["s1"], l["s2"]) == (nbx * nby * nzc, nby, nzc), where
                    want.pop("B")
                    assert _geom_of(l, want) == want, (where, _geom_of(l, want), want)


def test_every_documented_bit_has_its_field(lib):
    """sp3d_tuning.h lists the bits; a word with one of them set differs from word 0 in exactly that field"""
    with open(os.path.join(ROOT, "selfpose3d_amd", "csrc", "sp3d_tuning.h")) as fh:
        text = fh.read()
    documented = []
    for hi, lo, bit in re.findall(r"^ \*   bits? (?:(\d+):(\d+)|(\d+)) ", text, re.M):
        documented += list(range(int(lo), int(hi) + 1)) if hi else [int(bit)]
    bits = {0: "unroll", 1: "unroll", 2: "no_xcd_map", 3: "pipe", 4: "one_wave", 5: "brick", 6: "brick_own_wg", 8: "z_fastest",
            10: "view_sync", 11: "ballast", 12: "ballast", 13: "ballast", 17: "forced_chunk", 18: "forced_chunk", 19: "forced_chunk",
            20: "forced_chunk", 21: "plain_sweep", 22: "chunk_map"}
    assert sorted(documented) == sorted(list(bits) + [24])      # bit 24 is the result layout, not a tuning
    base = plan("variant", word=0)[2]
    assert set(base) == set(bits.values()) and len(base) == len(_lib.PLAN_TUNING)
    values = set()
    for bit, field in bits.items():
        t = plan("variant", word=1 << bit)[2]
        assert [k for k in t if t[k] != base[k]] == [field], (bit, t)
        values.add((field, t[field]))
    assert len(values) == len(bits)                              # each bit of a multi-bit field moves it to its own value
    for bit in (7, 9, 14, 15, 16, 23):                           # no field: ignored
        assert plan("variant", word=1 << bit)[2] == base
    cl = plan("variant", J=16, word=120 | (1 << 24))
    assert cl[2] == plan("variant", word=120)[2] and cl[1][0]["name"] == "unproject_brick_kernel<16, true, float, float, false, 16>"
    for word, default in ((24, dict()), (56, dict(cube=(24, 16, 32))), (120, dict(J=16, flags=_lib.OUT_CHANNELS_LAST))):
        assert plan(**default)[2] == plan("variant", word=word)[2]          # the three library defaults, as the header names them
