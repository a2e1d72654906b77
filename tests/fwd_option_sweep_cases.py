"""Cases, options, expectations and CPU referee of the forward-unprojection option sweep (tests/test_fwd_option_sweep_reference.py
proves this table on the CPU, tests/test_gpu_fwd_option_sweep.py runs every pair of it on the GPU, bit for bit against the
oracle).  Plain helper module: no pytest hooks, no GPU, every input generated from fixed seeds.

A case is (P, B, V, J, (w, h), cube, grid kind) plus the pattern of its ``valid`` bytes: P cubes over B samples, V views, J
joints, a w x h heat-map of a 4w x 4h image; inputs as tests/test_gpu_random_sweep.py draws them (syn.random_meta with augment
/ ssv_style alternating, random flips, heat-maps in [-0.3, 1.3], space / fine / pitch grids as tests/bwd_sweep_cases.py).  The
packed pixel has Jp = 4 ceil(J / 4) channels, 32 for J > 16.

An option is one request to the library on a case's inputs:
  entry    indexed | strided | variant (the tuning-word entry, with the channels-last bit) and, for the planar-input kernel,
           indexed with LAYOUT_PLANAR;
  form     of the result: dense planar, channels-last ("cl": Jc = Jp channels, the pad channels are zeros), and three strided
           ones inside a larger buffer - rows of 4-element multiples ("strided_aligned"), rows that are not
           ("strided_unaligned"), and aligned rows behind a base pointer 4 bytes off a 16-byte boundary ("strided_offbase");
  storage  bf16 heat-maps and / or bf16 cubes;
  mode     of sample_of: "none" and "perm" (a permutation) when P == B, "repeat" when P > B, "subset" when P < B;
  grids    whether the grids are asked for (the strided entry has none).
With bf16 at Jp < 16 (no such kernels) a form is asked once, not once per mode and grids: those pairs are refused before
anything is launched.

expect() restates resolve_fwd / resolve_group / set_result_strides of selfpose3d_amd/csrc/sp3d_unproject.hip and the store
predicates of the kernels in Python and NAMES, per pair, the return code, the kernel family, the kernels, the store path and
the brick stack (nwz, nzc, zw); whether a kernel exists is read from the SP3D_ROW tables of the sources (table_rows()).

Referee: oracle.unproject_fwd on the gathered batch (hms[c][sample_of], cam[sample_of]); for bf16 heat-maps on the bf16-rounded
maps; for bf16 cubes its fp32 result rounded to bf16 (RNE): the parity definition of tests/test_gpu_parity.py::
test_bf16_storage_config.  No tolerance anywhere.

One-pixel maps (1 x N, N x 1): the oracle divides by (w - 1) as the reference does: +-inf, clamped to +-1.1, times
(w - 1) / 2 = 0 gives +-0, the kernels' rw1 = 0 (make_geom) gives 0 the same way, so both sample column 0 for every voxel
(tests/test_fwd_option_sweep_reference.py::test_oracle_on_one_pixel_maps); the oracle takes such maps.
"""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "selfpose3d_amd", "csrc")
OK, EUNSUPPORTED = 0, -4
GUARD = 4096
FORMS = ("dense", "cl", "strided_aligned", "strided_unaligned", "strided_offbase")
STORAGE = ((False, False), (True, False), (False, True), (True, True))          # (bf16 heat-maps, bf16 cubes)
CL_WORDS = (0, 1, 2, 8, 24)      # tuning words of the variant entry run with the channels-last bit


def _c(P, B, V, J, wh, cube, kind, valid="random", seed=0):
    return dict(P=P, B=B, V=V, J=J, wh=wh, cube=cube, kind=kind, valid=valid, seed=seed)


CASES = [
    # bricks and pipe tiles: every way a 4x4x4 brick, a 64-voxel tile and a 16-byte piece can be cut
    _c(1, 1, 1, 1, (2, 2), (1, 1, 1), "fine", "all", seed=1),             # one voxel on a 2x2 map (seed 0: the view misses it)
    _c(2, 2, 3, 16, (9, 7), (3, 3, 3), "space", "all"),                   # N = 27 < 64; 9 x 16 floats a row: not a multiple of 32
    _c(3, 3, 2, 4, (12, 10), (4, 4, 4), "fine", "first0"),                # one whole brick, N = 64
    _c(2, 2, 3, 15, (16, 12), (5, 5, 5), "space", "last0"),               # N = 125: N % 4 != 0
    _c(4, 4, 2, 8, (24, 18), (7, 6, 1), "fine", "mid0"),                  # Z = 1
    _c(5, 5, 3, 12, (20, 15), (6, 5, 20), ("pitch", 40.0), "random"),     # N = 600: N % 4 == 0, a last tile of 24; Z % 4 == 0
    _c(2, 2, 7, 4, (5, 64), (5, 3, 33), "fine", "all"),                   # 9 bricks along z; 5 pixels wide
    _c(8, 8, 3, 7, (33, 17), (8, 5, 6), "space", "random"),               # X % 4 == 0, Y and Z ragged; Z % 4 != 0, N % 4 == 0
    _c(3, 3, 2, 13, (31, 22), (6, 5, 32), ("pitch", 45.0), "first0"),     # brick stacks, nzc = 1
    _c(2, 2, 2, 16, (20, 16), (5, 6, 64), "fine", "all"),                 # brick stacks, nzc = 2
    _c(1, 1, 4, 10, (40, 30), (9, 10, 11), "fine", "all"),                # Jp = 12 above J
    _c(2, 2, 5, 15, (96, 72), (17, 13, 9), "space", "all"),               # the one large map
    _c(4, 4, 3, 16, (24, 18), (16, 4, 4), "space", "last0"),              # N = 256: whole tiles only
    _c(2, 2, 2, 14, (11, 9), (4, 12, 8), ("pitch", 50.0), "all"),         # whole bricks, N = 384 = 6 tiles, Z % 4 == 0
    # cube counts and sample_of
    _c(9, 9, 2, 5, (17, 13), (6, 6, 6), "fine", "mid0"),
    _c(16, 16, 2, 16, (14, 11), (6, 6, 6), "space", "only"),              # every cube but one skipped
    _c(40, 3, 2, 15, (18, 14), (5, 6, 4), "fine", "random"),              # P = 40 over B = 3
    _c(5, 2, 3, 9, (22, 16), (10, 7, 12), ("pitch", 32.0), "first0"),     # P = 5 over B = 2
    _c(2, 5, 3, 16, (15, 12), (7, 9, 8), "fine", "all"),                  # P = 2 of B = 5
    _c(3, 7, 2, 3, (8, 6), (5, 4, 3), "fine", "last0"),                   # P = 3 of B = 7
    # one-pixel maps: the tile kernel, or a refusal
    _c(2, 2, 3, 6, (1, 24), (6, 5, 7), "fine", "all"),
    _c(3, 3, 2, 16, (19, 1), (5, 4, 9), "space", "mid0"),
    _c(1, 1, 2, 17, (1, 9), (4, 4, 4), "fine", "all"),                    # Jp = 32 on a one-pixel map: refused
    _c(1, 1, 2, 2, (1, 5), (3, 4, 5), "fine", "all"),
    _c(2, 2, 2, 11, (7, 1), (4, 3, 6), "fine", "first0"),
    # brick stacks below 16 channels
    _c(2, 2, 2, 3, (10, 8), (6, 5, 32), "fine", "all"),
    _c(1, 1, 3, 8, (12, 9), (6, 5, 32), ("pitch", 35.0), "all"),
    _c(3, 2, 2, 11, (9, 12), (6, 5, 32), "fine", "mid0"),
    # Jp = 32: group 1 of width 4, 8, 12, 16, each through the pipe kernel and through the brick stacks
    _c(2, 2, 3, 17, (16, 12), (7, 5, 6), "space", "first0"),
    _c(3, 3, 2, 20, (33, 17), (6, 5, 32), "fine", "mid0"),
    _c(2, 2, 2, 21, (13, 9), (9, 3, 10), "fine", "all"),
    _c(1, 1, 3, 24, (21, 16), (5, 6, 64), ("pitch", 30.0), "all"),
    _c(4, 2, 2, 25, (12, 12), (6, 5, 32), "fine", "last0"),
    _c(2, 2, 2, 28, (18, 10), (5, 8, 12), "space", "all"),                # N = 480: N % 4 == 0, a last tile of 32
    _c(2, 2, 2, 29, (10, 14), (4, 7, 9), "space", "all"),
    _c(2, 3, 2, 32, (16, 10), (6, 5, 32), "fine", "all"),
]


def jp_of(J):
    return 32 if J > 16 else 4 * ((J + 3) // 4)


def case_id(idx):
    c = CASES[idx]
    k = c["kind"] if isinstance(c["kind"], str) else "pitch%g" % c["kind"][1]
    return "%02d-P%dB%dV%dJ%d-%dx%d-%dx%dx%d-%s-%s" % ((idx, c["P"], c["B"], c["V"], c["J"]) + c["wh"] + c["cube"] + (k, c["valid"]))


def modes_of(case):
    return ("none", "perm") if case["P"] == case["B"] else (("repeat",) if case["P"] > case["B"] else ("subset",))


# ---- options ---------------------------------------------------------------------------------------------------------------------
def _o(entry, form, mode, grids, in_bf16=False, out_bf16=False, layout="nhwc", word=None, Jc=None):
    return dict(entry=entry, form=form, mode=mode, grids=grids, in_bf16=in_bf16, out_bf16=out_bf16, layout=layout, word=word, Jc=Jc)


@functools.lru_cache(maxsize=None)
def options(idx):
    """every request made on case ``idx``; ``Jc`` = channels asked for (J, or Jp with a channels-last result)"""
    case = CASES[idx]
    J, jp, modes = case["J"], jp_of(case["J"]), modes_of(case)
    out = []
    for form in FORMS:
        Jc = jp if (form == "cl" and jp <= 16) else J
        for in_bf16, out_bf16 in STORAGE:
            for mi, mode in enumerate(modes):
                for grids in ((True, False) if form in ("dense", "cl") else (False,)):
                    if (in_bf16 or out_bf16) and jp < 16 and (mi or grids):
                        continue
                    out.append(_o("strided" if form.startswith("strided") else "indexed", form, mode, grids, in_bf16, out_bf16, Jc=Jc))
    if J % 4 and jp <= 16:
        out.append(_o("indexed", "cl", modes[0], False, Jc=J))           # channels-last rows that are no 16-byte multiples
    for mode in modes:                                                   # the planar-input kernel
        out.append(_o("indexed", "dense", mode, True, layout="planar", Jc=J))
    if "none" in modes:                                                  # the entry has no sample_of
        for word in CL_WORDS:
            out.append(_o("variant", "cl", "none", True, word=word, Jc=jp if jp <= 16 else J))
    return tuple(out)


def option_id(o):
    s = "%s/%s/%s%s" % (o["entry"] if o["layout"] == "nhwc" else "planar-input", o["form"], o["mode"], "/grids" if o["grids"] else "")
    s += "/in16" * o["in_bf16"] + "/out16" * o["out_bf16"] + ("/J%d" % o["Jc"])
    return s + ("/word%d" % o["word"] if o["word"] is not None else "")


def pairs():
    return [(i, o) for i in range(len(CASES)) for o in options(i)]


# ---- the result buffer of a form -------------------------------------------------------------------------------------------------
def result_layout(form, P, Jc, cube, out_bf16):
    """where the (P, Jc, X, Y, Z) result lies in a flat buffer of ``total`` elements: ``offset`` of its first element and its
    element strides (sB, sJ, sX, sY, 1).  Dense and channels-last results are slabs between GUARD elements; a strided result
    is the corner of a (P, Jc + 1, X + 1, Y + 1, Z + pz) block between GUARD elements: the padding is the guard."""
    X, Y, Z = cube
    N = X * Y * Z
    if form == "dense":
        return dict(offset=GUARD, strides=(Jc * N, N, Y * Z, Z, 1), total=P * Jc * N + 2 * GUARD)
    if form == "cl":
        return dict(offset=GUARD, strides=(Jc * N, 1, Y * Z * Jc, Z * Jc, Jc), total=P * Jc * N + 2 * GUARD)
    pz = 4 - Z % 4 + (1 if form == "strided_unaligned" else 0)           # rows of 4-element multiples, or one more
    sY = Z + pz
    sX = (Y + 1) * sY
    sJ = (X + 1) * sX
    sB = (Jc + 1) * sJ
    offset = GUARD + ((4 // (2 if out_bf16 else 4)) if form == "strided_offbase" else 0)     # 4 bytes past a 16-byte boundary
    return dict(offset=offset, strides=(sB, sJ, sX, sY, 1), total=offset + P * sB + GUARD)


# ---- the plan's rule, restated ---------------------------------------------------------------------------------------------------
def decode_word(word):
    """sp3d_tuning.h: the fields of the tuning word that choose a kernel"""
    return dict(unroll=1 if (word & 3) == 0 else (4 if (word & 3) == 2 else 2), xcd=not (word >> 2) & 1, pipe=bool((word >> 3) & 1),
                one_wave=bool((word >> 4) & 1), brick=bool((word >> 5) & 1), own_wg=bool((word >> 6) & 1))


def brick_stack(Z, own_wg):
    """bricks along z, workgroups along z, bricks per workgroup (resolve_group)"""
    nwz = (Z + 3) // 4
    nzc = (nwz + 7) // 8
    zw = (nwz + nzc - 1) // nzc
    return (nwz, nwz, 1) if own_wg else (nwz, nzc, zw)


def _b(v):
    return "true" if v else "false"


def _t(bf16):
    return "bf16_t" if bf16 else "float"


def kernel_name(family, jp, ps, t, cl, in_bf16, out_bf16):
    if family == "planar":
        return "unproject_planar_kernel<%d>" % jp
    if family == "tile":
        return "unproject_nhwc_kernel<%d, %s, %d>" % (jp, _b(t["xcd"]), t["unroll"]) if not (cl or in_bf16 or out_bf16 or ps != jp) else None
    if family == "pipe":
        return "unproject_pipe_kernel<%d, %s, %d, %s, %s, %s, %d>" % (jp, _b(t["xcd"]), 1 if t["one_wave"] else 4, _b(cl), _t(in_bf16),
                                                                      _t(out_bf16), ps)
    if family == "brick":
        return "unproject_brick_kernel<%d, %s, %s, %s, false, %d>" % (jp, _b(cl), _t(in_bf16), _t(out_bf16), ps)
    return "unproject_brick_h_kernel<%s, %s, %d>" % (_b(cl), _t(out_bf16), ps) if jp == 16 else None      # two lanes per bf16 pixel: 16 channels


def expect(idx, o):
    """what the library must answer to option ``o`` of case ``idx``: dict(rc, family, names, store, stack, groups, vec4, dense,
    tail).  ``store`` is the path of the whole tiles / bricks: "vec16" (16-byte pieces; for bf16 cubes the same four elements in
    8 bytes) or "scalar"; ``tail``: the pipe / tile kernel's last tile is ragged and leaves through the scalar path whatever
    ``store`` says; ``groups``: [(channels gathered, channels written)] per launch."""
    case = CASES[idx]
    P, J, (w, h), (X, Y, Z) = case["P"], o["Jc"], case["wh"], case["cube"]
    N, jp = X * Y * Z, jp_of(case["J"])
    cl, io = o["form"] == "cl", o["in_bf16"] or o["out_bf16"]
    refused = dict(rc=EUNSUPPORTED, family=None, names=[], store=None, stack=None, groups=[], tail=False)
    lay = result_layout(o["form"], P, J, case["cube"], o["out_bf16"])
    dense = o["form"] in ("dense", "cl")
    # set_result_strides: 16-byte pieces need rows of 4-element multiples and a 16-byte aligned base
    vec4 = dense or (all(s % 4 == 0 for s in lay["strides"][:4]) and (lay["offset"] * (2 if o["out_bf16"] else 4)) % 16 == 0)
    refused.update(vec4=vec4, dense=dense)
    if o["layout"] == "planar":                        # resolve_fwd: fp32, planar result, any J
        jc = 1 if J == 1 else (4 if J <= 4 else 16)
        return dict(rc=OK, family="planar", names=[kernel_name("planar", jc, jc, None, False, False, False)], store="scalar", stack=None,
                    groups=[(jc, J)], vec4=True, dense=True, tail=False)
    tile_only = w < 2 or h < 2                         # (and above 2^24 pixels, which no buffer here holds)
    if o["entry"] == "strided" and tile_only:          # sp3d_unproject_fwd_strided itself, before the plan: the tile kernel
        return dict(refused, by_entry=True)            # writes dense results only
    if o["entry"] == "variant":
        t = decode_word(o["word"])
    else:                                              # default_tuning: bricks of their own, brick stacks, 64-voxel tiles
        t = dict(unroll=1, xcd=True, pipe=True, one_wave=True, brick=cl or Z % 32 == 0, own_wg=cl)
    asked = dict(t)
    if tile_only:
        t["pipe"] = t["brick"] = False
    if t["brick"]:
        t["pipe"] = True
    if io:
        t["one_wave"] = True
    if jp == 32:
        defaults = [dict(unroll=1, xcd=True, pipe=True, one_wave=True, brick=b, own_wg=False) for b in (False, True)]
        if J > 32 or cl or tile_only or asked not in defaults:
            return refused
        groups = [(16, min(J, 16))] + ([(16 if io else 4 * ((J - 16 + 3) // 4), J - 16)] if J > 16 else [])
    else:
        if jp < J or cl and J % 4 or io and not t["pipe"]:
            return refused
        groups = [(jp, J)]
    family = ("brick_h" if o["in_bf16"] else "brick") if t["brick"] else ("pipe" if t["pipe"] else "tile")
    names = [kernel_name(family, g, jp, t, cl, o["in_bf16"], o["out_bf16"]) for g, _ in groups]
    if any(n not in table_rows() for n in names):       # a missing row is SP3D_EUNSUPPORTED
        return refused
    stack = brick_stack(Z, t["own_wg"]) if t["brick"] else None
    tile = dict(tile=256, pipe=64).get(family)
    if cl:
        store = "vec16"                                # a voxel's channel quads leave as 16-byte pieces from the gather mapping
    elif family == "tile":
        store = "vec16" if N % 4 == 0 and N >= tile else "scalar"
    elif family == "pipe":                             # 4 consecutive voxels lie in one z-column: dense any 4, strided Z % 4 == 0
        store = "vec16" if vec4 and N % 4 == 0 and N >= tile and (dense or Z % 4 == 0) else "scalar"
    else:
        store = "vec16" if vec4 and Z % 4 == 0 else "scalar"
    return dict(rc=OK, family=family, names=names, store=store, stack=stack, groups=groups, vec4=vec4, dense=dense,
                tail=tile is not None and N % tile != 0)


def group_offsets(idx, o):
    """byte offsets of the second channel group of Jp = 32: 16 channels into the packed pixel, 16 channel planes into the result"""
    lay = result_layout(o["form"], CASES[idx]["P"], o["Jc"], CASES[idx]["cube"], o["out_bf16"])
    return 16 * (2 if o["in_bf16"] else 4), 16 * lay["strides"][1] * (2 if o["out_bf16"] else 4)


# ---- the kernel tables, read from the sources ---------------------------------------------------------------------------------
def _split_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
            continue
        depth += ch in "({"
        depth -= ch in ")}"
        cur += ch
    return out + [cur.strip()]


def _expand(text, macros):
    """expand the function-like macros of ``macros`` in ``text`` until only SP3D_ROW(...) invocations are left"""
    pat = re.compile(r"\b(%s)\s*\(" % "|".join(sorted(macros, key=len, reverse=True)))
    while True:
        m = pat.search(text)
        if not m:
            return text
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        params, body = macros[m.group(1)]
        args = _split_args(text[m.end():i - 1])
        assert len(args) == len(params), (m.group(1), args)
        for p, a in zip(params, args):
            body = re.sub(r"\b%s\b" % p, a, body)
        text = text[:m.start()] + body + text[i:]


@functools.lru_cache(maxsize=None)
def table_rows():
    """{kernel name: table} of every row of find_planar_kernel, find_tile_kernel, find_pipe_kernel and find_brick_kernel, as
    SP3D_ROW prints it (the kernel and its template arguments, blanks normalised)"""
    rows = {}
    for fname, tables in (("sp3d_unproject_tile.hip", ("planar", "tile")), ("sp3d_unproject_pipe.hip", ("pipe",)),
                          ("sp3d_unproject_brick.hip", ("brick",))):
        with open(os.path.join(CSRC, fname)) as fh:
            src = fh.read().replace("\\\n", " ")
        macros = {m.group(1): ([p.strip() for p in m.group(2).split(",")], m.group(3))
                  for m in re.finditer(r"^#define (SP3D_\w+)\(([^)]*)\)\s+(.*)$", src, re.M) if m.group(1) != "SP3D_ROW"}
        for table in tables:
            body = re.search(r"^int find_%s_kernel\([^)]*\)\s*\{(.*?)^\}" % table, src, re.M | re.S).group(1)
            body = _expand(re.sub(r"//[^\n]*", "", body), macros)
            found = re.findall(r"SP3D_ROW\(\w+,\s*\(KernelKey\{[^}]*\}\),\s*(\w+),\s*([^)]*)\)", body)
            assert found and body.count("SP3D_ROW") == len(found), (table, body)
            for kernel, args in found:
                name = "%s<%s>" % (kernel, ", ".join(a.strip() for a in args.split(",")))
                assert name not in rows, name
                rows[name] = table
    return rows


ZD_ROW = "unproject_brick_kernel<16, false, float, float, true, 16>"
WORD_ONLY = "only a tuning word reaches it (tile kernel: plain block order, unroll 2 or 4; pipe kernel: plain block order, four waves a " \
            "workgroup with a planar result): tests/test_gpu_parity.py and tests/test_gpu_random_sweep.py run those words"
NO_ENTRY = "no entry point can ask for it: bf16 storage comes with the layout word, which the tuning-word entry does not take, and " \
           "every other entry gives bf16 the XCD map and sends channels-last results to the bricks"


@functools.lru_cache(maxsize=None)
def excluded_rows():
    """{row: reason} of the rows this sweep does not reach; the CPU test fails if one of them IS reached or exists no more"""
    out = {ZD_ROW: "the z-spectrum form: tests/test_gpu_fused_zdft.py"}
    for name, table in table_rows().items():
        a = [s.strip() for s in name[name.index("<") + 1:-1].split(",")]
        if table == "tile" and (a[1] == "false" or a[2] != "1"):
            out[name] = WORD_ONLY
        if table == "pipe":
            jp, xcd, nw, cl, ti, to, ps = a
            if "bf16_t" in (ti, to) and (xcd == "false" or cl == "true"):
                out[name] = NO_ENTRY
            elif xcd == "false" or (nw == "4" and cl == "false"):
                out[name] = WORD_ONLY
    return out


# ---- inputs and referee ----------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """fp32 -> bf16 (round to nearest even) -> fp32, as torch rounds"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


class Case:
    """inputs of one case (numpy, host) and, lazily, its CPU references"""

    def __init__(self, idx):
        import torch
        from selfpose3d_amd import synthetic as syn
        from selfpose3d_amd.camera_pack import pack_cameras
        c = CASES[idx]
        self.idx = idx
        self.P, self.B, self.V, self.J, (self.w, self.h), self.cube, self.kind = c["P"], c["B"], c["V"], c["J"], c["wh"], c["cube"], c["kind"]
        P, B, V, J, w, h = self.P, self.B, self.V, self.J, self.w, self.h
        self.jp = jp_of(J)
        self.N = self.cube[0] * self.cube[1] * self.cube[2]
        rng = np.random.default_rng(7000 + idx + 100 * c["seed"])
        self.img = img = (w * 4, h * 4)
        meta = syn.random_meta(B, V, img, seed=300 + idx + 100 * c["seed"], augment=(idx % 2 == 0), ssv_style=(idx % 3 == 0))
        flip = torch.from_numpy(rng.random(B) < 0.4) if idx % 2 == 0 else None
        self.cam = pack_cameras(meta, B, img, flip).reshape(B, V, 64)
        self.hms = [(rng.random((B, J, h, w), dtype=np.float32) * 1.6 - 0.3) for _ in range(V)]
        self.hms_bf16 = [bf16_round(x) for x in self.hms]
        if self.kind == "space":
            self.centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), P, 0)
            self.grid_size = [float(s) for s in syn.SPACE_SIZE]
        else:
            self.centers = np.stack([rng.uniform(-1500, 1500, P), rng.uniform(-2000, 1000, P), rng.uniform(200, 1500, P)], 1).astype(np.float32)
            self.grid_size = [float(rng.uniform(500, 3000))] * 3 if self.kind == "fine" else [self.kind[1] * max(n - 1, 1) for n in self.cube]
        valid = (rng.random(P) < 0.8).astype(np.uint8)
        how = c["valid"]
        if how == "all":
            valid[:] = 1
        elif how == "only":
            valid[:] = 0
            valid[P // 3] = 1
        elif how == "first0":
            valid[0], valid[-1] = 0, 1
        elif how == "mid0":
            valid[0], valid[P // 2] = 1, 0
        elif how == "last0":
            valid[0], valid[-1] = 1, 0
        elif not valid.any():
            valid[P // 2] = 1
        self.valid = valid
        perm = rng.permutation(B)
        if B > 1 and np.array_equal(perm, np.arange(B)):
            perm = np.roll(perm, 1)
        self.sample_of = {"none": None, "perm": perm.astype(np.int32)} if P == B else \
            ({"repeat": rng.integers(0, B, P).astype(np.int32)} if P > B else {"subset": rng.choice(B, P, replace=False).astype(np.int32)})

    def gathered(self, mode, in_bf16):
        so = self.sample_of[mode]
        so = np.arange(self.P) if so is None else so
        return [x[so] for x in (self.hms_bf16 if in_bf16 else self.hms)], self.cam[so]

    @functools.lru_cache(maxsize=None)
    def oracle(self, mode, in_bf16):
        """((P, J, X, Y, Z) cubes, (P, N, 3) grids), fp32"""
        from oracle import oracle
        hms, cam = self.gathered(mode, in_bf16)
        return oracle.unproject_fwd(hms, cam, self.centers, self.valid, self.grid_size, self.cube, self.img)

    def reference(self, o):
        """-> (cubes (P, Jc, X, Y, Z) fp32 - bf16 cubes: the values of the rounded result -, grids (P, N, 3))"""
        cubes, grids = self.oracle(o["mode"], o["in_bf16"])
        if o["Jc"] > self.J:
            cubes = np.concatenate([cubes, np.zeros((self.P, o["Jc"] - self.J) + tuple(self.cube), np.float32)], 1)
        return (bf16_round(cubes) if o["out_bf16"] else cubes), grids


@functools.lru_cache(maxsize=None)
def get(idx):
    return Case(idx)
