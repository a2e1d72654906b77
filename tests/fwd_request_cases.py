"""The forward-unprojection requests whose answers tests/golden/fwd_request_census.json records, and the one spelling of a
request that both sides read:

  tools/record_fwd_request_census.py  asks a library (the parent commit's) for every request and writes the table;
  tests/test_fwd_request_census.py    holds the library under test to it.

A request is (case, layout byte, flag word).  A case is a dict: entry (one of _lib.PLAN_ENTRIES), jp, J, B, V, h, w, cube, and
optionally strides (the strided entry), word (the variant entry's tuning word) and fact (a fact about the pointers that only a
real entry can be given: the plan entry has no pointers).  Every case is asked with the layout bytes 0, 1, 2 and all 512 subsets
of the nine flag bits 0x100..0x10000, flag word i being i << 8.

Two ways to ask, both without a GPU:
  ask_plan   sp3d_unproject_fwd_plan: (rc, launches, tuning); launches and tuning only when rc == 0
  ask_entry  the real extern "C" entry with dummy non-NULL pointers that are never dereferenced: the refusal code, or a
             positive HIP error where the request was accepted and reached a launch - ONLY where no GPU is visible."""
import ctypes as C

from selfpose3d_amd import _lib

LAYOUT_BYTES = (0, 1, 2)
FLAG_WORDS = 512
WORDS = (0, 24, 56, 120, 120 | 1 << 24, 56 | 1 << 22)
FACTS = ("cubes+8", "cubes+64", "grids")


def flags_of(i):
    return i << 8


def _shape(sid, jp=16, J=15, B=2, V=3, h=18, w=24, cube=(24, 16, 20)):
    return dict(id=sid, jp=jp, J=J, B=B, V=V, h=h, w=w, cube=tuple(cube))


def shapes():
    out = [_shape("jp16_J15"), _shape("jp16_J16_z32", J=16, cube=(24, 16, 32)), _shape("jp12_J12", jp=12, J=12)]
    out += [_shape(f"jp32_J{J}", jp=32, J=J) for J in (16, 21, 33)]
    out += [_shape("one_J1_V9", jp=5, J=1, V=9), _shape("one_J4", jp=5, J=4)]
    for tag, cube in (("root", (80, 80, 20)), ("root_x78", (78, 80, 20)), ("root_z24", (80, 80, 24))):
        out += [_shape(f"{tag}_jp{jp}_J{J}", jp=jp, J=J, B=1, V=5, cube=cube) for jp, J in ((16, 15), (32, 17), (16, 1))]
    for h, w in ((18, 1), (1, 24), (4097, 4096)):
        out += [_shape(f"img{h}x{w}_jp16", h=h, w=w), _shape(f"img{h}x{w}_one", jp=5, J=1, h=h, w=w)]
    out += [_shape("jp0_J1", jp=0, J=1), _shape("row_2p24", jp=1 << 22, J=1, h=2, w=4), _shape("bytes_2p31", jp=64, J=1, h=4096, w=2048)]
    out += [_shape("V17", V=17), _shape("J0", J=0)]
    return out


def _strides(s, pad=(0, 0, 0), how="dense"):
    X, Y, Z = s["cube"]
    sy = Z + pad[2]
    sx = (Y + pad[1]) * sy
    sj = (X + pad[0]) * sx
    if how == "overlap":
        sj -= 1
    if how == "wide":
        sj = (1 << 31) + 4
    return (s["J"] * sj, sj, sx, sy)


STRIDED_EXTRA = ("jp16_J15", "jp32_J21", "one_J1_V9")           # the shapes that also get the four non-dense stride sets
VARIANT_SHAPES = ("jp16_J15", "jp16_J16_z32", "jp12_J12", "jp32_J16", "jp32_J21", "jp32_J33", "root_jp16_J15", "root_jp32_J17",
                  "img18x1_jp16", "img1x24_jp16", "img4097x4096_jp16", "V17", "J0")
FACT_SHAPES = {"cubes+8": "one_J4", "cubes+64": "root_jp16_J1", "grids": "root_jp16_J1"}


def cases(facts=False):
    """every case the plan entry can be asked (facts=False), or the pointer-fact cases of the real entries (facts=True)"""
    by_id = {s["id"]: s for s in shapes()}
    out = []
    if facts:
        for entry in ("indexed", "strided", "train", "zdft", "one_train"):        # the variant entry reads no pointer fact
            for fact in FACTS:
                s = by_id[FACT_SHAPES[fact]]
                out.append(dict(s, id=f"{s['id']}@{fact}", entry=entry, fact=fact, strides=_strides(s) if entry == "strided" else None))
        return out
    for entry in _lib.PLAN_ENTRIES:
        for s in shapes():
            if entry == "variant":
                if s["id"] in VARIANT_SHAPES:
                    out += [dict(s, id=f"{s['id']}_word{word}", entry=entry, word=word) for word in WORDS]
                continue
            out.append(dict(s, entry=entry, strides=_strides(s) if entry == "strided" else None))
            if entry == "strided" and s["id"] in STRIDED_EXTRA:
                out.append(dict(s, id=s["id"] + "_pad224", entry=entry, strides=_strides(s, (2, 2, 4))))
                out.append(dict(s, id=s["id"] + "_pad111", entry=entry, strides=_strides(s, (1, 1, 1))))
                out.append(dict(s, id=s["id"] + "_overlap", entry=entry, strides=_strides(s, how="overlap")))
                out.append(dict(s, id=s["id"] + "_sj2p31", entry=entry, strides=_strides(s, how="wide")))
    assert len({(c["entry"], c["id"]) for c in out}) == len(out)
    return out


def has_layout_word(entry):
    """sp3d_unproject_fwd_zdft and sp3d_unproject_fwd_variant take no hm_layout: the real entry is one request per case"""
    return entry not in ("zdft", "variant")


class Asker:
    """a loaded library and the buffers every question reuses"""

    def __init__(self, lib):
        self.lib = lib
        nf, nt = len(_lib.PLAN_FIELDS), len(_lib.PLAN_TUNING)
        self.names = C.create_string_buffer(2 * 96)
        self.fields, self.tuning, self.n = (C.c_int32 * (2 * nf))(), (C.c_int32 * nt)(), C.c_int32(0)
        self.gs = (C.c_float * 3)(8000, 8000, 2000)
        self.views = (C.c_void_p * 17)(*[0x100000] * 17)
        self.d = C.c_void_p(0x100000)

    def ask_plan(self, c, layout, flags):
        X, Y, Z = c["cube"]
        st = (C.c_int64 * 4)(*c["strides"]) if c.get("strides") else None
        rc = self.lib.sp3d_unproject_fwd_plan(_lib.PLAN_ENTRIES.index(c["entry"]), layout | flags, c["jp"], st, c["B"], c["V"], c["J"],
                                              c["h"], c["w"], X, Y, Z, c.get("word", 0), self.names, self.fields, self.tuning,
                                              C.byref(self.n))
        if rc:
            return (rc, (), None)
        nf = len(_lib.PLAN_FIELDS)
        launches = tuple((self.names.raw[i * 96:(i + 1) * 96].split(b"\0")[0].decode(),) + tuple(self.fields[i * nf:(i + 1) * nf])
                         for i in range(self.n.value))
        return (0, launches, tuple(self.tuning))

    def ask_entry(self, c, layout, flags):
        """the real entry's code: a refusal (< 0), or > 0 = accepted, HIP found no device.  Never call this where a GPU is visible."""
        X, Y, Z = c["cube"]
        lib, d, fact = self.lib, self.d, c.get("fact")
        res = C.c_void_p(0x100000 + {"cubes+8": 8, "cubes+64": 64}.get(fact, 0))
        grids = d if fact == "grids" else None
        dims = (c["B"], c["V"], c["J"], c["h"], c["w"], X, Y, Z, self.gs, 96, 72)
        hl, e = layout | flags, c["entry"]
        if e == "indexed":
            return lib.sp3d_unproject_fwd_indexed(self.views, hl, c["jp"], d, None, d, d, res, grids, *dims, None)
        if e == "strided":
            return lib.sp3d_unproject_fwd_strided(self.views, hl, c["jp"], d, None, d, d, res, (C.c_int64 * 4)(*c["strides"]), *dims, None)
        if e == "train":
            return lib.sp3d_unproject_fwd_train(self.views, hl, c["jp"], d, None, d, d, res, grids, d, *dims, None)
        if e == "one_train":
            return lib.sp3d_unproject_one_fwd_train(self.views, hl, c["jp"], d, None, d, d, res, grids, d, *dims, None)
        if e == "zdft":
            return lib.sp3d_unproject_fwd_zdft(self.views, c["jp"], d, d, d, res, *dims, 28, None)
        return lib.sp3d_unproject_fwd_variant(self.views, c["jp"], d, d, d, res, grids, *dims, c["word"], None)
