"""The forward-unprojection requests whose launches tests/golden/fwd_launch_census.json records (kernel name, workgroups,
workgroup size, dynamic LDS per dispatch), and the one spelling of a request that both sides read:

  tools/record_fwd_launch_census.py  runs every request on a GPU under a kernel trace and writes the table;
  tests/test_fwd_launch_plan.py      asks the library's launch plan (sp3d_unproject_fwd_plan, no GPU) for the same requests.

A request is a dict: entry (indexed | strided | train | zdft | variant), layout (nhwc | planar), jp, J, B, V, h, w, cube and
the optional flags in_bf16, out_bf16, cl (channels-last result), pad (strided result inside a larger buffer), one (one-channel
read), word (tuning word of the variant entry).  Heat-maps are 24 x 18: the grids are what the census is about."""

H, W = 18, 24

PARITY_WORDS = [0, 1, 2, 4, 5, 6, 8, 12, 24, 28, 24 | (1 << 21), 24 | (1 << 17), 24 | (7 << 17), 56, 56 | (1 << 21), 56 | (1 << 17),
                56 | (5 << 17), 120, 120 | (1 << 17), 56 | 64, 120 | 64, 56 | 256, 120 | (1 << 22), 56 | (1 << 22)]   # test_gpu_parity.py
SWEEP_WORDS = [1, 8, 24, 56, 120]                                                                      # test_gpu_random_sweep.py
BF16_IO = [(True, False), (False, True), (True, True)]


def _rq(rid, entry="indexed", layout="nhwc", jp=16, J=15, B=2, V=3, cube=(24, 16, 20), **flags):
    return dict(id=rid, entry=entry, layout=layout, jp=jp, J=J, B=B, V=V, h=H, w=W, cube=tuple(cube), **flags)


def requests():
    out = []
    for jp in (4, 8, 12, 16):
        out.append(_rq(f"nhwc_jp{jp}_z20", jp=jp, J=jp - 1))                                   # pipe
        out.append(_rq(f"nhwc_jp{jp}_z32", jp=jp, J=jp - 1, cube=(24, 16, 32)))                # brick stacks
        out.append(_rq(f"nhwc_jp{jp}_cl", jp=jp, J=jp, cl=True))                               # bricks
    for i, o in BF16_IO:
        for cl in (False, True):
            out.append(_rq(f"bf16_in{int(i)}_out{int(o)}_cl{int(cl)}", J=16 if cl else 15, in_bf16=i, out_bf16=o, cl=cl))
    out.append(_rq("strided_dense", entry="strided"))
    out.append(_rq("strided_padded", entry="strided", pad=(2, 2, 4)))
    out.append(_rq("train_planar", entry="train"))
    out.append(_rq("train_cl", entry="train", J=16, cl=True))
    out.append(_rq("zdft_root_grid", entry="zdft", B=1, V=5, cube=(80, 80, 20)))
    for J in (1, 4, 15):
        out.append(_rq(f"planar_J{J}", layout="planar", jp=0, J=J))
    for Z in (20, 32):
        for J in (17, 20, 21, 25, 29, 32):
            out.append(_rq(f"wide_J{J}_z{Z}", jp=32, J=J, cube=(24, 16, Z)))
        for i, o in BF16_IO:
            out.append(_rq(f"wide_J17_in{int(i)}_out{int(o)}_z{Z}", jp=32, J=17, cube=(24, 16, Z), in_bf16=i, out_bf16=o))
    for V in (1, 5, 7, 9, 12, 16):
        for layout in ("planar", "nhwc"):
            for cl in (False, True):
                out.append(_rq(f"one_V{V}_{layout}_cl{int(cl)}", layout=layout, jp=5, J=4 if cl else 1, V=V, one=True, cl=cl))
    words = sorted(set(PARITY_WORDS + SWEEP_WORDS))
    for B in (1, 2, 3, 4):
        for word in words:
            out.append(_rq(f"word_{word}_B{B}", entry="variant", B=B, word=word))
        for word in (120, 120 | (1 << 22)):                                                    # tools/pmc_blocks.sh
            out.append(_rq(f"word_{word}_cl_B{B}", entry="variant", J=16, B=B, word=word, cl=True))
    assert len({r["id"] for r in out}) == len(out)
    return out
