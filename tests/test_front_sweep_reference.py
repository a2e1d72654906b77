"""The opening-conv sweep's own parts, without a GPU (tests/front_sweep_cases.py): the table covers the rows, classes and
values it says, every float64 referee agrees with a naive evaluation of the same operation, every case has signal, the
comparison rejects altered outputs at every row's effective bound, and the entries the sweep guards take ``out=``."""
import inspect

import pytest
import torch

from tests import front_sweep_cases as fs

_names = [r.name for r in fs.ROWS]


def test_table_covers_every_row_class_and_value():
    assert _names == ["zdft_fwd_cl", "zdft_inv_cl", "cfft2d_88", "cfft2d_88_tiled", "freq_contract", "freq_contract_ty",
                      "crop_shift_act_cl", "unproject_fwd_zdft", "front"]
    assert [r.rule for r in fs.ROWS] == ["library"] * 7 + ["bits", "bound"]
    for r in fs.ROWS:                                   # no factor above 1.5 without its measured ratio and reason
        assert r.factor in (None, 1.5) or (r.factor > 1.5 and r.why), r
    by = {r.name: fs.cases(r) for r in fs.ROWS}
    for name, cs in by.items():
        tags = [fs.tag_of(c) for c in cs]
        assert len(set(tags)) == len(tags), name
    # zdft_fwd_cl: the padded plane against the 16-position tile, every Cout and batch on every class
    zf = by["zdft_fwd_cl"]
    assert {c["dims"] for c in zf} == {(1, 1, 2, 6), (2, 3, 4, 4), (20, 18, 22, 18), (4, 6, 4, 6), (12, 10, 18, 16)}
    planes = sorted({c["dims"][2] * c["dims"][3] for c in zf})
    assert planes == [12, 16, 24, 288, 396] and 396 % 16 == 12 and 18 % 16 != 0
    assert any(c["dims"][0] == c["dims"][2] and c["dims"][1] == c["dims"][3] for c in zf)
    assert len(zf) == 5 * 3 * 2 and {(c["cout"], c["B"]) for c in zf} == {(co, B) for co in (1, 15, 16) for B in (1, 2)}
    # zdft_inv_cl: Y against the 16-row tile
    zi = by["zdft_inv_cl"]
    assert {c["dims"][1] for c in zi} == {1, 15, 16, 17, 33} and {c["dims"][0] for c in zi} == {1, 3}
    for Y in (1, 15, 16, 17, 33):
        sub = [c["dims"] for c in zi if c["dims"][1] == Y]
        assert any(d[3] == Y for d in sub) and any(d[3] > Y for d in sub) and {d[0] for d in sub} == {1, 3}, Y
    assert any(c["dims"][0] == c["dims"][2] for c in zi) and any(c["dims"][0] < c["dims"][2] for c in zi)
    assert len(zi) == 10 * 2 * 2 and {(c["relu"], c["B"]) for c in zi} == {(r, B) for r in (True, False) for B in (1, 2)}
    # the 88 x 88 plane transform
    f88 = [c for c in by["cfft2d_88"] if c["kind"] == "f88"]
    assert {c["rows"][0] for c in f88} == set(fs.ROWS_88) == {c["rows"][1] for c in f88} == {1, 3, 75, 80, 82, 87, 88}
    assert {(1, 1), (80, 80), (88, 88), (87, 3), (3, 87)} <= {c["rows"] for c in f88}
    for p in fs.PAIRS_88:
        assert {(c["inverse"], c["planes"]) for c in f88 if c["rows"] == p} == {(i, n) for i in (False, True) for n in (1, 3)}
    assert any(not c["inverse"] and c["rows"][1] < 88 for c in f88)           # forward on the "way back" pass order
    assert any(c["inverse"] and c["rows"][0] < 88 for c in f88)               # inverse of planes with padding rows
    assert [c["kind"] for c in by["cfft2d_88"][-2:]] == ["f88_unaligned", "f_other"] and by["cfft2d_88"][-1]["size"] == (48, 32)
    assert {(c["xy"], c["planes"]) for c in by["cfft2d_88_tiled"]} == {
        (xy, n) for xy in ((4, 4), (4, 88), (88, 4), (76, 84), (80, 80), (88, 88)) for n in (1, 3)}
    # the contractions: pairwise coverage of the listed values
    assert dict(fs.CONTRACT_FACTORS) == dict(I=(1, 2, 3, 4, 5), J=(1, 8, 9, 16, 17), K=(1, 15, 16), F=(1, 255, 256, 257, 513),
                                             form=("plain", "fwd", "dx", "dw"))
    assert fs.covers_pairwise(by["freq_contract"], fs.CONTRACT_FACTORS) and len(by["freq_contract"]) <= 40
    assert dict(fs.TY_FACTORS) == dict(rows=(1, 3, 4, 5, 31, 32, 33, 36), O=(1, 4, 5, 16), C=(1, 15, 16), SY=(8, 20, 88, 96),
                                       B=(1, 4, 5))
    ty = by["freq_contract_ty"]
    assert fs.covers_pairwise(ty[:-1], fs.TY_FACTORS) and len(ty) <= 50
    assert ty[-1] == dict(kind="ty_plan", S=(8, 20, 28), C=15, O=16, B=2)
    assert 4 * 96 == 384 and (33 + 3) // 4 > 8                                  # SY = 96 fills the block; 33 rows: a second group of 8
    # crop, unprojection, the whole front
    cr = by["crop_shift_act_cl"]
    assert {c["cls"] for c in cr} == {"thin", "ragged", "no_crop"} and {c["relu"] for c in cr} == {True, False}
    C, X, Y, Zc, SX, SY, SZc = fs.CROP_CLASSES["ragged"]
    assert Y % 4 and X < SX and Y < SY and Zc < SZc and fs.CROP_CLASSES["no_crop"][1:4] == fs.CROP_CLASSES["no_crop"][4:]
    assert [(c["cube"], c["V"], c["valid"]) for c in by["unproject_fwd_zdft"]] == [
        ((4, 4, 20), 1, (1, 1)), ((8, 12, 20), 5, (1, 0)), ((76, 84, 20), 5, (1, 1))]
    fr = {c["route"]: c for c in by["front"]}
    assert list(fr) == ["zdft_library_planes", "zdft_88_planes", "zdft_88_planes_ty", "zspectrum_88_planes", "rfft_cin15",
                        "rfft_cin1", "rfft_z_not_4"]
    assert fr["zdft_library_planes"]["grid"] == (12, 10, 20) and fr["zdft_88_planes"]["grid"] == (76, 82, 20)
    assert fr["zdft_88_planes_ty"]["grid"] == (76, 82, 20) and fr["zdft_88_planes_ty"]["ty"] and fr["zdft_88_planes"]["B"] == 2
    assert fr["rfft_cin15"]["grid"] == (6, 5, 8) and (fr["rfft_cin1"]["cin"], fr["rfft_cin1"]["fc"]) == (1, 4)
    assert fr["rfft_z_not_4"]["grid"][2] % 4 and "channel_shift_act_" in fr["rfft_z_not_4"]["calls"]
    for c in fr.values():
        assert not set(c["calls"]) & set(c["never"])


def test_front_routes_have_the_fft_shapes_they_are_named_for():
    from selfpose3d_amd.v2v_net import _FoldedV2V
    fr = {c["route"]: c for c in fs.cases(fs.ROW["front"])}
    assert _FoldedV2V._fft_shape(*fr["zdft_library_planes"]["grid"], 7) == (18, 16, 28)
    assert _FoldedV2V._fft_shape(*fr["zdft_88_planes"]["grid"], 7) == (88, 88, 28)
    assert _FoldedV2V._fft_shape(*fr["zspectrum_88_planes"]["grid"], 7) == (88, 88, 28)
    for X in range(75, 83):                              # the grids of the issue: 88-point planes with rows_in = X != 80
        assert _FoldedV2V._fft_shape(X, X, 20, 7) == (88, 88, 28)
    assert _FoldedV2V._fft_shape(*fr["rfft_z_not_4"]["grid"], 7)[2] % 4 == 0


def test_every_guarded_entry_takes_out():
    """the sweep hands every entry a guarded buffer: ``out`` is keyword-only, last, and defaults to a fresh tensor"""
    from selfpose3d_amd import _lib
    assert set(fs.OUT_ENTRIES) == {e for r in fs.ROWS for e in r.entries} - {"cfft2d_"}
    for entry in fs.OUT_ENTRIES:
        ps = inspect.signature(getattr(_lib, entry)).parameters
        assert ps["out"].kind is inspect.Parameter.KEYWORD_ONLY and ps["out"].default is None, entry
        assert list(ps)[-1] == "out", entry


def test_out_is_validated_for_shape_type_density_and_alignment():
    from selfpose3d_amd import _lib
    dev = torch.device("cpu")
    shape = (2, 16, 3, 5, 20)
    good = _lib._result_dense(None, shape, torch.float32, dev, "t", 16, cl3d=True)
    assert tuple(good.shape) == shape and good.permute(0, 2, 3, 4, 1).is_contiguous()
    assert _lib._result_dense(good, shape, torch.float32, dev, "t", 16, cl3d=True) is good
    buf = torch.empty(2 * 16 * 3 * 5 * 20 + 8)
    off = [o for o in range(4) if (buf.data_ptr() + 4 * o) % 16][0]
    bad = [torch.empty((2, 16, 3, 5, 21)).permute(0, 4, 1, 2, 3),                                  # another shape
           torch.empty(shape),                                                                    # planar where channels-last is due
           torch.empty((2, 3, 5, 20, 16), dtype=torch.float64).permute(0, 4, 1, 2, 3),            # another type
           torch.empty((2, 3, 5, 20, 32)).permute(0, 4, 1, 2, 3)[:, ::2],                         # not dense
           buf[off:off + 2 * 16 * 3 * 5 * 20].view(2, 3, 5, 20, 16).permute(0, 4, 1, 2, 3)]       # not 16-byte aligned
    for out in bad:
        with pytest.raises(_lib.Sp3dError):
            _lib._result_dense(out, shape, torch.float32, dev, "t", 16, cl3d=True)
    c = torch.empty((3, 4, 7), dtype=torch.complex64)
    assert _lib._result_dense(c, (3, 4, 7), torch.complex64, dev, "t") is c
    for out in (c[:, :, :6], c.transpose(0, 1), torch.empty((3, 4, 7, 2)), c.to(torch.complex128)):
        with pytest.raises(_lib.Sp3dError):
            _lib._result_dense(out, (3, 4, 7), torch.complex64, dev, "t")


def _is_small(case):
    """the classes a naive evaluation still finishes on at once"""
    k = case["kind"]
    if k == "contract":
        return case["F"] <= 257 and case["I"] * case["J"] * case["K"] <= 400
    if k == "ty":
        return case["rows"] * case["SY"] * case["O"] * case["C"] <= 12000
    if k in ("f88", "f88_unaligned", "tiled"):
        return case["planes"] == 1
    if k == "zfwd":
        return case["cls"] != "straddle" or case["cout"] == 15
    return True


@pytest.mark.parametrize("name", [n for n in _names if n not in ("unproject_fwd_zdft", "front")])
def test_referee_equals_naive_evaluation(name):
    row = fs.ROW[name]
    seen = 0
    for case in fs.cases(row):
        if not _is_small(case):
            continue
        ins = fs.make_inputs(case)
        ref, naive = fs.referee(case, ins), fs.referee(case, ins, naive=True)
        assert ref.shape == naive.shape and ref.dtype in (torch.float64, torch.complex128)
        e = fs.compare(naive, ref)["err"]
        # the plan's tables are fp32 roundings of float64 values: the formula on them is the exact spectrum to a few 2^-24
        tol = 4e-7 if case["kind"] == "ty_plan" else 1e-12
        assert max(e) <= tol, (case, e)
        seen += 1
    assert seen >= 3


def test_front_referee_equals_naive_convolution():
    for route in ("rfft_cin15", "rfft_cin1", "rfft_z_not_4"):
        case = [c for c in fs.cases(fs.ROW["front"]) if c["route"] == route][0]
        w0, s0 = _folded_front(case)
        x = fs.make_inputs(case)["x"]
        ref, naive = fs.ref_front(x, w0, s0), fs.naive_front(x, w0, s0)
        assert max(fs.compare(naive, ref)["err"]) <= 1e-12


def _folded_front(case):
    from selfpose3d_amd.v2v_net import _FoldedV2V
    net = fs.front_net(case["cin"], True)
    blk = net.front_layers[0].block
    with torch.no_grad():
        return _FoldedV2V._fold(blk[0], blk[1])


def test_unproject_spectrum_referee_and_tiling():
    """the tiled layout's round trip, and the z-spectrum referee against a DFT matrix on the oracle's cubes"""
    case = fs.UNPROJECT_CASES[1]
    u = fs.unproject_inputs(dict(kind="unproject", **case))
    cubes = u["cubes"]
    assert tuple(cubes.shape) == (2, 15, 8, 12, 20) and float(cubes[0].max()) > 0.2 and not bool(cubes[1].any())
    ref = fs.ref_unproject_spectrum(cubes, 15)
    x16 = torch.cat([cubes, torch.zeros(2, 1, 8, 12, 20)], 1)
    assert max(fs.compare(fs.naive_zfwd(x16, 15, 8, 12), ref)["err"]) <= 1e-12
    t = fs.tile44(ref)
    assert tuple(t.shape) == (2, 15, 15, 2, 3, 16) and torch.equal(fs.untile44(t, 8, 12), ref)
    assert t[0, 0, 0, 1, 2, 4 * 3 + 1] == ref[0, 0, 0, 7, 9]              # inside a tile: 4 * (x % 4) + (y % 4)


def test_sample_one_is_a_thousand_times_sample_zero_and_first_sample_is_sample_zero():
    key = {"zfwd": "x", "zinv": "spec", "f88": "x", "tiled": "x", "contract": "P", "ty": "X", "ty_plan": "X", "crop": "src", "front": "x"}
    seen = set()
    for name in _names:
        for case in fs.cases(fs.ROW[name]):
            k = case["kind"]
            if k not in key or case.get("B", case.get("planes", case.get("I", 1))) < 2:
                continue
            ins = fs.make_inputs(case)
            full, one = ins[key[k]], fs.first_sample(ins, case)[key[k]]
            if k == "contract" and case["form"] == "dw":
                full, one = full.transpose(0, 1), one.transpose(0, 1)
            assert one.shape[0] == 1 and torch.equal(one[0], full[0]), case
            assert 300.0 < float(full[1].abs().max() / full[0].abs().max()) < 3000.0, case
            assert all(v is ins[n] for n, v in fs.first_sample(ins, case).items() if n != key[k])
            seen.add(k)
    assert seen == set(key)


@pytest.mark.parametrize("name", _names)
def test_every_case_has_signal_and_compare_rejects_altered_outputs(name):
    """signal on every case; teeth on the row's largest batched case, each alteration visible in sample 0 at the row's effective
    bound: one bin / voxel off by 1e-3 of the range, one tile (16 positions, a 4-row block, an output-channel group) zeroed, two
    rows swapped, sample 0 contaminated by 1e-6 of sample 1 (the unprojection's samples are not scaled: there the
    bit-identity check is what sees a neighbour, and it sees any change)."""
    row = fs.ROW[name]
    bound = fs.effective_bound(row)
    assert bound <= 3.0e-6 + 1e-12
    teeth = None
    for case in fs.cases(row):
        k = case["kind"]
        if k == "unproject":
            ref = fs.ref_unproject_spectrum(fs.unproject_inputs(case)["cubes"], fs.UNPROJECT_J)
            cmp = fs.compare(ref.to(torch.complex64), ref)
            assert all(r > 1.0 for r, v in zip(cmp["range"], case["valid"]) if v) and \
                all(r == 0.0 for r, v in zip(cmp["range"], case["valid"]) if not v)
        elif k == "front":
            if max(case["grid"]) > 20:
                continue                                   # the 76 x 82 x 20 referee runs on the GPU; same nets and seeds
            w0, s0 = _folded_front(case)
            ref = fs.ref_front(fs.make_inputs(case)["x"], w0, s0)
            cmp = fs.compare(ref.float(), ref)
            assert fs.has_signal(case, cmp), (case, cmp["pos"])
        else:
            ref = fs.referee(case, fs.make_inputs(case))
            cmp = fs.compare(ref.to(torch.complex64 if ref.is_complex() else torch.float32), ref)
            assert fs.has_signal(case, cmp), (case, cmp)
        assert max(cmp["err"]) <= 1.2e-7 and max(cmp["err"]) <= bound / 10, (case, cmp["err"])      # the rounded exact answer passes
        if ref.shape[0] >= 2 and ref[0].numel() >= 64 and (teeth is None or ref.numel() > teeth[1].numel()):
            teeth = (case, ref)
    case, ref = teeth[0], teeth[1].contiguous()
    flat = ref[0].reshape(-1)
    rng = float(flat.abs().max())
    a = ref.clone()
    a[0].view(-1)[int(flat.abs().argmax())] += 1e-3 * rng
    b = ref.clone()
    bflat = b[0].reshape(-1)
    start = (int(flat.abs().argmax()) // 16) * 16
    bflat[start:start + 16] = 0.0
    b[0] = bflat.reshape(ref[0].shape)
    c = ref.clone()
    ax = ref[0].dim() - 2                                                # rows: x of a plane, j of an (j, f) slab, y of a volume
    n = ref[0].shape[ax]
    r0 = int(ref[0].abs().movedim(ax, 0).reshape(n, -1).amax(1).argmax())
    order = list(range(n))
    order[r0], order[(r0 + 1) % n] = order[(r0 + 1) % n], order[r0]
    c[0] = ref[0].index_select(ax, torch.tensor(order))
    alts = [("bin", a), ("tile", b), ("rows", c)]
    if case["kind"] != "unproject":
        d = ref.clone()
        d[0] += 1e-6 * ref[1]
        alts.append(("neighbour", d))
    for kind, alt in alts:
        assert not torch.equal(alt, ref), kind
        e = fs.compare(alt, ref)["err"]
        assert e[0] > bound, (name, kind, e, bound)
    # a NaN left in a result fails the comparison whatever the bound
    n = ref.clone()
    n[0].view(-1)[0] = float("nan")
    assert not fs.compare(n, ref)["err"][0] <= bound
