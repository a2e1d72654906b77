"""tests/train_sweep_cases.py without a GPU: the tables enter every class the issue of the sweep names (asserted through the
geometry helpers), the helpers restate sp3d_gbn.hip, the float64 referees agree with independent forms (a per-group
nn.BatchNorm loop, a per-element loop, the CPU paths of
cuboid_proposal_net_soft.py), the conditions on the inputs hold (mask-edge shares, shares of positive outputs, nonzero
gradient scales), and the comparison functions reject every emulated defect."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import train_sweep_cases as ts

F32, F64 = ts.F32, ts.F64
_small = [c for c in ts.all_gbn_cases() if c["C"] <= 48]
_all = ts.all_gbn_cases()


def find(pred, cases=None):
    for c in (_all if cases is None else cases):
        if pred(c):
            return c
    raise AssertionError("the table holds no such case")


# ---- geometry --------------------------------------------------------------------------------------------------------------
def test_geometry_helpers_restate_the_kernel_source():
    g = ts.gbn_geometry
    # GbnMap, sp3d_gbn.hip:55-60: cpp = min(CV, 256), RP = 256 / cpp, active = ro < RP, ncol = ceil(CV / 256)
    assert (g(F32, 4, 4, 1)["CV"], g(F32, 4, 4, 1)["RP"], g(F32, 4, 4, 1)["idle_threads"]) == (1, 256, 0)
    assert (g(F32, 20, 3, 409)["CV"], g(F32, 20, 3, 409)["RP"], g(F32, 20, 3, 409)["idle_threads"]) == (5, 51, 1)
    assert (g(F32, 1024, 3, 139)["CV"], g(F32, 1024, 3, 139)["RP"], g(F32, 1024, 3, 139)["passes"]) == (256, 1, 1)
    assert (g(F32, 1028, 1, 1)["CV"], g(F32, 1028, 1, 1)["passes"]) == (257, 2)
    assert (g(F32, 1536, 1, 1)["CV"], g(F32, 2048, 1, 1)["CV"]) == (384, 512)
    assert (g(F64, 6, 1, 1)["CV"], g(F64, 6, 1, 1)["RP"], g(F64, 6, 1, 1)["idle_threads"]) == (3, 85, 1)
    assert (g(F64, 514, 1, 1)["CV"], g(F64, 1024, 1, 1)["CV"], g(F64, 1024, 1, 1)["passes"]) == (257, 512, 2)
    # gbn_rows, sp3d_gbn.hip:413-420: rows = max(RP 8, roundup(ceil(N S / 2048), RP 8)); chunks, :453
    assert (g(F32, 32, 3, 256)["rows"], g(F32, 32, 3, 256)["chunks"], g(F32, 32, 3, 257)["chunks"]) == (256, 1, 2)
    assert (g(F32, 20, 3, 409)["rows"], g(F32, 20, 3, 409)["chunks"]) == (408, 2)
    assert (g(F32, 1024, 3, 139)["rows"], g(F32, 1024, 3, 139)["chunks"]) == (8, 18)
    assert (g(F32, 4, 4, 3)["rows"], g(F32, 4, 4, 3)["chunks"]) == (2048, 1)
    # the apply grid, sp3d_gbn.hip:454-458: ab = min(ceil(S CV / 1024), ceil(4096 / N)), at least 1
    big = g(F32, 1024, 2, 8300)
    assert (big["rows"], big["rows_min"], big["chunks"], big["ab_free"], big["cap"], big["ab"]) == (16, 8, 519, 2075, 2048, 2048)
    assert g(F32, 4, 3, 1)["ab"] == 1 and g(F32, 2048, 40, 5)["ab"] == 3
    # the finaliser grid, :460: ceil(C / 16) blocks of 16 channels - C = 4 fills a quarter of one, C = 20 a quarter of its second
    assert g(F32, 4, 1, 1)["fin_blocks"] == 1 and g(F32, 20, 1, 1)["fin_blocks"] == 2 and 20 % 16 == 4
    # gbn_check, :403-410
    for dtype, C in ts.REFUSED:
        assert ts.gbn_refusal(dtype, C) == ts.EUNSUPPORTED
    for dtype, C in ts.COLUMNS:
        assert ts.gbn_refusal(dtype, C) == 0
    assert {(F32, 2052), (F64, 1026), (F32, 6)} <= set(ts.REFUSED) and any(d == F64 and C % 2 for d, C in ts.REFUSED)
    # the root maps' grid, sp3d_synth.hip:100
    assert ts.root_blocks(129, 130) == (64, True) and (129 * 130 + 255) // 256 == 66 and ts.root_blocks(3, 5) == (1, False)


def test_the_table_enters_every_class():
    cols = set(ts.COLUMNS)
    assert {(F32, C) for C in (4, 20, 48, 1024, 1028, 1536, 2048)} <= cols
    assert {(F64, C) for C in (2, 6, 512, 514, 1024)} <= cols
    every = set()
    for dtype, C in ts.COLUMNS:
        cases = ts.gbn_cases(dtype, C)
        names = set().union(*(ts.gbn_classes(c) for c in cases))
        every |= names
        assert {"S=1", "S=rows", "S=rows+1", "S=2rows-1", "one value", "interleaved", "ragged", "no affine", "no running",
                "G_update=0", "G_update=G", "momentum=0.1", "momentum=0.5", "momentum=1"} <= names, (dtype, C, names)
        if ts.gbn_geometry(dtype, C, 1, 1)["RP"] > 3:
            assert "S<RP" in names
        assert {(c["mode"], c["family"]) for c in cases} >= {(m, f) for m in (0, 1, 2) for f in ts.FAMILIES}
        for c in cases:                                     # the row classes keep rows at its minimum, as their names say
            geo = ts.gbn_geometry(dtype, C, c["N"], c["S"])
            assert geo["rows"] == geo["rows_min"] and geo["ab_free"] <= geo["cap"]
    grouped = [c for c in _all if (c["dtype"], c["C"]) in ts.GROUP_COLUMNS]
    for dtype in (F32, F64):
        for mode in (1, 2):
            names = set().union(*(ts.gbn_classes(c) for c in grouped if c["mode"] == mode and c["dtype"] == dtype))
            assert {"G=1", "G=8", "G=9", "G=16", "G=17", "second replica fetch", "third replica fetch", "interleaved", "ragged",
                    "empty group in the middle", "one value", "G_update=0", "G_update=G-1", "G_update=G"} <= names, (dtype, mode)
            assert any(c["N"] == 40 and c["G"] == 17 and c["mode"] == mode for c in grouped)
            assert any(c["family"] == "zero-pad" and c["sizes"][-1] == 0 and c["sizes"][-2] > 0 and c["G_update"] == c["G"] - 3 and c["mode"] == mode for c in grouped)
    assert any(c["sizes"] == [2, 0, 3] for c in _all)
    assert any(c["sizes"][0] == 1 and c["S"] == 1 for c in _all)
    assert find(lambda c: (c["C"], c["S"]) == (4, 3)) and find(lambda c: (c["C"], c["S"]) == (20, 409))
    assert {c["S"] for c in _all if c["C"] == 32 and c["dtype"] == F32} >= {256, 257}
    assert "replicas wrap" in ts.gbn_classes(find(lambda c: (c["C"], c["N"], c["S"]) == (1024, 3, 139)))
    assert {"idle threads", "C%16!=0", "second column pass"} <= every
    big = ts.gbn_classes(ts.large_case())
    assert {"rows>min", "apply cap binds", "replicas wrap"} <= big
    assert not any({"rows>min", "apply cap binds"} & ts.gbn_classes(c) for c in _all)          # the only large case
    # rendering
    tc = ts.target_cases()
    assert {(c["shape"], c["R"], c["family"]) for c in tc} == {(s, r, f) for s in ((5, 7, 9), (1, 1, 1)) for r in (1, 10)
                                                               for f in ("random", "window edge", "outside")}
    assert 5 * 7 * 9 % 256
    for h, w in ts.ROOT_IMAGES:
        rc = ts.root_cases(h, w)
        assert {c["R"] for c in rc} == {1, 10} and any(c["behind"] for c in rc) and all(c["B"] == 3 for c in rc)


# ---- the referees ------------------------------------------------------------------------------------------------------------
def _bn_loop(case, ins):
    """per-group nn.BatchNorm1d in float64 on the CPU, in group order"""
    C = case["C"]
    bn = nn.BatchNorm1d(C, eps=ts.EPS, momentum=case["momentum"], affine=True).double().train()
    plain = nn.BatchNorm1d(C, eps=ts.EPS, affine=False, track_running_stats=False).double().train()     # a padding group
    with torch.no_grad():
        if ins["weight"] is not None:
            bn.weight.copy_(ins["weight"].double()); bn.bias.copy_(ins["bias"].double())
        if ins["running_mean"] is not None:
            bn.running_mean.copy_(ins["running_mean"].double()); bn.running_var.copy_(ins["running_var"].double())
    x = ins["x"].double().requires_grad_(True)
    r = ins["residual"].double().requires_grad_(True)
    go = torch.as_tensor(case["group_of"])
    y = torch.zeros_like(x)
    for g in range(case["G"]):
        idx = torch.nonzero(go == g).flatten()
        xg = x[idx].permute(0, 2, 1)
        yg = bn(xg) if g < case["G_update"] else plain(xg) * bn.weight.view(1, -1, 1) + bn.bias.view(1, -1, 1)
        yg = yg.permute(0, 2, 1)
        if case["mode"] == 2:
            yg = yg + r[idx]
        y = y.index_put((idx,), torch.relu(yg) if case["mode"] else yg)
    (y * ins["dy"].double()).sum().backward()
    return dict(y=y.detach(), dx=x.grad, grad_residual=r.grad, grad_weight=bn.weight.grad, grad_bias=bn.bias.grad,
                running_mean=bn.running_mean, running_var=bn.running_var)


def _rel(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def test_gbn_referee_equals_a_per_group_batchnorm_loop():
    wide = [find(lambda c: c["C"] == C and c["dtype"] == d and c["family"] == f and c["mode"] == 2)
            for d, C, f in ((F32, 1028, "scaled"), (F64, 514, "offset100"))]
    n = 0
    for case in _small + wide:
        if any(s * case["S"] <= 1 for s in case["sizes"]):
            continue
        ins, ref, _ = ts.gbn_problem(case)
        want = _bn_loop(case, ins)
        for k in ("y", "dx", "grad_weight", "grad_bias") + (("grad_residual",) if case["mode"] == 2 else ()):
            assert _rel(ref[k], want[k]) <= 1e-12 * max(1.0, ts.f64_factor(ref) ** 0.5), (case["name"], k)
        if case["running"]:
            assert _rel(ref["running_mean"], want["running_mean"]) <= 1e-12 and _rel(ref["running_var"], want["running_var"]) <= 1e-12
        n += 1
    assert n > 100


def test_gbn_referee_equals_a_per_element_loop():
    for case in [c for c in _all if c["N"] * c["S"] * c["C"] <= 64][:12]:
        ins, ref, _ = ts.gbn_problem(case)
        x, dy, res = (ins[k].double().numpy() for k in ("x", "dy", "residual"))
        N, S, C = x.shape
        w = np.ones(C) if ins["weight"] is None else ins["weight"].double().numpy()
        b = np.zeros(C) if ins["bias"] is None else ins["bias"].double().numpy()
        for c in range(C):
            gw = gb = 0.0
            for g in range(case["G"]):
                vals = [(n, s) for n in range(N) if case["group_of"][n] == g for s in range(S)]
                if not vals:
                    assert ref["mean"][g, c] == 0 and abs(float(ref["invstd"][g, c]) - 1 / math.sqrt(ts.EPS)) < 1e-9
                    continue
                m = math.fsum(x[n, s, c] for n, s in vals) / len(vals)
                v = math.fsum((x[n, s, c] - m) ** 2 for n, s in vals) / len(vals)
                inv = 1 / math.sqrt(v + ts.EPS)
                d, xh = [], []
                for n, s in vals:
                    pre = (x[n, s, c] - m) * inv * w[c] + b[c] + (res[n, s, c] if case["mode"] == 2 else 0.0)
                    on = pre > 0 or case["mode"] == 0
                    assert abs(float(ref["y"][n, s, c]) - (pre if on else 0.0)) <= 1e-12 * max(1, abs(pre))
                    d.append(dy[n, s, c] if on else 0.0)
                    xh.append((x[n, s, c] - m) * inv)
                a, bb = math.fsum(d) / len(vals), math.fsum(p * q for p, q in zip(d, xh)) / len(vals)
                gb += math.fsum(d)
                gw += math.fsum(p * q for p, q in zip(d, xh))
                for (n, s), dv, xv in zip(vals, d, xh):
                    assert abs(float(ref["dx"][n, s, c]) - w[c] * inv * (dv - a - xv * bb)) <= 1e-10
            assert abs(float(ref["grad_bias"][c]) - gb) <= 1e-12 * max(1, abs(gb)) and abs(float(ref["grad_weight"][c]) - gw) <= 1e-10


def test_running_statistics_at_momentum_one_are_the_last_updating_group():
    case = find(lambda c: c["momentum"] == 1.0 and c["G"] == 9 and c["G_update"] == 8 and c["C"] == 32)
    ins, ref, _ = ts.gbn_problem(case)
    cnt = ref["cnt"][7]
    assert torch.equal(ref["running_mean"], ref["mean"][7]) and _rel(ref["running_var"], ref["var"][7] * cnt / (cnt - 1)) < 1e-15
    one = find(lambda c: c["sizes"][0] == 1 and c["S"] == 1 and c["G_update"] == 3 and c["C"] == 32)       # cnt = 1: no update
    ins, ref, _ = ts.gbn_problem(dict(one, G_update=1))
    assert torch.equal(ref["running_mean"], ins["running_mean"].double()) and torch.equal(ref["running_var"], ins["running_var"].double())


def _soft_net(hm=None):
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
    net = CuboidProposalNetSoft(load_config(None, NETWORK__ROOTNET_ROOTHM=True, NETWORK__ROOTNET_TRAIN_SYNTH=True))
    net.noise_std = 0.0
    if hm:
        net.hm_h, net.hm_w = hm
    return net


def test_target_and_root_referees_equal_the_cpu_paths():
    net = _soft_net()
    for case in ts.target_cases():
        ins = ts.target_inputs(case)
        net.cur_sigma = case["sigma"]
        net.grid1Dx, net.grid1Dy, net.grid1Dz = ins["gx"], ins["gy"], ins["gz"]
        ref = ts.target_referee(ins["roots"], ins["gx"], ins["gy"], ins["gz"], case["sigma"])
        assert float((net.target_cubes(ins["roots"]).double() - ref).abs().max()) <= 1e-7, case["name"]
        if case["family"] == "window edge":                  # the edge voxel is inside: exp(-4.5) (or more, from another root)
            for b, i, j, k in ins["edge"]:
                assert float(ref[b, i, j, k]) >= math.exp(-4.5) * (1 - 1e-15)
            assert any(abs(float(ref[e]) - math.exp(-4.5)) < 1e-15 for e in ins["edge"])
        if case["family"] == "outside":
            assert float(ref[0].abs().max()) == 0.0
        if case["family"] != "outside" and case["shape"] != (1, 1, 1):
            assert float(ref.max()) > 0.1
    for h, w in ts.ROOT_IMAGES:
        net = _soft_net((h, w))
        for case in ts.root_cases(h, w):
            ins = ts.root_inputs(case)
            net.stride = ins["stride"]
            ref, depth = ts.root_referee(ins["roots"], ins["cam"], h, w, ins["stride"])
            got = torch.stack(net.render_root_heatmaps(ins["roots"], ins["meta"]), 0)
            assert tuple(ref.shape) == tuple(got.shape) == (case["V"], 3, 1, h, w)
            assert float((got.double() - ref).abs().max()) <= 2e-5, case["name"]
            assert bool((depth[1, 0, 0] < 0)) == case["behind"]
        assert any(float(ts.root_referee(i["roots"], i["cam"], h, w, i["stride"])[0].max()) > 0.05
                   for i in map(ts.root_inputs, ts.root_cases(h, w)))


# ---- conditions on the inputs -------------------------------------------------------------------------------------------------
def _conditions(case):
    ins, ref, share = ts.gbn_problem(case)
    assert share <= ts.MASK_EDGE_CAP, (case["name"], share)
    if case["mode"] and ref["y"].numel() >= 256:
        pos = float((ref["y"] > 0).double().mean())
        assert 0.1 <= pos <= 0.9, (case["name"], pos)
    for k in ("grad_weight", "grad_bias", "dx"):
        assert float(ref[k].abs().max()) > 1e-6, (case["name"], k)
    if case["family"] == "zero-pad":                          # exact zeros at nonzero dy: only a strict > masks them
        pad = torch.as_tensor(case["group_of"]) >= case["G_update"]
        z = ins["zero_bias"]
        assert bool((ref["pre"][pad][:, :, z] == 0).all()) and float(ins["dy"][pad][:, :, z].abs().min()) > 0
        if case["mode"]:
            assert float(ref["dx"][pad][:, :, z].abs().max()) == 0.0
    if case["family"] in ("offset100", "offset1000"):
        r = (ref["mean"].abs() * ref["invstd"])
        want = 100.0 if case["family"] == "offset100" else 1000.0
        assert 0.5 * want <= float(r.median()) <= 2.5 * want, (case["name"], float(r.median()))
    if case["family"] == "constant":
        assert float(ref["var"][:, 1::4].max()) == 0.0 and float(ref["var"][:, 0::4].min()) > 0


def test_every_case_meets_its_conditions():
    for case in _all:
        _conditions(case)


def test_the_large_case_meets_its_conditions():
    _conditions(ts.large_case())


# ---- the comparison rejects each defect ----------------------------------------------------------------------------------------
def _verdict(case, defect):
    ins, ref, _ = ts.gbn_problem(case)
    bad = ts.gbn_problem(case, defect=defect)[1] if defect else ref
    lib = None
    if case["dtype"] == F32:
        lib = ts.gbn_library(case, ins["x"], ins["dy"], ins["residual"], ins["weight"], ins["bias"])
    return ts.gbn_compare(case, ts.round_like(case, bad), ref, lib)[0]


DEFECTS = [
    ("pooled", lambda c: c["family"] == "scaled" and c["G"] >= 2 and c["C"] == 32),
    ("pooled", lambda c: c["family"] == "normal" and c["G"] == 8 and c["C"] == 32),
    ("replica", lambda c: c["family"] == "normal" and c["C"] == 1028 and c["mode"] == 0),
    ("replica", lambda c: c["family"] == "offset1000" and c["C"] == 48 and c["mode"] == 1),
    ("skip8", lambda c: c["G"] == 9 and c["C"] == 32 and c["G_update"] == 9),
    ("skip8", lambda c: c["G"] == 17 and c["N"] == 40 and c["C"] == 2048),
    ("reverse", lambda c: c["momentum"] == 1.0 and c["G"] == 9 and c["G_update"] == 9 and c["C"] == 32),
    ("reverse", lambda c: c["momentum"] == 0.5 and c["G"] == 3 and c["C"] == 20),
    ("biased", lambda c: c["S"] == 1 and c["N"] == 4 and c["C"] == 2048),
    ("biased", lambda c: c["momentum"] == 0.1 and c["C"] == 4 and c["S"] > 2000),
    ("ge", lambda c: c["family"] == "zero-pad" and c["mode"] == 1 and c["C"] == 48),
    ("ge", lambda c: c["family"] == "zero-pad" and c["mode"] == 2 and c["C"] == 1536),
]


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("which", range(len(DEFECTS)))
def test_gbn_comparison_rejects_the_defect(which, dtype):
    defect, pred = DEFECTS[which]
    case = find(lambda c: pred(c) and c["dtype"] == dtype, _all + [dict(c, dtype=F64) for c in _all if c["dtype"] == F32])
    assert _verdict(case, None) == [], "the rounded referee itself must pass"
    fails = _verdict(case, defect)
    assert fails, (defect, case["name"])


def test_rounded_referee_passes_every_small_case():
    for case in _small[::3]:
        assert _verdict(case, None) == [], case["name"]


def test_an_exclusive_window_edge_is_far_over_the_target_tolerance():
    for case in ts.target_cases():
        if case["family"] == "window edge":
            ins = ts.target_inputs(case)
            ref = ts.target_referee(ins["roots"], ins["gx"], ins["gy"], ins["gz"], case["sigma"])
            bad = ts.target_referee(ins["roots"], ins["gx"], ins["gy"], ins["gz"], case["sigma"], inclusive=False)
            assert float((bad - ref).abs().max()) >= 0.9 * math.exp(-4.5) > 1000 * ts.TARGET_TOL, case["name"]


def test_guarded_buffers_catch_the_out_of_bounds_breakages():
    """the two breakages that may not run on a GPU, emulated on CPU copies of the guarded buffers of
    tests/test_gpu_train_sweep.py: the finaliser without ``c < C`` (C = 4: threads of channels 4 .. 15 store their mean past
    row g, the last group's past the end) and the block merge without ``col < CV`` (C = 1028: the second column pass adds
    columns 257 .. 511 to the next (replica, group) row, the last row's past the workspace)"""
    from tests.test_gpu_train_sweep import Guarded
    G, C = 3, 4
    mean = Guarded(G * C, torch.float32, "cpu")
    flat = mean.buf                                            # what the kernel's pointer arithmetic reaches
    for g in range(G):
        for c in range(16):                                    # ok = c < C dropped
            flat[ts_guard() + g * C + c] = 1.0
    assert any("AFTER" in p for p in mean.problems("mean")) and not any("BEFORE" in p for p in mean.problems("mean"))
    fine = Guarded(G * C, torch.float32, "cpu")
    fine.t.fill_(1.0)
    assert fine.problems("mean") == [] and not fine.untouched()
    C, CV, W = 1028, 257, 4
    ws = Guarded(16 * G * C * 2, torch.float64, "cpu", zero=True)
    row = (15 * G + (G - 1)) * C * 2                           # the last (replica, group) row
    for col in range(256, 512):                                # the second pass of every thread, col < CV dropped
        for e in range(W):
            ws.buf[ts_guard() + row + (col * W + e) * 2] += 1.0
    assert any("AFTER" in p for p in ws.problems("the workspace"))
    assert int(torch.count_nonzero(Guarded(8, torch.float64, "cpu", zero=True).t.view(torch.int64))) == 0


def ts_guard():
    from tests.test_gpu_train_sweep import GUARD
    return GUARD
