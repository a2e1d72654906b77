"""CPU emulation of conv3_split128_kernel's accumulation (sp3d_conv3_quarter.hip) on one mid_res-like residual block,
against float64 - run BEFORE the kernel was written, to decide how many K-partials a workgroup keeps.

    python tools/sim_quarter_direct_error.py [--partials 4] [--json profiles/r15_quarter_direct_errors.json]

What is emulated: the exact products of the bf16 pieces (hi, mid, lo of both operands; the six products the kernel forms),
each matrix instruction's 16-term dot product formed without rounding (float64) and added to an fp32 accumulator in the
kernel's order - chunk by chunk, within a chunk the taps wave, wave + 4, ... of each wave - then the four (or eight: two
alternating accumulator sets per wave) partial sums added in fp32 in their fixed order, then the fp32 epilogue.  What is
not: the matrix instruction's internal summation order, hence the rule "emulated error <= half the bound".
Block: x (1,128,20,20,5) >= 0 (a ReLU output of unit spread), y = relu(conv2(relu(conv1(x) + s1)) + s2 + x), weights of
unit output spread (what tests/test_gpu_v2v_plan_f64.py::fill_far_from_identity arranges).  Metric: max|d| / max(1, max|f64|),
bound 2.0e-6 (BOUNDS["conv3_split128_"], the same figure as the three-launch form's BOUNDS["wino_conv3d_"])."""
import argparse
import json
import os

import numpy as np

BOUND = 2.0e-6


def bf16(a):
    """float32 array -> nearest-even bfloat16, as float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.view(np.float32)


def split3(a):
    a = a.astype(np.float32)
    hi = bf16(a)
    r = a - hi
    mid = bf16(r)
    lo = bf16(r - mid)
    return hi.astype(np.float64), mid.astype(np.float64), lo.astype(np.float64)


def conv_emulated(x, w, partials):
    """x (X,Y,Z,C) fp32, w (O,C,3,3,3) fp32 -> (X,Y,Z,O) fp32 by the kernel's accumulation order"""
    X, Y, Z, C = x.shape
    O = w.shape[0]
    xp = np.zeros((X + 2, Y + 2, Z + 2, C), np.float32)
    xp[1:-1, 1:-1, 1:-1] = x
    xh, xm, xl = split3(xp)
    wh, wm, wl = split3(w)
    acc = np.zeros((partials, X * Y * Z, O), np.float32)
    sets = partials // 4
    for cc in range(C // 8):
        c0 = slice(8 * cc, 8 * cc + 8)
        for wave in range(4):
            for j, tap in enumerate(range(wave, 27, 4)):
                dz, dy, dx = tap // 9, (tap // 3) % 3, tap % 3
                sl = (slice(dx, dx + X), slice(dy, dy + Y), slice(dz, dz + Z), c0)
                ah, am, al = (p[sl].reshape(-1, 8) for p in (xh, xm, xl))
                bh, bm, bl = (p[:, c0, dx, dy, dz].T for p in (wh, wm, wl))
                p = wave * sets + (j % sets)
                for dot in (al @ bh + ah @ bl, ah @ bh + am @ bh, ah @ bm + am @ bm):      # the three matrix instructions
                    acc[p] = (acc[p].astype(np.float64) + dot).astype(np.float32)
    out = acc[0]
    for p in range(1, partials):
        out = out + acc[p]
    return out.reshape(X, Y, Z, O)


def conv_f64(x, w):
    X, Y, Z, C = x.shape
    xp = np.zeros((X + 2, Y + 2, Z + 2, C), np.float64)
    xp[1:-1, 1:-1, 1:-1] = x
    out = np.zeros((X * Y * Z, w.shape[0]), np.float64)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out += xp[dx:dx + X, dy:dy + Y, dz:dz + Z].reshape(-1, C) @ w[:, :, dx, dy, dz].T.astype(np.float64)
    return out.reshape(X, Y, Z, -1)


def block_error(partials, seed=0, grid=(20, 20, 5), C=128):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal(grid + (C,)), 0).astype(np.float32)
    ws, ss = [], []
    for _ in range(2):
        w = rng.standard_normal((C, C, 3, 3, 3)) * 2.0 ** rng.uniform(-1, 1, (C, 1, 1, 1, 1))
        ws.append(w)
        ss.append(rng.uniform(-1, 1, C).astype(np.float32))
    # unit output spread per channel, on the float64 path
    h64 = conv_f64(x, ws[0])
    ws[0] = (ws[0] / h64.std(axis=(0, 1, 2)).reshape(-1, 1, 1, 1, 1)).astype(np.float32)
    h64 = np.maximum(conv_f64(x, ws[0]) + ss[0], 0)
    y64 = conv_f64(h64, ws[1])
    ws[1] = (ws[1] / y64.std(axis=(0, 1, 2)).reshape(-1, 1, 1, 1, 1)).astype(np.float32)
    y64 = np.maximum(conv_f64(h64, ws[1]) + ss[1] + x, 0)
    h = np.maximum(conv_emulated(x, ws[0], partials) + ss[0], np.float32(0))
    y = np.maximum((conv_emulated(h, ws[1], partials) + ss[1]) + x, np.float32(0))
    den = max(1.0, float(np.abs(y64).max()))
    # one layer alone, the same metric: the first conv against float64 on the same input
    e1 = float(np.abs(h.astype(np.float64) - h64).max()) / max(1.0, float(np.abs(h64).max()))
    return {"partials": partials, "K": 27 * C, "block_error": float(np.abs(y.astype(np.float64) - y64).max()) / den,
            "first_layer_error": e1, "max_abs_f64": float(np.abs(y64).max())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--partials", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--json")
    a = ap.parse_args()
    res = [block_error(p) for p in a.partials]
    for r in res:
        r["within_half_the_bound"] = r["block_error"] <= BOUND / 2
        print(json.dumps(r))
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc["emulation"] = {"tool": "tools/sim_quarter_direct_error.py", "bound": BOUND, "rule": "emulated block error <= bound / 2",
                            "results": res}
        json.dump(doc, open(a.json, "w"), indent=1)
