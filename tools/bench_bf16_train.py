#!/usr/bin/env python3
"""Training through bf16 heat-maps: ProjectLayer.bf16_train (SP3D_HM_BF16_TRAIN) against the route it replaces, same bf16 maps.

Forward + backward of the unprojection alone, through ``ProjectLayer.get_voxel`` under autograd: bf16 leaf heat-maps that
require a gradient -> fp32 cubes -> ``cubes.backward(grad)`` -> a bf16 ``.grad`` on every leaf.
  off   today's route: the views widened and re-tiled into fp32 pixels, the fp32 training forward, the scatter into a fp32
        buffer, the autograd engine casting each gradient view back to bf16
  on    ``bf16_train``: bf16 pixels re-tiled bf16 to bf16 (or one channel read where it lies), the bf16-tap training forward,
        the same scatter, the buffer rounded once
Legs: the root grid 80x80x20 at B = 1 and B = 4 for 15 joints (5 x 240x128 maps), 17 joints on the Campus and Shelf rigs
(``wide_grad``) and the one-channel root input (channel 2 of 15, ``one_channel_grad``); eight 64^3 person cubes over B = 4 at
15 joints.  Every leg with the fp32-atomic scatter and with the deterministic one.  The maps are new tensors to the layer in
every call, as in a training step (the pack cache is cleared); the one-channel legs run with ``cache_packs = False`` in both
layers, because today's route has no re-tile from bf16 planes into fp32 pixels of 4 channels and works from widened copies only.
Both legs run three times in every alternation.  The run-to-run spread is the largest difference between the medians of the
repeats of a leg (the larger of the two legs'), and the rule for a later flip of the default is
applied to the slowest switched-on repeat: below the switched-off median by more than the spread, in every leg.  Device events,
warm-up first, then --iters timed calls per repeat in alternating blocks of --block calls inside one process.

    python tools/bench_bf16_train.py [--iters 200] [--out profiles/r25_bf16_train.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from selfpose3d_amd import synthetic as syn  # noqa: E402
from selfpose3d_amd.config import load_config  # noqa: E402
from selfpose3d_amd.project_layer import ProjectLayer, clear_pack_cache  # noqa: E402
from tools.bench_roothm import aa_spread, stats, timed_legs  # noqa: E402

YAML = {"campus_synthetic": os.path.join(ROOT, "configs", "campus_synthetic_coco17_cam3.yaml"),
        "shelf_synthetic": os.path.join(ROOT, "configs", "shelf_synthetic_coco17_cam5.yaml")}
ROOT_CUBE, FINE_CUBE, CH = (80, 80, 20), (64, 64, 64), 2
BF = torch.bfloat16


def legs():
    """(key, config, rig, joints handed over, shape, the switches both layers get)"""
    out = []
    for shape in ("root_B1", "root_B4"):
        out.append((f"joints15_{shape}", None, None, 15, shape, {}))
        for rig in YAML:
            out.append((f"joints17_{rig}_{shape}", YAML[rig], rig, 17, shape, dict(wide_grad=True)))
        out.append((f"one_channel_{shape}", None, None, 1, shape, dict(one_channel_grad=True, cache_packs=False)))
    out.append(("joints15_fine_8x64", None, None, 15, "fine_8x64", {}))
    return out


def setup(cfg, rig, J, shape, dev):
    """-> (leaves, maps handed to the layer, meta, grid size, centres, cube, sample_of, gradient)"""
    img, hm = [int(v) for v in cfg.NETWORK.IMAGE_SIZE], [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]
    V = int(cfg.DATASET.CAMERA_NUM)
    center = tuple(float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER)
    B = 1 if shape == "root_B1" else 4
    meta = syn.make_meta(B, V, img, rig=rig, target=center) if rig else syn.make_meta(B, V, img)
    full = max(J, 15)
    leaves = [x.to(dev).to(BF).requires_grad_(True) for x in syn.random_heatmaps(B, V, full, hm[1], hm[0], seed=70 + B)]
    maps = [a[:, CH:CH + 1] for a in leaves] if J == 1 else leaves
    if shape.startswith("root"):
        P, cube, grid, centers, so = B, ROOT_CUBE, [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE], [list(center)], None
    else:
        rng = np.random.default_rng(8)
        gc = np.asarray(center) + rng.uniform(-1500, 1500, (8, 3)) * np.array([1, 1, 0.2])
        P, cube, grid = 8, FINE_CUBE, [float(v) for v in syn.FINE_GRID_SIZE]
        centers, so = torch.from_numpy(gc.astype(np.float32)).to(dev), torch.tensor([0, 0, 1, 2, 2, 3, 3, 1], dtype=torch.int32, device=dev)
    grad = torch.rand((P, J) + cube, generator=torch.Generator().manual_seed(11)).to(dev) + 0.5
    return leaves, maps, meta, grid, centers, list(cube), so, grad, dict(V=V, heatmap=hm, B=B, cubes=P, cube=list(cube), joints=J)


def measure(cfg, rig, J, shape, switches, deterministic, dev, args):
    leaves, maps, meta, grid, centers, cube, so, grad, what = setup(cfg, rig, J, shape, dev)
    last = {}

    def leg(on):
        layer = ProjectLayer(cfg)
        layer.bf16_train, layer.deterministic_backward = on, deterministic
        for k, v in switches.items():
            setattr(layer, k, v)

        def run():
            for a in leaves:
                a.grad = None
            clear_pack_cache()
            cubes, _ = layer.get_voxel(maps, meta, grid, centers, cube, want_grids=False, sample_of=so)
            cubes.backward(grad)
            last[on] = cubes
        return run
    off, on = leg(False), leg(True)
    names = ["off", "on", "off_again", "on_again", "off_again2", "on_again2"]
    ts = timed_legs([off, on, off, on, off, on], args.iters, args.warmup, args.block)
    r = {n: stats(t) for n, t in zip(names, ts)}
    offs, ons = [r[n] for n in names[0::2]], [r[n] for n in names[1::2]]
    spread = max(aa_spread(*offs), aa_spread(*ons))
    off_median = float(np.median([x["median_us"] for x in offs]))
    on_slowest = max(x["median_us"] for x in ons)
    r.update(shape=what, aa_spread_us=spread, off_median_us=off_median, on_median_us=float(np.median([x["median_us"] for x in ons])),
             on_slowest_us=on_slowest, speedup=off_median / on_slowest, faster_by_more_than_spread=bool(on_slowest + spread < off_median))
    # the same results either way: cubes, and with the deterministic scatter the gradient bits
    off()
    c, g = last[False].detach().clone(), [a.grad.clone() for a in leaves]
    on()
    r["cubes_equal"] = bool(torch.equal(torch.nan_to_num(c), torch.nan_to_num(last[True].detach())))
    r["gradient_dtype"] = str(leaves[0].grad.dtype)
    d = max(float((a.grad.float() - b.float()).abs().max()) for a, b in zip(leaves, g))
    r["max_gradient_difference"] = d
    r["gradients_equal"] = bool(d == 0.0)
    r["gradient_nonzero_pixels"] = int(sum(int(torch.count_nonzero(a.grad)) for a in leaves))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--legs", default="", help="comma-separated keys (default: every leg)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_bf16_train.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"what": __doc__.strip().split("\n")[0], "device": torch.cuda.get_device_name(0), "iters": args.iters, "block": args.block,
           "rule": "default on only if the slowest switched-on repeat + spread < the switched-off median in every leg",
           "switch": "ProjectLayer.bf16_train / SP3D_BF16_TRAIN stays off whatever this file says; a later change flips it by the rule",
           "legs": {}}
    want = [k for k in args.legs.split(",") if k]
    for key, yaml, rig, J, shape, switches in legs():
        if want and key not in want:
            continue
        cfg = load_config(yaml)
        for scatter, det in (("fp32", False), ("deterministic", True)):
            res["legs"][f"{key}_{scatter}"] = r = measure(cfg, rig, J, shape, switches, det, dev, args)
            print(json.dumps({f"{key}_{scatter}": {k: round(r[k], 1) for k in ("off_median_us", "on_median_us", "on_slowest_us", "aa_spread_us")},
                              "rule": r["faster_by_more_than_spread"], "equal": [r["cubes_equal"], r["gradients_equal"]]}), flush=True)
    rows = res["legs"].values()
    res["rule_met_in_every_leg"] = bool(all(r["faster_by_more_than_spread"] for r in rows))
    res["cubes_equal_in_every_leg"] = bool(all(r["cubes_equal"] for r in rows))
    res["deterministic_gradients_equal_in_every_leg"] = bool(all(r["gradients_equal"] for k, r in res["legs"].items() if k.endswith("_deterministic")))
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("rule met in every leg:", res["rule_met_in_every_leg"], "| cubes equal:", res["cubes_equal_in_every_leg"],
          "| deterministic gradients equal:", res["deterministic_gradients_equal_in_every_leg"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
