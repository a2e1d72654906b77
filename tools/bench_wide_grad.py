#!/usr/bin/env python3
"""17 joints WITH a heat-map gradient: the channels-last training pair (ProjectLayer.wide_grad) against the planar path it replaces.

Campus (3 views, 200x160 maps) and Shelf (5 views, 200x152 maps) from their YAMLs, J = 17, three grids each: the root grid
80x80x20 at B = 1 and B = 4, and eight 64^3 person cubes (2 m edge) over B = 4 samples, for both hand-overs (a list of planar
(B,17,h,w) tensors; views of a channels-last (V,B,h,w,32) buffer).  One call = forward to planar (P,17,X,Y,Z) cubes +
backward from a (P,17,X,Y,Z) gradient, four ways:
  planar        today's path: sp3d_unproject_fwd_indexed on the planar maps + sp3d_unproject_bwd_indexed, which re-reads the
                maps (channels-last hand-over: V contiguous copies of the views first, as the module makes them)
  wide_auto     re-tiling pass to Jp = 32 (planar hand-over only) + sp3d_unproject_fwd_train with SP3D_HM_WIDE_MASK +
                sp3d_unproject_bwd_packed with SP3D_SCATTER_WIDE, SCATTER_AUTO (zero-filled (V,B,h,w,32) buffer, views back)
  wide_per_tap  the same with SCATTER_PER_TAP
  wide_det      the same through sp3d_unproject_bwd_packed_det + sp3d_fixed_to_float (SCATTER_AUTO)
What autograd does with the returned gradients follows every leg alike and is left out.
The new leg (wide_auto) runs three times in every alternation: the largest difference between the medians of its repeats is
the run-to-run spread, and the rule for a later flip of the default is applied to its slowest repeat:
below planar by more than the spread, in every leg.  Device events, warm-up first, then --iters timed calls per leg in
alternating blocks of --block calls inside one process.

    python tools/bench_wide_grad.py [--iters 300] [--out profiles/r14_wide_grad.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from selfpose3d_amd import _lib, synthetic as syn  # noqa: E402
from selfpose3d_amd.config import load_config  # noqa: E402
from selfpose3d_amd.project_layer import ProjectLayer, nhwc_heatmap_views  # noqa: E402
from tools.bench_roothm import aa_spread, stats, timed_legs  # noqa: E402

J, JP = 17, 32
YAML = {"campus_synthetic": os.path.join(ROOT, "configs", "campus_synthetic_coco17_cam3.yaml"),
        "shelf_synthetic": os.path.join(ROOT, "configs", "shelf_synthetic_coco17_cam5.yaml")}
ROOT_CUBE, FINE_CUBE = (80, 80, 20), (64, 64, 64)
REPEATS = ("wide_auto", "wide_auto_again", "wide_auto_again2")


def grid_setup(cfg, rig, shape, dev):
    """-> dict(B, P, cube, grid_size, centers (P,3), valid (P), sample_of | None, cam) of one of the three grids"""
    img = [int(v) for v in cfg.NETWORK.IMAGE_SIZE]
    center = tuple(float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER)
    B = 1 if shape == "root_B1" else 4
    layer = ProjectLayer(cfg)
    meta = syn.make_meta(B, int(cfg.DATASET.CAMERA_NUM), img, rig=rig, target=center)
    cam = layer.camera_table(meta, B, None, dev)
    if shape.startswith("root"):
        cen, val = layer.centers_valid([list(center)], B, dev)
        return dict(B=B, P=B, cube=ROOT_CUBE, grid_size=[float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE], centers=cen, valid=val,
                    sample_of=None, cam=cam, img=img)
    rng = np.random.default_rng(8)
    gc = np.asarray(center) + rng.uniform(-1500, 1500, (8, 3)) * np.array([1, 1, 0.2])
    so = torch.tensor([0, 0, 1, 2, 2, 3, 3, 1], dtype=torch.int32, device=dev)
    return dict(B=B, P=8, cube=FINE_CUBE, grid_size=[float(v) for v in syn.FINE_GRID_SIZE], sample_of=so, cam=cam, img=img,
                centers=torch.from_numpy(gc.astype(np.float32)).to(dev), valid=torch.ones(8, dtype=torch.uint8, device=dev))


def legs_of(g, hms, dev, channels_last_source):
    """the four ways as callables -> list[V] of (B,17,h,w) gradients; the cubes of the last forward in `last`"""
    V = len(hms)
    B, P, cube = g["B"], g["P"], g["cube"]
    h, w = int(hms[0].shape[2]), int(hms[0].shape[3])
    N = cube[0] * cube[1] * cube[2]
    grad = torch.randn((P, J) + tuple(cube), generator=torch.Generator().manual_seed(11)).to(dev)
    geo = (cube, g["grid_size"], g["img"])
    source = hms[0]._sp3d_packed[0] if channels_last_source else None
    last = {}

    def planar():
        maps = [x.contiguous() for x in hms]                    # a copy for views of the channels-last buffer, nothing for planar maps
        last["cubes"] = _lib.unproject_fwd(maps, _lib.LAYOUT_PLANAR, 0, g["cam"], g["centers"], g["valid"], P, J, h, w, *geo, False,
                                           sample_of=g["sample_of"])[0]
        return _lib.unproject_bwd(maps, g["cam"], g["centers"], g["valid"], grad, *geo, sample_of=g["sample_of"])

    def wide(scatter, deterministic=False):
        def run():
            pk = source if source is not None else _lib.pack_heatmaps(hms, jp=JP)
            mask = torch.empty((2, P, N), dtype=torch.int16, device=dev)
            last["cubes"] = _lib.unproject_fwd([pk[c] for c in range(V)], _lib.LAYOUT_NHWC, JP, g["cam"], g["centers"], g["valid"], P, J,
                                               h, w, *geo, False, sample_of=g["sample_of"], pass_mask=mask, wide_mask=True)[0]
            return _lib.unproject_bwd_packed(g["cam"], g["centers"], g["valid"], grad, mask, B, V, J, JP, h, w, *geo,
                                             sample_of=g["sample_of"], deterministic=deterministic, scatter=scatter, wide=True)
        return run
    return {"planar": planar, "wide_auto": wide(_lib.SCATTER_AUTO), "wide_per_tap": wide(_lib.SCATTER_PER_TAP),
            "wide_det": wide(_lib.SCATTER_AUTO, True)}, last


def measure(g, hms, dev, channels_last_source, args):
    legs, last = legs_of(g, hms, dev, channels_last_source)
    names = list(legs) + list(REPEATS[1:])
    fns = [legs[n] for n in legs] + [legs["wide_auto"]] * 2
    with torch.no_grad():
        ts = timed_legs(fns, args.iters, args.warmup, args.block)
        r = {n: stats(t) for n, t in zip(names, ts)}
        aa = aa_spread(*(r[n] for n in REPEATS))
        new = max(r[n]["median_us"] for n in REPEATS)                                  # its slowest repeat
        r["aa_spread_us"] = aa
        r["speedup_vs_planar"] = r["planar"]["median_us"] / new
        r["faster_than_planar_by_more_than_spread"] = bool(new + aa < r["planar"]["median_us"])
        # the same results: the cubes (the planar kernel divides where the NHWC kernels multiply by a reciprocal: last bits),
        # the gradients (two any-order sums / a fixed-point sum of the same terms)
        gp = torch.stack([x.contiguous() for x in legs["planar"]()])
        cp = last["cubes"].clone()
        scale = max(1.0, float(gp.abs().max()))
        for nm in ("wide_auto", "wide_per_tap", "wide_det"):
            gw = torch.stack([x.contiguous() for x in legs[nm]()])
            r["max_gradient_difference_to_planar_" + nm] = float((gw - gp).abs().max())
            r["gradients_agree_" + nm] = bool(float((gw - gp).abs().max()) <= 2e-5 * scale)
        r["max_cube_difference_to_planar"] = float((last["cubes"] - cp).abs().max())
        r["gradient_nonzero_pixels"] = int(torch.count_nonzero(gp))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--rigs", default="campus_synthetic,shelf_synthetic")
    ap.add_argument("--shapes", default="root_B1,root_B4,fine_8x64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_wide_grad.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"what": __doc__.strip().split("\n")[0], "device": torch.cuda.get_device_name(0), "iters": args.iters, "block": args.block,
           "joints": J, "rule": "default on only if the new leg's slowest repeat + spread < planar in every leg",
           "switch": "ProjectLayer.wide_grad / SP3D_WIDE_GRAD stays off whatever this file says; a later change flips it by the rule",
           "legs": {}}
    for rig in args.rigs.split(","):
        cfg = load_config(YAML[rig])
        hm = [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]
        V = int(cfg.DATASET.CAMERA_NUM)
        for shape in args.shapes.split(","):
            g = grid_setup(cfg, rig, shape, dev)
            planar = [x.to(dev) for x in syn.random_heatmaps(g["B"], V, J, hm[1], hm[0], seed=70 + g["B"])]
            hands = {"planar": planar, "nhwc": nhwc_heatmap_views(_lib.pack_heatmaps(planar, jp=JP), J)}
            for hand, hms in hands.items():
                key = f"{rig}_{shape}_{hand}"
                res["legs"][key] = r = measure(g, hms, dev, hand == "nhwc", args)
                r["shape"] = {"V": V, "heatmap": hm, "B": g["B"], "cubes": g["P"], "cube": list(g["cube"])}
                print(json.dumps({key: {k: round(v["median_us"], 1) for k, v in r.items() if isinstance(v, dict) and "median_us" in v},
                                  "spread_us": round(r["aa_spread_us"], 1), "rule": r["faster_than_planar_by_more_than_spread"]}), flush=True)
    legs = res["legs"].values()
    res["rule_met_in_every_leg"] = bool(all(r["faster_than_planar_by_more_than_spread"] for r in legs))
    res["gradients_agree_in_every_leg"] = bool(all(v for r in legs for k, v in r.items() if k.startswith("gradients_agree_")))
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("rule met in every leg:", res["rule_met_in_every_leg"], "| gradients agree:", res["gradients_agree_in_every_leg"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
