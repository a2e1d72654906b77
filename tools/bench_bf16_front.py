#!/usr/bin/env python3
"""bf16 heat-maps through the fused fronts (SP3D_HM_BF16_IN, use_bf16_heatmaps()) against fp32 heat-maps, same nets.

One process, device events, the fp32 and the bf16 leg alternating in blocks of --block calls, three repeats of each in every
alternation: the largest difference between the medians of a leg's repeats is its run-to-run spread.
  (a) root_graph   the graphed root-net forward (GraphedRootNet) at B = 1 and B = 4, heat-maps handed over as views of the
                   backbone's channels-last buffer, fp32 (V,B,h,w,Jp) vs bf16 (V,B,h,w,Jp) under use_bf16_heatmaps():
                     cam5_roothm   configs/cam5_posenet.yaml (ROOTNET_ROOTHM, 15 joints) with SP3D_ONE_FRONT on
                     cam5_15       the same shapes with ROOTNET_ROOTHM off: the 15-joint z-spectrum front
                     campus17      configs/campus_synthetic_coco17_cam3.yaml with SP3D_WIDE_FRONT on
                     shelf17       configs/shelf_synthetic_coco17_cam5.yaml with SP3D_WIDE_FRONT on
                   accuracy: the bf16 run against the fp32 run on the widened maps (bit-equal by construction: recorded as a
                   boolean) and against the fp32 run on the maps before rounding (largest difference of the root cubes over
                   their range; proposals compared with torch.equal)
  (b) pose_stage   ProjectLayer.get_voxel of eight 64^3 person cubes (cam5 shapes, B = 4, two cubes per sample), fp32 cubes
                   from fp32 vs bf16 pixels; largest cube difference against the maps before rounding next to the derived
                   bound 2^-8 max |hm|
  (c) cast         the backbone's hand-over cast alone: (V,B,h,w,16) fp32 -> bf16, one torch pass (B = 1 and B = 4)
and the bytes of the heat-map buffer in both types.  Nothing here asserts a speed-up: the feature is storage and capability.

    python tools/bench_bf16_front.py [--iters 300] [--out profiles/r24_bf16_front.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_roothm import aa_spread, stats, timed_legs  # noqa: E402
from selfpose3d_amd import _lib, synthetic as syn  # noqa: E402
from selfpose3d_amd.config import load_config  # noqa: E402
from selfpose3d_amd.project_layer import ProjectLayer, nhwc_heatmap_views  # noqa: E402

CONFIGS = {"cam5_roothm": ("cam5_posenet.yaml", {}, "one"), "cam5_15": ("cam5_posenet.yaml", {"NETWORK__ROOTNET_ROOTHM": False}, None),
           "campus17": ("campus_synthetic_coco17_cam3.yaml", {}, "wide"), "shelf17": ("shelf_synthetic_coco17_cam5.yaml", {}, "wide")}
REPEATS = ("", "_again", "_again2")


def buffers(dev, cfg, B, seed):
    """the backbone's hand-over in three forms: fp32 before rounding, bf16, and the bf16 values widened to fp32"""
    w, h = (int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    V, J = int(cfg.DATASET.CAMERA_NUM), int(cfg.NETWORK.NUM_JOINTS)
    jp = ProjectLayer.jp_for(J)
    raw = _lib.pack_heatmaps([x.to(dev) for x in syn.random_heatmaps(B, V, J, h, w, seed=seed)], jp=jp)
    bf = raw.to(torch.bfloat16)
    return J, raw, bf, bf.float()


def meta_for(cfg, B):
    """the cameras of the configuration's synthetic rig, collated as a loader would"""
    from selfpose3d_amd.synthetic_dataset import SyntheticPanoptic
    from torch.utils.data import default_collate
    ds = SyntheticPanoptic(cfg, num_frames=B, seed=5, images=False)
    items = [ds[i] for i in range(B)]
    return [default_collate([it[4][v] for it in items]) for v in range(int(cfg.DATASET.CAMERA_NUM))]


def three(legs, args):
    """{name: fn} -> the legs alternating, each three times: stats per repeat, the spread and the slowest median per leg"""
    names = [n + r for r in REPEATS for n in legs]
    ts = timed_legs([legs[n] for _ in REPEATS for n in legs], args.iters, args.warmup, args.block)
    r = {n: stats(t) for n, t in zip(names, ts)}
    for n in legs:
        r[n + "_spread_us"] = aa_spread(*(r[n + x] for x in REPEATS))
        r[n + "_slowest_us"] = max(r[n + x]["median_us"] for x in REPEATS)
    return r


def root_graph(name, dev, B, args):
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.graphs import GraphedRootNet
    yaml, over, switch = CONFIGS[name]
    cfg = load_config(os.path.join(ROOT, "configs", yaml), **over)
    net = CuboidProposalNet(cfg)
    syn.fill_parameters_deterministic(net, seed=5, scale=0.05)
    net.eval().to(dev).use_channels_last(True)
    if switch == "one":
        net.project_layer.one_zspectrum = net.v2v_net.one_front = True
    if switch == "wide":
        net.project_layer.wide_zspectrum = net.v2v_net.wide_front = True
    J, raw, bf, wide = buffers(dev, cfg, B, 70 + B)
    meta = meta_for(cfg, B)
    with torch.no_grad():
        o_raw = [t.clone() for t in net(nhwc_heatmap_views(raw, J), meta)]
        o_wide = [t.clone() for t in net(nhwc_heatmap_views(wide, J), meta)]
    g32 = GraphedRootNet(net, nhwc_heatmap_views(raw, J), meta)
    net.use_bf16_heatmaps(True)
    g16 = GraphedRootNet(net, nhwc_heatmap_views(bf, J), meta)
    net.use_bf16_heatmaps(False)
    r = three({"fp32": g32, "bf16": g16}, args)
    torch.cuda.synchronize()
    o16 = [t.clone() for t in g16()]
    torch.cuda.synchronize()
    rng = max(float(o_raw[0].abs().max()), 1e-30)
    r["heatmap_bytes"] = {"fp32": raw.numel() * 4, "bf16": bf.numel() * 2}
    r["bit_equal_to_fp32_on_widened_maps"] = bool(torch.equal(o16[0], o_wide[0]) and torch.equal(o16[1], o_wide[1]))
    r["max_diff_over_range_vs_unrounded"] = float((o16[0] - o_raw[0]).abs().max()) / rng
    r["proposals_equal_to_unrounded"] = bool(torch.equal(o16[1][..., :4], o_raw[1][..., :4]))
    return r


def pose_stage(dev, args):
    cfg = load_config(os.path.join(ROOT, "configs", "cam5_posenet.yaml"))
    B, P = 4, 8
    J, raw, bf, wide = buffers(dev, cfg, B, 81)
    meta = meta_for(cfg, B)
    grid, cube = [float(v) for v in cfg.PICT_STRUCT.GRID_SIZE], [64, 64, 64]
    centers = torch.zeros(P, 5, device=dev)
    centers[:, :3] = torch.tensor([float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER], device=dev) + \
        300.0 * torch.randn(P, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    sample_of = torch.arange(P, device=dev) % B
    layers = {"fp32": ProjectLayer(cfg), "bf16": ProjectLayer(cfg)}
    layers["bf16"].bf16_maps = True
    views = {"fp32": nhwc_heatmap_views(raw, J), "bf16": nhwc_heatmap_views(bf, J)}
    run = lambda n, v=None: layers[n].get_voxel(v or views[n], meta, grid, centers, cube, want_grids=False, sample_of=sample_of)[0]
    with torch.no_grad():
        r = three({n: (lambda n=n: run(n)) for n in layers}, args)
        a, b, c = run("bf16"), run("fp32", nhwc_heatmap_views(wide, J)), run("fp32")
        r["heatmap_bytes"] = {"fp32": raw.numel() * 4, "bf16": bf.numel() * 2}
        r["bit_equal_to_fp32_on_widened_maps"] = bool(torch.equal(a, b))
        r["max_cube_diff_vs_unrounded"] = float((a - c).abs().max())
        r["derived_bound"] = 2.0 ** -8 * float(raw.abs().max())
    return r


def cast(dev, B, args):
    cfg = load_config(os.path.join(ROOT, "configs", "cam5_posenet.yaml"))
    _, raw, _, _ = buffers(dev, cfg, B, 90 + B)
    r = three({"to_bf16": lambda: raw.to(torch.bfloat16)}, args)
    r["bytes_read"], r["bytes_written"] = raw.numel() * 4, raw.numel() * 2
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_bf16_front.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"what": __doc__.strip().split("\n")[0], "device": torch.cuda.get_device_name(0), "iters": args.iters, "block": args.block,
           "root_graph": {}, "pose_stage": {}, "cast": {}}
    brief = lambda r: {k: round(v["median_us"], 2) for k, v in r.items() if isinstance(v, dict) and "median_us" in v}
    for B in (int(b) for b in args.batches.split(",")):
        if "a" in args.legs:
            for name in CONFIGS:
                res["root_graph"][f"{name}_B{B}"] = r = root_graph(name, dev, B, args)
                print(json.dumps({f"{name}_B{B}": brief(r)}), flush=True)
        if "c" in args.legs:
            res["cast"][f"B{B}"] = r = cast(dev, B, args)
            print(json.dumps({f"cast_B{B}": brief(r)}), flush=True)
    if "b" in args.legs:
        res["pose_stage"]["B4_P8_64cubed"] = r = pose_stage(dev, args)
        print(json.dumps({"pose_stage": brief(r)}), flush=True)
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
