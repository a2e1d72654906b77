#!/usr/bin/env python3
"""ROOTNET_ROOTHM root net: the one-channel z-spectrum front (SP3D_ONE_FRONT) against the routes it replaces.

Shapes of configs/cam5_posenet.yaml (5 x 240x128 heat-maps, root channel 2 of 15, root grid 80x80x20, channels-last conv
stack), B = 1 and B = 4, for both hand-overs (a list of planar (B,15,h,w) tensors; views of the backbone's channels-last
(V,B,h,w,16) buffer):
  (a) root_front   from the heat-maps handed over to the input of the first 3x3x3 layer (unprojection + opening 7x7x7 conv with
                   its folded BatchNorm and ReLU), three ways -
                     default      slice copies + re-tiling pass to Jp = 4 + packed kernel -> channels-last 4-channel cubes ->
                                  _front_fft (copy into the padded buffer, the library's 3-D real transforms, contraction, crop)
                     one_channel  the same with ProjectLayer.one_channel (SP3D_ONE_CHANNEL=1): one unprojection launch
                     one_front    get_voxel_zspectrum (one launch, no cubes) -> _front_zspectrum (plane transforms, contraction,
                                  inverse planes, inverse z-DFT + shift + ReLU)
                   the new leg three times in every alternation: the largest difference between the medians of its repeats is
                   the run-to-run spread, and the rule is applied to its slowest repeat
  (b) root_graph   the graphed root-net forward (GraphedRootNet), switch off vs on (on three times), and the largest difference
                   of the root cubes relative to their range; proposals compared with torch.equal
Device events, warm-up first, then --iters timed calls per leg; the legs alternate in blocks of --block calls inside one
process.

    python tools/bench_roothm_front.py [--iters 300] [--out profiles/r21_roothm_front.json]
    rocprofv3 --kernel-trace --stats -- python tools/bench_roothm_front.py --iters 50 --legs a --out /dev/null
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_roothm import aa_spread, stats, timed_legs  # noqa: E402
from selfpose3d_amd import _lib, synthetic as syn  # noqa: E402
from selfpose3d_amd.config import load_config  # noqa: E402
from selfpose3d_amd.project_layer import ProjectLayer, nhwc_heatmap_views  # noqa: E402
from selfpose3d_amd.v2v_net import TiledZSpectrum  # noqa: E402

YAML = os.path.join(ROOT, "configs", "cam5_posenet.yaml")
NEW = ("one_front", "one_front_again", "one_front_again2")


def hand_overs(dev, cfg, B, seed):
    w, h = (int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    V, J = int(cfg.DATASET.CAMERA_NUM), int(cfg.NETWORK.NUM_JOINTS)
    planar = [x.to(dev) for x in syn.random_heatmaps(B, V, J, h, w, seed=seed)]
    return {"planar": planar, "nhwc": nhwc_heatmap_views(_lib.pack_heatmaps(planar, jp=16), J)}


def leg_a(cfg, net, dev, B, full, args):
    img, cube = [int(v) for v in cfg.NETWORK.IMAGE_SIZE], [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE]
    space, center = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE], [[float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER]]
    meta = syn.make_meta(B, len(full), img)
    ch = int(net.root_id)
    layers = {"default": ProjectLayer(cfg), "one_channel": ProjectLayer(cfg), "one_front": ProjectLayer(cfg)}
    layers["default"].one_channel, layers["one_channel"].one_channel, layers["one_front"].one_zspectrum = False, True, True
    plan = net.v2v_net._get_plan()
    plan._ensure_built()
    w0, s0 = plan.layers["front"][:2]
    sl = lambda: [a[:, ch:ch + 1] for a in full]

    def cubes_route(layer):
        x, _ = layer.get_voxel(sl(), meta, space, center, cube, want_grids=False, pad_channels=True, channels_last=True)
        return plan._front_fft(x, w0, s0)

    def spectrum_route():
        spec = layers["one_front"].get_voxel_zspectrum(sl(), meta, space, center, cube, 28)
        return plan._front_zspectrum(TiledZSpectrum(spec, *cube, 28), w0, s0)
    legs = {"default": lambda: cubes_route(layers["default"]), "one_channel": lambda: cubes_route(layers["one_channel"]),
            "one_front": spectrum_route}
    with torch.no_grad():
        names = list(legs) + list(NEW[1:])
        fns = [legs[n] for n in legs] + [spectrum_route] * 2
        ts = timed_legs(fns, args.iters, args.warmup, args.block)
        r = {n: stats(t) for n, t in zip(names, ts)}
        r["aa_spread_us"] = aa_spread(*(r[n] for n in NEW))
        new = max(r[n]["median_us"] for n in NEW)
        r["speedup_vs_default"] = r["default"]["median_us"] / new
        r["speedup_vs_one_channel"] = r["one_channel"]["median_us"] / new
        r["not_slower_than_either"] = bool(new <= min(r["default"]["median_us"], r["one_channel"]["median_us"]) + r["aa_spread_us"])
        a, b, c = legs["default"]().clone(), legs["one_channel"]().clone(), legs["one_front"]().clone()
        r["one_channel_equals_default"] = bool(torch.equal(a, b))
        r["max_diff_over_range"] = float((c - a).abs().max()) / max(float(a.abs().max()), 1e-30)
    return r


def leg_b(net, dev, B, full, cfg, args):
    from selfpose3d_amd.graphs import GraphedRootNet
    meta = syn.make_meta(B, len(full), [int(v) for v in cfg.NETWORK.IMAGE_SIZE])
    graphs = {}
    for name, on in (("off", False), ("on", True)):
        net.project_layer.one_zspectrum = net.v2v_net.one_front = on
        graphs[name] = GraphedRootNet(net, full, meta)
    net.project_layer.one_zspectrum = net.v2v_net.one_front = False
    t_off, t_on, t_on2, t_on3 = timed_legs([graphs["off"], graphs["on"], graphs["on"], graphs["on"]], args.iters, args.warmup, args.block)
    torch.cuda.synchronize()
    o_off = [t.clone() for t in graphs["off"]()]
    o_on = [t.clone() for t in graphs["on"]()]
    r = {"off": stats(t_off), "on": stats(t_on), "on_again": stats(t_on2), "on_again2": stats(t_on3)}
    r["aa_spread_us"] = aa_spread(r["on"], r["on_again"], r["on_again2"])
    slowest = max(r[n]["median_us"] for n in ("on", "on_again", "on_again2"))
    r["slowest_on_us"] = slowest
    r["faster_by_more_than_spread"] = bool(slowest < r["off"]["median_us"] - r["aa_spread_us"])
    r["max_diff_over_range"] = float((o_on[0] - o_off[0]).abs().max()) / max(float(o_off[0].abs().max()), 1e-30)
    r["proposals_equal"] = bool(torch.equal(o_on[1][..., :4], o_off[1][..., :4]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_roothm_front.json"))
    args = ap.parse_args()
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    dev = torch.device("cuda:0")
    cfg = load_config(YAML)
    torch.manual_seed(0)
    net = CuboidProposalNet(cfg)
    syn.fill_parameters_deterministic(net, seed=5, scale=0.05)
    net.eval().to(dev).use_channels_last(True)
    res = {"what": __doc__.strip().split("\n")[0], "device": torch.cuda.get_device_name(0), "iters": args.iters, "block": args.block,
           "config": "configs/cam5_posenet.yaml", "channels_last": True, "root_front": {}, "root_graph": {}}
    for B in (int(b) for b in args.batches.split(",")):
        for hand, full in hand_overs(dev, cfg, B, 70 + B).items():
            key = f"B{B}_{hand}"
            with torch.no_grad():
                net(full, syn.make_meta(B, len(full), [int(v) for v in cfg.NETWORK.IMAGE_SIZE]))     # builds the inference plan
            if "a" in args.legs:
                res["root_front"][key] = r = leg_a(cfg, net, dev, B, full, args)
                print(json.dumps({key: {k: round(v["median_us"], 2) for k, v in r.items() if isinstance(v, dict)}}), flush=True)
            if "b" in args.legs:
                res["root_graph"][key] = r = leg_b(net, dev, B, full, cfg, args)
                print(json.dumps({key + "_graph": {k: round(v["median_us"], 2) for k, v in r.items() if isinstance(v, dict)}}), flush=True)
    # the flip rule of DESIGN.md §4.2a: the graphed forward faster by more than the spread at every batch size and hand-over,
    # and no root-front leg slower
    if res["root_front"] and res["root_graph"]:
        res["flip_rule_holds"] = bool(all(r["faster_by_more_than_spread"] for r in res["root_graph"].values())
                                      and all(r["not_slower_than_either"] for r in res["root_front"].values()))
        print("flip rule holds:", res["flip_rule_holds"])
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
