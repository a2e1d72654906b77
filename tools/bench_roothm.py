#!/usr/bin/env python3
"""ROOTNET_ROOTHM root input: one heat-map channel unprojected in place against the paths it replaces.

5 x 240x128 heat-maps, channel 2 of 15, root grid 80x80x20, B = 1 and B = 4, for both hand-overs (a list of planar
(B,15,h,w) tensors; views of the backbone's channels-last (V,B,h,w,16) buffer):
  (a) root_input   from the heat-maps handed over to cubes ready for the V2V net, three ways -
                     default_off  slice copies + re-tiling pass to Jp = 4 + pipelined kernel (ProjectLayer.one_channel = False)
                     planar       the planar kernel on contiguous slices (ProjectLayer(mode="planar")), its dense (B,1,X,Y,Z)
                                  result then padded to channels-last / copied into the buffer
                     one_channel  the one-channel kernel on the slices as they lie (one launch)
                   for the channels-last 4-channel result and for out= into the opening conv's zero-padded FFT input buffer
  (b) root_graph   the graphed ROOTNET_ROOTHM root-net forward (GraphedRootNet), switch off vs on, outputs compared with
                   torch.equal, and GraphedRootNet(time_unprojection=True).unprojection_us() of each for information (with the
                   switch off it covers the re-tiling pass and the kernel, not the slice copies in front of get_voxel)
  (aa)             the new leg three times in every alternation: the largest difference between the medians of the repeats is
                   the run-to-run spread, and the rule is applied to the slowest repeat
Device events, warm-up first, then --iters timed calls per leg; the legs alternate in blocks of --block calls inside one
process.  GB/s counts the algorithmic bytes 4 B (V h w + N) - information only, the path is latency bound.

    python tools/bench_roothm.py [--iters 300] [--out profiles/r08_roothm.json]
    rocprofv3 --kernel-trace --stats -- python tools/bench_roothm.py --iters 50 --no-launch-count --out /dev/null
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

IMG, HM, V, J, CH, CUBE = (960, 512), (240, 128), 5, 15, 2, (80, 80, 20)


def timed_legs(fns, iters, warmup, block):
    """alternating blocks of the legs, device-event timed per call: list of time arrays (us)"""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    while len(acc[0]) < iters:
        for f, a in zip(fns, acc):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(block)]
            for s, e in evs:
                s.record()
                f()
                e.record()
            torch.cuda.synchronize()
            a.extend(s.elapsed_time(e) * 1e3 for s, e in evs)
    return [np.array(a[:iters]) for a in acc]


def stats(t):
    return {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90)),
            "n": int(t.size)}


def count_launches(f):
    """device kernels + copies of one call, counted by torch's profiler (--no-launch-count leaves it out, e.g. under rocprofv3)"""
    from torch.profiler import ProfilerActivity, profile
    f()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        f()
        torch.cuda.synchronize()
    return int(sum(1 for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower()))


def aa_spread(*rs):
    """run-to-run spread of one leg measured several times in the same alternation: the largest difference between the
    medians of its repeats"""
    m = [r["median_us"] for r in rs]
    return float(max(m) - min(m))


def hand_overs(dev, B, seed):
    planar = [h.to(dev) for h in syn.random_heatmaps(B, V, J, HM[1], HM[0], seed=seed)]
    packed = _lib.pack_heatmaps(planar, jp=16)
    return {"planar": planar, "nhwc": nhwc_heatmap_views(packed, J)}


def leg_a(cfg, dev, B, full, v2v, args):
    meta = syn.make_meta(B, V, list(IMG))
    space, center = list(syn.SPACE_SIZE), [list(syn.SPACE_CENTER)]
    on, off, planar = ProjectLayer(cfg), ProjectLayer(cfg), ProjectLayer(cfg, mode="planar")
    on.one_channel, off.one_channel = True, False
    X, Y, Z = CUBE
    N = X * Y * Z
    view = v2v.input_view(B, X, Y, Z, dev) if v2v is not None else None
    if view is None:                                             # the same geometry as the opening conv's padded input
        view = torch.zeros((B, 1, 88, 88, 28), device=dev)[:, :, :X, :Y, :Z]
    sl = lambda: [a[:, CH:CH + 1] for a in full]
    slc = lambda: [a[:, CH:CH + 1].contiguous() for a in full]
    forms = {
        "channels_last4": {
            "default_off": lambda: off.get_voxel(slc(), meta, space, center, CUBE, want_grids=False, pad_channels=True, channels_last=True),
            "planar": lambda: torch.nn.functional.pad(planar.get_voxel(slc(), meta, space, center, CUBE, want_grids=False)[0],
                                                      (0, 0, 0, 0, 0, 0, 0, 3)).contiguous(memory_format=torch.channels_last_3d),
            "one_channel": lambda: on.get_voxel(sl(), meta, space, center, CUBE, want_grids=False, pad_channels=True, channels_last=True),
        },
        "out_fft_buffer": {
            "default_off": lambda: off.get_voxel(slc(), meta, space, center, CUBE, want_grids=False, out=view),
            "planar": lambda: view.copy_(planar.get_voxel(slc(), meta, space, center, CUBE, want_grids=False)[0]),
            "one_channel": lambda: on.get_voxel(sl(), meta, space, center, CUBE, want_grids=False, out=view),
        },
    }
    res = {}
    with torch.no_grad():
        for form, legs in forms.items():
            names = list(legs) + ["one_channel_again", "one_channel_again2"]
            fns = [legs[n] for n in legs] + [legs["one_channel"]] * 2
            ts = timed_legs(fns, args.iters, args.warmup, args.block)
            r = {n: stats(t) for n, t in zip(names, ts)}
            aa = aa_spread(r["one_channel"], r["one_channel_again"], r["one_channel_again2"])
            new = max(r[n]["median_us"] for n in ("one_channel", "one_channel_again", "one_channel_again2"))   # its slowest repeat
            r["aa_spread_us"] = aa
            r["algorithmic_bytes"] = 4 * B * (V * HM[0] * HM[1] + N)
            r["one_channel_GBps"] = r["algorithmic_bytes"] / (new * 1e-6) / 1e9
            r["speedup_vs_default_off"] = r["default_off"]["median_us"] / new
            r["speedup_vs_planar"] = r["planar"]["median_us"] / new
            r["faster_than_both_by_more_than_spread"] = bool(new + aa < min(r["default_off"]["median_us"], r["planar"]["median_us"]))
            if not args.no_launch_count:
                r["launches_per_call"] = {n: count_launches(legs[n]) for n in legs}
            # same bits, whichever way
            a = legs["default_off"]()
            a = (a[0] if isinstance(a, tuple) else a).clone()
            b = legs["one_channel"]()
            r["bit_identical_to_default_off"] = bool(torch.equal(a, b[0]))
            res[form] = r
    return res


def leg_b(net, dev, B, full, args):
    from selfpose3d_amd.graphs import GraphedRootNet
    meta = syn.make_meta(B, V, list(IMG))
    graphs = {}
    before = net.project_layer.one_channel
    for name, on in (("off", False), ("on", True)):
        net.project_layer.one_channel = on
        graphs[name] = GraphedRootNet(net, full, meta)
    t_off, t_on, t_on2, t_on3 = timed_legs([graphs["off"], graphs["on"], graphs["on"], graphs["on"]], args.iters, args.warmup, args.block)
    torch.cuda.synchronize()
    o_off = [t.clone() for t in graphs["off"]()]
    o_on = [t.clone() for t in graphs["on"]()]
    r = {"off": stats(t_off), "on": stats(t_on), "on_again": stats(t_on2), "on_again2": stats(t_on3)}
    r["aa_spread_us"] = aa_spread(r["on"], r["on_again"], r["on_again2"])
    r["outputs_equal"] = bool(torch.equal(o_off[0], o_on[0]) and torch.equal(o_off[1], o_on[1]))
    slowest = max(r[n]["median_us"] for n in ("on", "on_again", "on_again2"))
    r["not_slower_by_more_than_spread"] = bool(slowest <= r["off"]["median_us"] + r["aa_spread_us"])
    del graphs
    unp = {}
    for name, on in (("off", False), ("on", True)):
        net.project_layer.one_channel = on
        g = GraphedRootNet(net, full, meta, time_unprojection=True)
        vals = []
        for _ in range(20):
            g()
            vals.append(g.unprojection_us())
        unp[name] = {"get_voxel_us": float(np.median([v[0] for v in vals])), "marker_us": float(np.median([v[1] for v in vals]))}
        del g
    r["unprojection_in_step_us"] = unp
    net.project_layer.one_channel = before
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--no-launch-count", action="store_true", help="do not start torch's profiler (use under rocprofv3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_roothm.json"))
    args = ap.parse_args()
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    dev = torch.device("cuda:0")
    cfg = load_config(None, NETWORK__ROOTNET_ROOTHM=True, DATASET__ROOTIDX_PSEUDO=CH)
    torch.manual_seed(0)
    net = CuboidProposalNet(cfg).eval().to(dev)
    res = {"what": __doc__.strip().split("\n")[0], "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "block": args.block, "shape": {"V": V, "heatmap": list(HM), "channel": CH, "of": J, "cube": list(CUBE)},
           "bytes_formula": "4*B*(V*h*w + N)", "root_input": {}, "root_graph": {}}
    for B in (int(b) for b in args.batches.split(",")):
        for hand, full in hand_overs(dev, B, 70 + B).items():
            key = f"B{B}_{hand}"
            with torch.no_grad():
                net(full, syn.make_meta(B, V, list(IMG)))             # builds the inference plan and its buffers
            if "a" in args.legs:
                res["root_input"][key] = leg_a(cfg, dev, B, full, net.v2v_net, args)
                print(json.dumps({key: {f: {k: round(v["median_us"], 2) for k, v in r.items() if isinstance(v, dict) and "median_us" in v}
                                        for f, r in res["root_input"][key].items()}}), flush=True)
            if "b" in args.legs:
                res["root_graph"][key] = leg_b(net, dev, B, full, args)
                print(json.dumps({key + "_graph": {k: round(v["median_us"], 2) for k, v in res["root_graph"][key].items()
                                                   if isinstance(v, dict) and "median_us" in v}}), flush=True)
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
