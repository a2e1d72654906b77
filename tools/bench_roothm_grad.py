#!/usr/bin/env python3
"""ROOTNET_ROOTHM root input WITH a heat-map gradient: the one-channel training pair against the paths it replaces.

5 x 240x128 heat-maps, channel 2 of 15, root grid 80x80x20, B = 1 and B = 4, for both hand-overs (a list of planar
(B,15,h,w) tensors; views of the backbone's channels-last (V,B,h,w,16) buffer).  One call = forward to channels-last
(B,4,X,Y,Z) cubes + backward from a channels-last (B,4,X,Y,Z) gradient to the V (B,1,h,w) gradients of the channel, four ways:
  packed_auto     today's path: V slice copies + re-tiling pass to Jp = 4 + packed training forward (pass mask) +
                  sp3d_unproject_bwd_packed, SCATTER_AUTO (fp32 atomics, zero-filled (V,B,h,w,4) buffer, strided views back)
  packed_per_tap  the same with SCATTER_PER_TAP
  planar          the planar kernels on contiguous slices: sp3d_unproject_fwd (result padded to channels-last) +
                  sp3d_unproject_bwd, which re-reads the heat-maps
  one_channel     sp3d_unproject_one_fwd_train on the slices as they lie + sp3d_unproject_one_bwd (dense (V,B,h,w) buffer)
The zero-fill of the full (B,15,h,w) gradient by autograd's slice backward follows every leg alike and is left out.
The new leg runs three times in every alternation: the largest difference between the medians of its repeats is the
run-to-run spread, and the default rule is applied to its slowest repeat: below packed_auto AND planar by
more than the spread, in every leg.  Device events, warm-up first, then --iters timed calls per leg in alternating blocks of
--block calls inside one process.

    python tools/bench_roothm_grad.py [--iters 300] [--out profiles/r09_roothm_grad.json]
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
from selfpose3d_amd.project_layer import ProjectLayer, one_channel_source  # noqa: E402
from tools.bench_roothm import CH, CUBE, HM, IMG, V, aa_spread, hand_overs, stats, timed_legs  # noqa: E402

REPEATS = ("one_channel", "one_channel_again", "one_channel_again2")


def legs_of(cfg, dev, B, full, deterministic=False):
    """the four ways as callables -> list[V] of (B,1,h,w) gradients, and the cubes of the last forward in `last`"""
    layer = ProjectLayer(cfg)
    meta = syn.make_meta(B, V, list(IMG))
    cam = layer.camera_table(meta, B, None, dev)
    cen, val = layer.centers_valid([list(syn.SPACE_CENTER)], B, dev)
    space, img = [float(s) for s in syn.SPACE_SIZE], layer.img_size
    X, Y, Z = CUBE
    h, w = HM[1], HM[0]
    grad = torch.randn((B, X, Y, Z, 4), generator=torch.Generator().manual_seed(11)).to(dev).permute(0, 4, 1, 2, 3)
    sl = lambda: [a[:, CH:CH + 1] for a in full]
    slc = lambda: [a[:, CH:CH + 1].contiguous() for a in full]
    layout, jp = one_channel_source(sl())
    last = {}

    def packed(scatter):
        def run():
            pk = _lib.pack_heatmaps(slc(), jp=4)
            mask = torch.empty((B, X * Y * Z), dtype=torch.int16, device=dev)
            last["cubes"] = _lib.unproject_fwd([pk[c] for c in range(V)], _lib.LAYOUT_NHWC, 4, cam, cen, val, B, 4, h, w, CUBE, space,
                                               img, False, channels_last=True, pass_mask=mask)[0]
            return _lib.unproject_bwd_packed(cam, cen, val, grad, mask, B, V, 1, 4, h, w, CUBE, space, img,
                                             deterministic=deterministic, scatter=scatter)
        return run

    def planar():
        hms = slc()
        c = _lib.unproject_fwd(hms, _lib.LAYOUT_PLANAR, 0, cam, cen, val, B, 1, h, w, CUBE, space, img, False)[0]
        last["cubes"] = torch.nn.functional.pad(c, (0, 0, 0, 0, 0, 0, 0, 3)).contiguous(memory_format=torch.channels_last_3d)
        return _lib.unproject_bwd(hms, cam, cen, val, grad, CUBE, space, img)

    def one():
        mask = torch.empty((B, X * Y * Z), dtype=torch.int16, device=dev)
        last["cubes"] = _lib.unproject_one_fwd_train(sl(), layout, jp, cam, cen, val, B, 4, h, w, CUBE, space, img, mask, False,
                                                     channels_last=True)[0]
        return _lib.unproject_one_bwd(cam, cen, val, grad, mask, B, V, h, w, CUBE, space, img, deterministic=deterministic)
    return {"packed_auto": packed(_lib.SCATTER_AUTO), "packed_per_tap": packed(_lib.SCATTER_PER_TAP), "planar": planar,
            "one_channel": one}, last


def measure(cfg, dev, B, full, args):
    legs, last = legs_of(cfg, dev, B, full)
    names = list(legs) + list(REPEATS[1:])
    fns = [legs[n] for n in legs] + [legs["one_channel"]] * 2
    with torch.no_grad():
        ts = timed_legs(fns, args.iters, args.warmup, args.block)
        r = {n: stats(t) for n, t in zip(names, ts)}
        aa = aa_spread(*(r[n] for n in REPEATS))
        new = max(r[n]["median_us"] for n in REPEATS)                                  # its slowest repeat
        r["aa_spread_us"] = aa
        r["speedup_vs_packed_auto"] = r["packed_auto"]["median_us"] / new
        r["speedup_vs_planar"] = r["planar"]["median_us"] / new
        r["faster_than_both_by_more_than_spread"] = bool(new + aa < min(r["packed_auto"]["median_us"], r["planar"]["median_us"]))
        # the same results, whichever way: cubes equal, deterministic gradients bit-equal to the packed path's
        det, dlast = legs_of(cfg, dev, B, full, deterministic=True)
        a = torch.stack([g.contiguous() for g in det["packed_per_tap"]()])
        ca = dlast["cubes"].clone()
        b = torch.stack([g.contiguous() for g in det["one_channel"]()])
        r["cubes_equal_to_packed"] = bool(torch.equal(ca, dlast["cubes"]))
        r["deterministic_gradient_bit_identical_to_packed"] = bool(torch.equal(a, b))
        r["gradient_nonzero_pixels"] = int(torch.count_nonzero(b))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_roothm_grad.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = load_config(None, NETWORK__ROOTNET_ROOTHM=True, DATASET__ROOTIDX_PSEUDO=CH)
    res = {"what": __doc__.strip().split("\n")[0], "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "block": args.block, "shape": {"V": V, "heatmap": list(HM), "channel": CH, "of": 15, "cube": list(CUBE)},
           "rule": "default on only if the new leg's slowest repeat + spread < min(packed_auto, planar) in every leg",
           "root_input_grad": {}}
    for B in (int(b) for b in args.batches.split(",")):
        for hand, full in hand_overs(dev, B, 70 + B).items():
            key = f"B{B}_{hand}"
            res["root_input_grad"][key] = r = measure(cfg, dev, B, full, args)
            print(json.dumps({key: {k: round(v["median_us"], 2) for k, v in r.items() if isinstance(v, dict) and "median_us" in v},
                              "spread_us": round(r["aa_spread_us"], 2), "rule": r["faster_than_both_by_more_than_spread"]}), flush=True)
    legs = res["root_input_grad"].values()
    res["rule_met_in_every_leg"] = bool(all(r["faster_than_both_by_more_than_spread"] for r in legs))
    res["results_equal_in_every_leg"] = bool(all(r["cubes_equal_to_packed"] and r["deterministic_gradient_bit_identical_to_packed"]
                                                 for r in legs))
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("rule met in every leg:", res["rule_met_in_every_leg"], "| results equal:", res["results_equal_in_every_leg"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
