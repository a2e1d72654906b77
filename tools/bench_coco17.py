#!/usr/bin/env python3
"""17-joint (COCO) unprojection on the Shelf / Campus rigs: the Jp = 32 NHWC path against the planar kernel it replaces.

For both rigs at B = 4, J = 17 (configs/campus_synthetic_coco17_cam3.yaml, configs/shelf_synthetic_coco17_cam5.yaml):
  (a) root_unproject   one root-grid (80x80x20) unprojection launch: packed maps (Jp = 32) vs the planar kernel
  (b) person_cubes     eight 64^3 person cubes through sample_of into the V2V plan's FFT input buffer vs planar cubes
  (c) root_graph       the graphed root-net forward (GraphedRootNet) with either unprojection
  (d) eval_frame       one eval frame from heat-maps: root net, then pose net on the proposals it found
  (e) root_graph_channels_last   the graphed root net after use_channels_last(True) - the configuration validate_3d.py and
                       bench.py run; (a)-(d) never call it, so their V2V stack is the planar library route - with the
                       17..32-joint z-spectrum front (SP3D_WIDE_FRONT) off and on; --legs e, profiles/r20_coco17_wide_front.json
Device events, warm-up first, then --iters timed iterations per leg; the two paths alternate in blocks of --block
iterations inside one process.  bytes/s counts the algorithmic bytes 4 B (V J h w + J N) of (a) and (b).

    python tools/bench_coco17.py [--iters 200] [--out profiles/r07_coco17.json]
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
from selfpose3d_amd.project_layer import ProjectLayer  # noqa: E402

YAML = {"campus": "configs/campus_synthetic_coco17_cam3.yaml", "shelf": "configs/shelf_synthetic_coco17_cam5.yaml"}


def timed_pair(fa, fb, iters, warmup, block):
    """alternating blocks of fa / fb, device-event timed per call: (times_a us, times_b us)"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    while len(ta) < iters:
        for f, acc in ((fa, ta), (fb, tb)):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(block)]
            for s, e in evs:
                s.record()
                f()
                e.record()
            torch.cuda.synchronize()
            acc.extend(s.elapsed_time(e) * 1e3 for s, e in evs)
    return np.array(ta[:iters]), np.array(tb[:iters])


def stats(t):
    return {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90)),
            "n": int(t.size)}


class PlanarRoot(torch.nn.Module):
    """the root net with the planar kernel's dense cubes handed to the same V2V and proposal layer (the path Jp = 32
    replaces: no hand-over into the FFT input buffer)"""

    def __init__(self, root, cfg):
        super().__init__()
        self.root = root
        self.project_layer = ProjectLayer(cfg, mode="planar")

    def forward(self, hms, meta, flip_xcoords=None):
        r = self.root
        cubes, _ = self.project_layer.get_voxel(hms, meta, r.grid_size, [r.grid_center], r.cube_size, flip_xcoords=flip_xcoords,
                                                want_grids=False)
        root_cubes = r.v2v_net(cubes).squeeze(1)
        return root_cubes, r.proposal_layer(root_cubes, meta)


def rig_inputs(name, dev, B):
    """cfg, heat-maps of synthetic people on the device, meta - what every leg of a rig runs on"""
    from selfpose3d_amd.synthetic_dataset import SyntheticPanoptic
    from torch.utils.data import default_collate
    # every proposal slot valid (random-init nets): (d) runs the pose net on B x 4 = 16 person cubes
    cfg = load_config(os.path.join(ROOT, YAML[name]), MULTI_PERSON__THRESHOLD=-1e9, MULTI_PERSON__MAX_PEOPLE_NUM=4)
    V = int(cfg.DATASET.CAMERA_NUM)
    ds = SyntheticPanoptic(cfg, num_frames=B, seed=5, images=False)
    items = [ds[i] for i in range(B)]
    hms = [torch.stack([it[1][v] for it in items]).to(dev) for v in range(V)]
    meta = [default_collate([it[4][v] for it in items]) for v in range(V)]
    return cfg, ds, hms, meta


def run_root_graph_channels_last(name, dev, iters, warmup, block, repeats=3, variant="both"):
    """(e) the graphed root net in the configuration validate_3d.py and bench.py run - use_channels_last(True), which legs
    (a)-(d) never call, so their V2V stack is the planar library route - with the 17..32-joint z-spectrum front
    (SP3D_WIDE_FRONT: ProjectLayer.wide_zspectrum + V2VNet.wide_front) off and on.  Both graphs live in one process and
    alternate in blocks (timed_pair); the pair is timed ``repeats`` times, and the largest difference between the
    switched-on medians is the run-to-run spread.  Rule for a later default flip: the slowest
    switched-on repeat is below the switched-off median by more than the spread, on both rigs."""
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.graphs import GraphedRootNet
    B = 4
    cfg, ds, hms, meta = rig_inputs(name, dev, B)
    torch.manual_seed(0)
    root = CuboidProposalNet(cfg).eval().to(dev).use_channels_last(True)
    static = [x.clone() for x in hms]

    def graphed(on):
        root.project_layer.wide_zspectrum = root.v2v_net.wide_front = on      # read while capturing
        try:
            return GraphedRootNet(root, static, meta)
        finally:
            root.project_layer.wide_zspectrum = root.v2v_net.wide_front = False
    if variant != "both":       # one graph alone, for a kernel trace of its own (rocprofv3 --kernel-trace --stats)
        g = graphed(variant == "on")
        t, _ = timed_pair(lambda: g(), lambda: g(), iters, warmup, block)
        return {"variant": variant, variant: stats(t)}
    g_off, g_on = graphed(False), graphed(True)
    a, b = g_off()[0].clone(), g_on()[0].clone()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        t_off, t_on = timed_pair(lambda: g_off(), lambda: g_on(), iters, warmup, block)
        runs.append({"off": stats(t_off), "on": stats(t_on)})
    on_med = [r["on"]["median_us"] for r in runs]
    off_med = float(np.median([r["off"]["median_us"] for r in runs]))
    spread = float(max(on_med) - min(on_med))
    return {"repeats": runs, "off_median_us": off_med, "on_medians_us": on_med, "on_spread_us": spread,
            "on_slowest_minus_off_us": float(max(on_med) - off_med),
            "on_wins_by_more_than_the_spread": bool(max(on_med) < off_med - spread),
            "root_cubes_max_abs_diff": float((a - b).abs().max()), "root_cubes_max_abs": float(a.abs().max())}


def run_rig(name, dev, iters, warmup, block):
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.graphs import GraphedRootNet
    from selfpose3d_amd.pose_regression_net import PoseRegressionNet
    from selfpose3d_amd.synthetic_dataset import SyntheticPanoptic
    from torch.utils.data import default_collate
    B, J = 4, 17
    # every proposal slot valid (random-init nets): (d) runs the pose net on B x 4 = 16 person cubes
    cfg = load_config(os.path.join(ROOT, YAML[name]), MULTI_PERSON__THRESHOLD=-1e9, MULTI_PERSON__MAX_PEOPLE_NUM=4)
    V = int(cfg.DATASET.CAMERA_NUM)
    w, h = (int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    ds = SyntheticPanoptic(cfg, num_frames=B, seed=5, images=False)
    items = [ds[i] for i in range(B)]
    hms = [torch.stack([it[1][v] for it in items]).to(dev) for v in range(V)]
    meta = [default_collate([it[4][v] for it in items]) for v in range(V)]
    space = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE]
    center = [float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER]
    root_cube = [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE]
    fine = [int(v) for v in cfg.PICT_STRUCT.CUBE_SIZE]
    out = {"V": V, "B": B, "J": J, "heatmap": [w, h], "image": list(ds.orig)}
    nhwc, planar = ProjectLayer(cfg), ProjectLayer(cfg, mode="planar")

    def gbs(us, N):
        return 4.0 * B * (V * J * h * w + J * N) / (us * 1e-6) / 1e9

    with torch.no_grad():
        # (a) the root-grid launch (NHWC: the re-tiled maps of the previous call are reused, as inside one forward)
        N = int(np.prod(root_cube))
        fa = lambda: nhwc.get_voxel(hms, meta, space, [center], root_cube, want_grids=False)
        fb = lambda: planar.get_voxel(hms, meta, space, [center], root_cube, want_grids=False)
        ta, tb = timed_pair(fa, fb, iters, warmup, block)
        out["a_root_unproject"] = {"nhwc_jp32": stats(ta), "planar": stats(tb),
                                   "nhwc_GBps": gbs(np.median(ta), N), "planar_GBps": gbs(np.median(tb), N),
                                   "speedup": float(np.median(tb) / np.median(ta))}
        # (b) eight 64^3 person cubes through sample_of into the plan's FFT input buffer
        torch.manual_seed(0)
        pose = PoseRegressionNet(cfg).eval().to(dev)
        P = 8
        rng = np.random.default_rng(1)
        gc = np.zeros((P, 5), np.float32)
        gc[:, :3] = np.asarray(center) + rng.uniform(-1500, 1500, (P, 3)) * np.array([1, 1, 0.2])
        gct = torch.from_numpy(gc).to(dev)
        sample_of = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3], dtype=torch.int32, device=dev)
        pose.v2v_net(torch.zeros((P, J, *fine), device=dev))            # builds the inference plan and its buffers
        whole, _ = pose.v2v_net.input_chunk_views(P, P, *fine, dev)
        N = int(np.prod(fine))
        fa = lambda: nhwc.get_voxel(hms, meta, syn.FINE_GRID_SIZE, gct, fine, want_grids=False, sample_of=sample_of, out=whole)
        fb = lambda: planar.get_voxel(hms, meta, syn.FINE_GRID_SIZE, gct, fine, want_grids=False, sample_of=sample_of)
        ta, tb = timed_pair(fa, fb, iters, warmup, block)
        out["b_person_cubes_8x64cube"] = {"nhwc_jp32_into_fft_buffer": stats(ta), "planar_dense": stats(tb),
                                          "nhwc_GBps": gbs(np.median(ta), N * P / B), "planar_GBps": gbs(np.median(tb), N * P / B),
                                          "speedup": float(np.median(tb) / np.median(ta))}
        # (c) graphed root-net forward
        torch.manual_seed(0)
        root = CuboidProposalNet(cfg).eval().to(dev)
    static = [x.clone() for x in hms]
    g_n = GraphedRootNet(root, static, meta)
    g_p = GraphedRootNet(PlanarRoot(root, cfg), static, meta)
    ta, tb = timed_pair(lambda: g_n(), lambda: g_p(), iters, warmup, block)
    torch.cuda.synchronize()
    same = bool(torch.equal(g_n()[0].clone(), g_p()[0].clone()))
    out["c_root_graph"] = {"nhwc_jp32": stats(ta), "planar": stats(tb), "speedup": float(np.median(tb) / np.median(ta)),
                           "root_cubes_bit_identical": same}
    del g_n, g_p
    # (d) one eval frame from heat-maps: root net, then pose net on the proposals found
    pose_p = PoseRegressionNet(cfg).eval().to(dev)
    pose_p.load_state_dict(pose.state_dict())
    pose_p.project_layer.mode = "planar"
    root_p = PlanarRoot(root, cfg)

    def frame(rn, pn):
        def f():
            _, centers = rn(hms, meta)
            return pn.forward_batched(hms, meta, centers)
        return f
    with torch.no_grad():
        n_prop = int((root(hms, meta)[1][:, :, 3] >= 0).sum())
        ta, tb = timed_pair(frame(root, pose), frame(root_p, pose_p), max(iters // 4, 50), warmup, max(block // 4, 5))
    out["d_eval_frame"] = {"nhwc_jp32": stats(ta), "planar": stats(tb), "speedup": float(np.median(tb) / np.median(ta)),
                           "proposals": n_prop}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--rigs", default="campus,shelf")
    ap.add_argument("--legs", default="abcd,e", help="'abcd' (legs a-d), 'e' (the channels-last root graph), or both")
    ap.add_argument("--e-variant", choices=["both", "off", "on"], default="both",
                    help="leg e: 'off' / 'on' replays that graph alone (for a kernel trace of its own)")
    ap.add_argument("--out", default=None, help="default: profiles/r07_coco17.json with legs a-d, else profiles/r20_coco17_wide_front.json")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r07_coco17.json" if "abcd" in legs else "r20_coco17_wide_front.json")
    dev = torch.device("cuda:0")
    res = {"what": __doc__.strip().split("\n")[0], "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "bytes_formula": "4*B*(V*J*h*w + J*N)", "rigs": {}}
    for name in args.rigs.split(","):
        res["rigs"][name] = run_rig(name, dev, args.iters, args.warmup, args.block) if "abcd" in legs else {}
        print(json.dumps({name: {k: v.get("speedup") for k, v in res["rigs"][name].items() if isinstance(v, dict)}}), flush=True)
        if "e" in legs:
            e = res["rigs"][name]["e_root_graph_channels_last"] = run_root_graph_channels_last(
                name, dev, args.iters, args.warmup, args.block, variant=args.e_variant)
            print(json.dumps({name: {k: e[k] for k in ("off_median_us", "on_medians_us", "on_spread_us") if k in e}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
