#!/usr/bin/env python3
"""17-joint golden vectors (the Shelf / Campus configurations), by RUNNING THE REFERENCE'S OWN PYTHON on CPU (build
container only; the import shims of make_goldens.py / make_goldens_r2.py, as make_goldens_r6.py uses them).

  unproj_coco17_cam3.npz   reference ProjectLayer (lib/models/project_layer.py:42-102) at J = 17 on the Campus-shape rig:
                           3 cameras of 360x288 (synthetic.RIGS["campus_synthetic"]), 800x640 network input, 200x160
                           heat-maps, U[0,1) maps.
                             small_*  B = 2, a 12x10x8 grid around two person centres (grid_center (B,5)), rotated and
                                      scaled crops, sample 1 flipped - stored whole
                             root_*   B = 2, the 80x80x20 root grid of configs/campus_synthetic_coco17_cam3.yaml, plain
                                      validation crops - every 97th voxel stored, plus float64 sums over every voxel

    python tests/golden/make_goldens_r7.py
"""
import os
import sys
import time
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore")

import make_goldens as mg        # noqa: E402
import make_goldens_r2 as mg2    # noqa: E402
from selfpose3d_amd import synthetic as syn   # noqa: E402

RIG = "campus_synthetic"
V, J = 3, 17
IMG, HM = (800, 640), (200, 160)
SPACE_SIZE, SPACE_CENTER = (12000.0, 12000.0, 2000.0), (3000.0, 4500.0, 1000.0)
ROOT_CUBE = (80, 80, 20)
ROOT_STRIDE = 97


def run(prefix, B, grid_size, grid_center, cube, seed, rotations=None, scale_mults=None, flip=None, stride=None):
    from models.project_layer import ProjectLayer
    cfg = mg.make_cfg(IMG, HM, SPACE_SIZE, SPACE_CENTER, cube, grid_size, cube, J)
    layer = ProjectLayer(cfg)
    meta = syn.make_meta(B, V, IMG, rotations=rotations, scale_mults=scale_mults, rig=RIG, target=SPACE_CENTER)
    hms = syn.random_heatmaps(B, V, J, HM[1], HM[0], seed=seed)
    gc_t = torch.from_numpy(grid_center) if isinstance(grid_center, np.ndarray) else grid_center
    flip_t = None if flip is None else torch.tensor(flip, dtype=torch.bool)
    with torch.no_grad():
        cubes, grids = layer(hms, meta, list(grid_size), gc_t, list(cube), flip_xcoords=flip_t)
    c, g = cubes.numpy(), grids.numpy()
    N = cube[0] * cube[1] * cube[2]
    rec = {"B": B, "grid_size": np.array(grid_size, np.float64), "cube": np.array(cube), "seed": seed,
           "grid_center": np.asarray(grid_center, np.float64), "center_is_list": isinstance(grid_center, list),
           "rotations": np.array([] if rotations is None else rotations, np.float64),
           "scale_mults": np.array([] if scale_mults is None else scale_mults, np.float64),
           "flip": np.array([] if flip is None else flip, bool),
           "cubes_sum": np.float64(c.astype(np.float64).sum()),
           "cubes_sum_per_joint": c.astype(np.float64).sum(axis=(0, 2, 3, 4)),
           "cubes_sum_per_sample_joint": c.astype(np.float64).sum(axis=(2, 3, 4)),
           "grids_sum": g.astype(np.float64).sum(axis=(0, 1))}
    if stride is None:
        rec.update(cubes=c, grids=g)
    else:
        idx = np.arange(0, N, stride)
        rec.update(sub_idx=idx, cubes_sub=c.reshape(B, J, N)[:, :, idx], grids_sub=g[:, idx])
    print(f"{prefix}: cubes {c.shape}, non-zero {int((c != 0).sum())} of {c.size}")
    return {prefix + k: v for k, v in rec.items()}


def main():
    t0 = time.time()
    rec = {"rig": RIG, "V": V, "J": J, "img": np.array(IMG), "hm": np.array(HM),
           "space_size": np.array(SPACE_SIZE), "space_center": np.array(SPACE_CENTER)}
    gc = np.array([[3300.0, 4100.0, 900.0, 0.0, 0.9],
                   [2500.0, 5200.0, 1100.0, 1.0, 0.6]], np.float32)
    rec.update(run("small_", 2, (2000.0, 2000.0, 2000.0), gc, (12, 10, 8), seed=701, rotations=[20.0, -35.0],
                   scale_mults=[1.1, 0.85], flip=[False, True]))
    rec.update(run("root_", 2, SPACE_SIZE, [list(SPACE_CENTER)], ROOT_CUBE, seed=702, stride=ROOT_STRIDE))
    out = os.path.join(HERE, "unproj_coco17_cam3.npz")
    np.savez_compressed(out, **rec)
    print(f"unproj_coco17_cam3: {time.time() - t0:.1f} s, {os.path.getsize(out) / 1e6:.2f} MB")


if __name__ == "__main__":
    mg2.install_shims()
    torch.set_num_threads(8)
    main()
