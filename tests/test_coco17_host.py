"""17..32 joints (the Shelf / Campus configurations) without a GPU: the CPU oracle against the reference's own 17-joint
outputs (the referee of tests/test_gpu_coco17.py), the Jp = 32 contract of the C ABI, the configurations and the
synthetic Shelf / Campus rigs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from selfpose3d_amd import _lib, build as sbuild, synthetic as syn
from selfpose3d_amd.camera_pack import pack_cameras
from selfpose3d_amd.config import load_config
from selfpose3d_amd.project_layer import ProjectLayer
from selfpose3d_amd.synthetic_dataset import SyntheticPanoptic, SyntheticPanopticSSV
from tests import golden_io as gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMPUS = os.path.join(ROOT, "configs", "campus_synthetic_coco17_cam3.yaml")
SHELF = os.path.join(ROOT, "configs", "shelf_synthetic_coco17_cam5.yaml")
VOX_TOL = 1e-6


def golden_case(g, prefix):
    """inputs of one record of unproj_coco17_cam3.npz, rebuilt as tests/golden/make_goldens_r7.py made them"""
    B = int(g[prefix + "B"])
    V, J = int(g["V"]), int(g["J"])
    img, hm = tuple(int(v) for v in g["img"]), tuple(int(v) for v in g["hm"])
    rot = g[prefix + "rotations"]
    mult = g[prefix + "scale_mults"]
    meta = syn.make_meta(B, V, img, rotations=list(rot) if len(rot) else None, scale_mults=list(mult) if len(mult) else None,
                         rig=str(g["rig"]), target=tuple(g["space_center"]))
    flip = torch.tensor(g[prefix + "flip"]) if len(g[prefix + "flip"]) else None
    hms = syn.random_heatmaps(B, V, J, hm[1], hm[0], seed=int(g[prefix + "seed"]))
    gc = g[prefix + "grid_center"]
    if bool(g[prefix + "center_is_list"]):
        centers = np.repeat(np.asarray(gc, np.float32).reshape(1, 3), B, 0)
        valid = np.ones(B, np.uint8)
    else:
        centers = np.asarray(gc[:, :3], np.float32)
        valid = (gc[:, 3] >= 0).astype(np.uint8)
    cam = pack_cameras(meta, B, img, flip)
    return dict(B=B, V=V, J=J, img=img, hm=hm, meta=meta, flip=flip, hms=hms, cam=cam, centers=centers, valid=valid,
                grid_size=[float(v) for v in g[prefix + "grid_size"]], cube=[int(v) for v in g[prefix + "cube"]])


@pytest.mark.parametrize("prefix", ["small_", "root_"])
def test_oracle_matches_reference_at_17_joints(prefix):
    g = gio.load("unproj_coco17_cam3")
    c = golden_case(g, prefix)
    cubes, grids = oracle.unproject_fwd([h.numpy() for h in c["hms"]], c["cam"], c["centers"], c["valid"], c["grid_size"],
                                        c["cube"], c["img"])
    B, J = c["B"], c["J"]
    N = int(np.prod(c["cube"]))
    assert cubes.shape == (B, J) + tuple(c["cube"])
    if prefix + "cubes" in g:
        exp_c, exp_g = g[prefix + "cubes"].reshape(B, J, N), g[prefix + "grids"]
        got_c, got_g = cubes.reshape(B, J, N), grids
    else:
        idx = g[prefix + "sub_idx"]
        exp_c, exp_g = g[prefix + "cubes_sub"], g[prefix + "grids_sub"]
        got_c, got_g = cubes.reshape(B, J, N)[:, :, idx], grids[:, idx]
    assert np.array_equal(got_g, exp_g), "grids must be bit-exact"
    assert np.abs(got_c - exp_c).max() <= VOX_TOL
    assert abs(cubes.astype(np.float64).sum() - float(g[prefix + "cubes_sum"])) <= 1e-7 * cubes.size
    assert np.allclose(cubes.astype(np.float64).sum(axis=(2, 3, 4)), g[prefix + "cubes_sum_per_sample_joint"], rtol=0,
                       atol=1e-7 * cubes[0, 0].size)
    assert np.allclose(grids.astype(np.float64).sum(axis=(0, 1)), g[prefix + "grids_sum"], rtol=1e-12, atol=1e-6)


def test_jp_for_wide_range():
    assert [ProjectLayer.jp_for(J) for J in range(17, 33)] == [32] * 16
    assert [ProjectLayer.jp_for(J) for J in (1, 4, 5, 8, 9, 12, 13, 16)] == [4, 4, 8, 8, 12, 12, 16, 16]


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def test_cabi_jp32_limits_validated_before_any_launch(lib):
    """every refusal below comes back as SP3D_EUNSUPPORTED (-4) with pointers that are never dereferenced: no launch"""
    gs = (C.c_float * 3)(8000, 8000, 2000)
    views = (C.c_void_p * 2)(0x1000, 0x1000)
    d = C.c_void_p(0x1000)
    f = lib.sp3d_unproject_fwd
    # a channel stride that is not one of 4/8/12/16/32
    assert f(views, 1, 36, d, d, d, d, None, 1, 2, 17, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
    assert f(views, 1, 20, d, d, d, d, None, 1, 2, 17, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
    # Jp = 32 holds at most 32 joints
    assert f(views, 1, 32, d, d, d, d, None, 1, 2, 33, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
    # Jp = 32: no channels-last result
    assert f(views, 1 | _lib.OUT_CHANNELS_LAST, 32, d, d, d, d, None, 1, 2, 20, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
    # Jp = 32: heat-maps of at least 2x2 pixels
    assert f(views, 1, 32, d, d, d, d, None, 1, 2, 17, 1, 8, 4, 4, 4, gs, 96, 72, None) == -4
    # the fused z-spectrum entry: Jp = 16 only
    z = lib.sp3d_unproject_fwd_zdft
    spec = C.c_void_p(0x10000)
    assert z(views, 32, d, d, d, spec, 1, 2, 17, 8, 8, 4, 4, 20, gs, 96, 72, 28, None) == -4
    # the pass-mask (training) forward and both packed backward entries: at most 16 channels
    t = lib.sp3d_unproject_fwd_train
    assert t(views, 1, 32, d, None, d, d, d, None, d, 1, 2, 17, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
    for name in ("sp3d_unproject_bwd_packed", "sp3d_unproject_bwd_packed_det"):
        b = getattr(lib, name)
        det = name.endswith("_det")
        args = [d, None, d, d, d, d, d] + ([d] if det else []) + [1, 1, 2, 17, 32, 8, 8, 4, 4, 4, gs, 96, 72, 0, None]
        assert b(*args) == -4, name
    # the re-tiling pass: Jp in 4/8/12/16/32, J <= Jp
    assert lib.sp3d_pack_heatmaps(views, d, 1, 2, 17, 36, 8, 8, None) == -4
    assert lib.sp3d_pack_heatmaps(views, d, 1, 2, 33, 32, 8, 8, None) == -4


@pytest.mark.parametrize("path,name,V", [(CAMPUS, "campus_synthetic", 3), (SHELF, "shelf_synthetic", 5)])
def test_configs_load(path, name, V):
    cfg = load_config(path)
    assert cfg.MODEL == "multi_person_posenet"
    assert int(cfg.NETWORK.NUM_JOINTS) == 17 and list(cfg.DATASET.ROOTIDX) == [11, 12]
    assert int(cfg.DATASET.CAMERA_NUM) == V
    assert cfg.DATASET.TRAIN_DATASET == name and cfg.DATASET.TEST_DATASET == name
    assert [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE] == [80, 80, 20]
    assert [int(v) for v in cfg.PICT_STRUCT.CUBE_SIZE] == [64, 64, 64]


@pytest.mark.parametrize("path,V,orig", [(CAMPUS, 3, (360, 288)), (SHELF, 5, (1032, 776))])
@pytest.mark.parametrize("cls", [SyntheticPanoptic, SyntheticPanopticSSV])
def test_dataset_rig(path, V, orig, cls):
    cfg = load_config(path)
    w, h = (int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    ds = cls(cfg, num_frames=6, seed=3, images=False)
    cams = syn.rig_cameras(cfg.DATASET.TEST_DATASET, cfg.MULTI_PERSON.SPACE_CENTER)[0]
    for i in range(len(ds)):
        item = ds[i]
        sets = [item[6 * k:6 * k + 6] for k in range(len(item) // 6)]
        for inputs, targets, weights, t3ds, metas, ihm in sets:
            assert len(targets) == V and len(metas) == V
            assert all(tuple(t.shape) == (17, h, w) for t in targets)
            m = metas[0]
            assert np.array_equal(np.asarray(m["center"], np.float64), np.array(orig, np.float64) / 2.0)
            if cls is SyntheticPanoptic:
                assert np.array_equal(np.asarray(m["scale"]), syn.get_scale(orig, cfg.NETWORK.IMAGE_SIZE))
            P = int(m["num_person"])
            assert P >= 1
            roots = np.asarray(m["roots_3d"])[:P]
            assert np.allclose(roots, np.asarray(m["joints_3d"])[:P][:, [11, 12]].mean(axis=1), rtol=0, atol=1e-9)
            # every synthetic root lies inside at least two camera images
            seen = np.zeros(P, int)
            for cam in cams:
                px = syn._project_f64(roots, cam)
                seen += (px[:, 0] >= 0) & (px[:, 0] < orig[0]) & (px[:, 1] >= 0) & (px[:, 1] < orig[1])
            assert seen.min() >= 2, seen


def test_rig_rejects_wrong_camera_count():
    cfg = load_config(SHELF, DATASET__CAMERA_NUM=4)
    with pytest.raises(ValueError):
        SyntheticPanoptic(cfg, num_frames=1, images=False)


def test_panoptic_rig_unchanged():
    """any other dataset name keeps the Panoptic ring of 1920x1080 cameras"""
    cfg = load_config(os.path.join(ROOT, "configs", "synthetic_small.yaml"))
    ds = SyntheticPanoptic(cfg, num_frames=1, images=False)
    m = ds[0][4][0]
    assert np.array_equal(m["center"], np.array([960.0, 540.0]))
    ring = syn.ring_cameras(int(cfg.DATASET.CAMERA_NUM))
    assert all(np.array_equal(a["R"], b["R"]) and float(a["fx"]) == float(b["fx"]) for a, b in zip(ds.cams, ring))
    assert np.array_equal(np.asarray(m["roots_3d"]), np.asarray(m["joints_3d"])[:, 2])
