"""17..32 joints on the NHWC path (Jp = 32: two 16-channel groups of one 128-byte pixel), on the Shelf / Campus rigs.
The referee is the CPU oracle, pinned against the reference's own 17-joint outputs by tests/test_coco17_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle
from selfpose3d_amd import _lib, synthetic as syn
from selfpose3d_amd.camera_pack import pack_cameras
from selfpose3d_amd.config import load_config
from selfpose3d_amd.project_layer import ProjectLayer, _packed_source

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = {"campus_synthetic": os.path.join(ROOT, "configs", "campus_synthetic_coco17_cam3.yaml"),
        "shelf_synthetic": os.path.join(ROOT, "configs", "shelf_synthetic_coco17_cam5.yaml")}
ROOT_CUBE = (80, 80, 20)
FINE = (64, 64, 64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def rig_setup(rig, B, J, seed, rotations=None, scale_mults=None, flip=None):
    cfg = load_config(YAML[rig], NETWORK__NUM_JOINTS=J)
    img = tuple(int(v) for v in cfg.NETWORK.IMAGE_SIZE)
    hm = tuple(int(v) for v in cfg.NETWORK.HEATMAP_SIZE)
    V = int(cfg.DATASET.CAMERA_NUM)
    center = tuple(float(v) for v in cfg.MULTI_PERSON.SPACE_CENTER)
    meta = syn.make_meta(B, V, img, rotations=rotations, scale_mults=scale_mults, rig=rig, target=center)
    hms = syn.random_heatmaps(B, V, J, hm[1], hm[0], seed=seed)
    flip_t = None if flip is None else torch.tensor(flip, dtype=torch.bool)
    cam = pack_cameras(meta, B, img, flip_t)
    return cfg, img, hm, V, center, meta, hms, flip_t, cam


def wide_calls(monkeypatch):
    """records the (layout, jp) of every unprojection launch made through _lib"""
    calls = []
    real = _lib.unproject_fwd

    def rec(views, layout, jp, *a, **k):
        calls.append((layout, jp))
        return real(views, layout, jp, *a, **k)
    monkeypatch.setattr(_lib, "unproject_fwd", rec)
    return calls


# ---- 1. the re-tiling pass at Jp = 32 -------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [17, 29, 32])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_pack_jp32_pads_with_zeros(dev, J, dt):
    hms = syn.random_heatmaps(2, 3, J, 19, 23, seed=J)
    src = [(h + 0.5).to(dev).to(dt) for h in hms]               # no zero in the maps: a zero channel is padding
    packed = _lib.pack_heatmaps(src, jp=32, out_dtype=dt)
    assert packed.shape == (3, 2, 19, 23, 32) and packed.dtype == dt
    assert torch.count_nonzero(packed[..., J:]) == 0
    want = torch.stack([h.permute(0, 2, 3, 1) for h in src])
    assert torch.equal(packed[..., :J], want)


# ---- 2. bit-exact against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["campus_synthetic", "shelf_synthetic"])
@pytest.mark.parametrize("J,B", [(17, 1), (17, 4), (20, 1), (24, 4), (32, 1), (32, 4)])
def test_root_grid_bit_exact(dev, rig, J, B):
    cfg, img, hm, V, center, meta, hms, _, cam = rig_setup(rig, B, J, seed=100 + J + B)
    space = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE]
    layer = ProjectLayer(cfg)
    with torch.no_grad():
        cubes, grids = layer([h.to(dev) for h in hms], meta, space, [list(center)], list(ROOT_CUBE))
    centers = np.repeat(np.asarray([center], np.float32), B, 0)
    ref, ref_g = oracle.unproject_fwd([h.numpy() for h in hms], cam, centers, np.ones(B, np.uint8), space, ROOT_CUBE, img)
    assert cubes.shape == (B, J) + ROOT_CUBE and cubes.is_contiguous()
    assert np.array_equal(cubes.cpu().numpy(), ref)
    assert np.array_equal(grids.cpu().numpy(), ref_g)


@pytest.mark.parametrize("rig", ["campus_synthetic", "shelf_synthetic"])
@pytest.mark.parametrize("J", [17, 20, 24, 32])
def test_person_cubes_into_padded_buffer(dev, rig, J):
    """8 64^3 cubes through sample_of, two of them invalid, written into a padded buffer: bit-exact, padding untouched"""
    B = 4
    cfg, img, hm, V, center, meta, hms, _, cam = rig_setup(rig, B, J, seed=200 + J)
    c = np.asarray(center)
    rng = np.random.default_rng(J)
    P = 8
    sample_of = np.array([0, 0, 1, 2, 2, 3, 3, 1], np.int32)
    gc = np.zeros((P, 5), np.float32)
    gc[:, :3] = c + rng.uniform(-1500, 1500, (P, 3)) * np.array([1, 1, 0.2])
    gc[:, 3] = 0.0
    gc[[2, 6], 3] = -1.0                                           # skipped rows: zero cubes
    buf = torch.full((P, J, 66, 65, 68), float("nan"), device=dev)
    out = buf[:, :, 1:65, :64, :64]
    layer = ProjectLayer(cfg)
    with torch.no_grad():
        layer.get_voxel([h.to(dev) for h in hms], meta, syn.FINE_GRID_SIZE, torch.from_numpy(gc).to(dev), list(FINE),
                        want_grids=False, sample_of=torch.from_numpy(sample_of).to(dev), out=out)
    ref, _ = oracle.unproject_fwd([h.numpy()[sample_of] for h in hms], cam[sample_of], gc[:, :3], (gc[:, 3] >= 0).astype(np.uint8),
                                  syn.FINE_GRID_SIZE, FINE, img, want_grids=False)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert not ref[[2, 6]].any()
    pad = torch.ones_like(buf, dtype=torch.bool)
    pad[:, :, 1:65, :64, :64] = False
    assert bool(torch.isnan(buf[pad]).all()), "elements outside the addressed cubes were written"


@pytest.mark.parametrize("rig", ["campus_synthetic", "shelf_synthetic"])
def test_flip_and_rotated_crop_bit_exact(dev, rig):
    B, J = 2, 17
    cfg, img, hm, V, center, meta, hms, flip, cam = rig_setup(rig, B, J, seed=7, rotations=[25.0, -40.0],
                                                               scale_mults=[1.15, 0.9], flip=[True, False])
    gc = torch.tensor([[center[0] + 300.0, center[1] - 200.0, 900.0, 0.0, 0.9],
                       [center[0] - 500.0, center[1] + 400.0, 1000.0, 1.0, 0.8]])
    layer = ProjectLayer(cfg)
    with torch.no_grad():
        cubes, grids = layer([h.to(dev) for h in hms], meta, syn.FINE_GRID_SIZE, gc.to(dev), list(FINE), flip_xcoords=flip)
    ref, ref_g = oracle.unproject_fwd([h.numpy() for h in hms], cam, gc[:, :3].numpy(), np.ones(B, np.uint8),
                                      syn.FINE_GRID_SIZE, FINE, img)
    assert np.array_equal(cubes.cpu().numpy(), ref) and np.array_equal(grids.cpu().numpy(), ref_g)


# ---- 3. bf16 storage at 17 joints ------------------------------------------------------------------------------------
def test_bf16_storage_17_joints(dev):
    """parity definition of test_gpu_parity.py::test_bf16_storage_config: the oracle on the bf16-rounded maps, its fp32
    result rounded to bf16 (RNE)"""
    B, J = 2, 17
    cfg, img, hm, V, center, meta, hms32, _, cam = rig_setup("campus_synthetic", B, J, seed=60)
    hms16 = [h.to(torch.bfloat16) for h in hms32]
    gc = torch.tensor([[center[0] + 300.0, center[1] - 800.0, 900.0, 0.0, 0.9],
                       [center[0] - 700.0, center[1] + 100.0, 1000.0, 1.0, 0.8]])
    ref, ref_g = oracle.unproject_fwd([h.float().numpy() for h in hms16], cam, gc[:, :3].numpy(), np.ones(B, np.uint8),
                                      syn.FINE_GRID_SIZE, FINE, img)
    ref16 = torch.from_numpy(ref).to(torch.bfloat16)
    layer = ProjectLayer(cfg, io_dtype=torch.bfloat16)
    for src in (hms16, hms32):
        with torch.no_grad():
            cubes, grids = layer([h.to(dev) for h in src], meta, syn.FINE_GRID_SIZE, gc.to(dev), list(FINE))
        assert cubes.dtype == torch.bfloat16 and grids.dtype == torch.float32
        assert torch.equal(cubes.cpu(), ref16)
        assert np.array_equal(grids.cpu().numpy(), ref_g)
    # bf16 maps -> fp32 cubes, fp32 maps -> bf16 cubes
    camd, cen = torch.from_numpy(cam).to(dev), gc[:, :3].contiguous().to(dev)
    val = torch.ones(B, dtype=torch.uint8, device=dev)
    p16 = _lib.pack_heatmaps([h.to(dev) for h in hms16], jp=32, out_dtype=torch.bfloat16)
    c32, _ = _lib.unproject_fwd([p16[c] for c in range(V)], _lib.LAYOUT_NHWC, 32, camd, cen, val, B, J, hm[1], hm[0], FINE,
                                syn.FINE_GRID_SIZE, img, False)
    assert torch.equal(c32.cpu(), torch.from_numpy(ref))
    ref32, _ = oracle.unproject_fwd([h.numpy() for h in hms32], cam, gc[:, :3].numpy(), np.ones(B, np.uint8),
                                    syn.FINE_GRID_SIZE, FINE, img, want_grids=False)
    p32 = _lib.pack_heatmaps([h.to(dev) for h in hms32], jp=32)
    cb, _ = _lib.unproject_fwd([p32[c] for c in range(V)], _lib.LAYOUT_NHWC, 32, camd, cen, val, B, J, hm[1], hm[0], FINE,
                               syn.FINE_GRID_SIZE, img, False, out_dtype=torch.bfloat16)
    assert torch.equal(cb.cpu(), torch.from_numpy(ref32).to(torch.bfloat16))


# ---- 4. the backbone's channels-last hand-over -----------------------------------------------------------------------
def test_backbone_emits_32_channel_buffer(dev):
    from selfpose3d_amd import pose_resnet
    B, J = 2, 17
    cfg = load_config(YAML["campus_synthetic"], POSE_RESNET__NUM_LAYERS=18)
    net = pose_resnet.get_pose_net(cfg, is_train=False)
    torch.manual_seed(0)
    for m in net.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            torch.nn.init.kaiming_normal_(m.weight)
    net.eval().to(dev).to(memory_format=torch.channels_last)
    views = [torch.randn(B, 3, 64, 96, device=dev) for _ in range(3)]
    with torch.no_grad():
        outs = net.forward_views(views)
        ref = [net(v) for v in views]
    src = _packed_source(outs, 32, torch.float32)
    assert src is not None and src.shape == (3, B, 16, 24, 32)
    assert torch.count_nonzero(src[..., J:]) == 0
    for o, r in zip(outs, ref):
        assert o.shape == r.shape == (B, J, 16, 24)
        assert float((o - r).abs().max()) <= 1e-4 * float(r.abs().max())
    # unprojecting the views == unprojecting a planar copy of them, bit for bit
    cfg2 = load_config(YAML["campus_synthetic"], NETWORK__HEATMAP_SIZE=[24, 16], NETWORK__IMAGE_SIZE=[96, 64])
    meta = syn.make_meta(B, 3, (96, 64), rig="campus_synthetic", target=tuple(cfg.MULTI_PERSON.SPACE_CENTER))
    layer = ProjectLayer(cfg2)
    space = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE]
    args = (meta, space, [list(cfg.MULTI_PERSON.SPACE_CENTER)], [24, 24, 8])
    with torch.no_grad():
        a, ga = layer(outs, *args)
        b, gb = layer([o.contiguous() for o in outs], *args)
    assert torch.equal(a, b) and torch.equal(ga, gb)


# ---- 5-7. root net and pose net at 17 joints --------------------------------------------------------------------------
def _nets(dev, J=17):
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    from selfpose3d_amd.pose_regression_net import PoseRegressionNet
    # every proposal slot valid (random-init nets score anywhere): the pose net always has cubes to work on
    cfg = load_config(YAML["campus_synthetic"], NETWORK__NUM_JOINTS=J, MULTI_PERSON__THRESHOLD=-1e9, MULTI_PERSON__MAX_PEOPLE_NUM=4)
    torch.manual_seed(3)
    root, pose = CuboidProposalNet(cfg), PoseRegressionNet(cfg)
    for net in (root, pose):
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 2.0)
        net.eval().to(dev)
    return cfg, root, pose


def _people_heatmaps(cfg, B, seed):
    """Gaussian heat-maps of synthetic people seen by the Campus rig (a root net has peaks to find)"""
    from selfpose3d_amd.synthetic_dataset import SyntheticPanoptic
    ds = SyntheticPanoptic(cfg, num_frames=B, seed=seed, images=False)
    items = [ds[i] for i in range(B)]
    hms = [torch.stack([it[1][v] for it in items]) for v in range(ds.V)]
    from torch.utils.data import default_collate
    meta = [default_collate([it[4][v] for it in items]) for v in range(ds.V)]
    return hms, meta


def _pose_from_cubes(pose, cubes, centers):
    """the pose net's chunk loop (PoseRegressionNet.forward_batched without the FFT-buffer hand-over) on given cubes"""
    outs = []
    for s0 in range(0, cubes.shape[0], 8):
        chunk = cubes[s0:s0 + 8]
        n = chunk.shape[0]
        m = 1 << (n - 1).bit_length()
        if m != n:
            chunk = torch.cat([chunk, chunk[-1:].expand(m - n, -1, -1, -1, -1)], 0)
        y = pose.v2v_net(chunk)[:n]
        outs.append(_lib.soft_argmax_grid(y, centers[s0:s0 + n], pose.grid_size, pose.cube_size, pose.soft_argmax_layer.beta))
    return torch.cat(outs, 0)


def test_root_and_pose_net_match_planar_cubes(dev, monkeypatch):
    """Root net V2VNet(17,1) and pose net V2VNet(17,17) in eval.  The Jp = 32 cubes are the oracle's bit for bit (above);
    the planar kernel's are not: it divides by the view count where the NHWC kernels multiply by its rounded reciprocal
    (fuse vs fuse_rcp, sp3d_device.h) and projects with the plain linspace / sample_pos, so they differ in the last bits.
    Hence: the nets' results equal the same cubes pushed through the same V2V bit for bit (the hand-over into the FFT
    buffer changes nothing), and the planar kernel's cubes through the same V2V within rounding, NMS picks identical."""
    B = 4
    cfg, root, pose = _nets(dev)
    hms, meta = _people_heatmaps(cfg, B, seed=11)
    hms = [h.to(dev) for h in hms]
    calls = wide_calls(monkeypatch)
    with torch.no_grad():
        root_cubes, grid_centers = (t.clone() for t in root(hms, meta))      # (plan-owned buffers: reused below)
        poses = pose.forward_batched(hms, meta, grid_centers).clone()
        assert len(calls) == 2 and all(l == _lib.LAYOUT_NHWC and jp == 32 for l, jp in calls), calls
        planar = ProjectLayer(cfg, mode="planar")
        cubes_p, _ = planar.get_voxel(hms, meta, root.grid_size, [root.grid_center], root.cube_size, want_grids=False)
        cubes_n, _ = root.project_layer.get_voxel(hms, meta, root.grid_size, [root.grid_center], root.cube_size,
                                                  want_grids=False)
        assert float((cubes_n - cubes_p).abs().max()) <= 1e-6
        root_n = root.v2v_net(cubes_n).squeeze(1).clone()
        centers_n = root.proposal_layer(root_n, meta).clone()
        root_p = root.v2v_net(cubes_p).squeeze(1).clone()
        centers_p = root.proposal_layer(root_p, meta).clone()
    assert torch.equal(root_cubes, root_n) and torch.equal(grid_centers, centers_n)
    assert float((root_cubes - root_p).abs().max()) <= 1e-4 * max(1.0, float(root_p.abs().max()))
    assert torch.equal(grid_centers[..., :4], centers_p[..., :4])            # NMS picks: same voxels, same order
    assert torch.allclose(grid_centers[..., 4], centers_p[..., 4], rtol=0, atol=1e-4)
    assert int((grid_centers[:, :, 3] >= 0).sum()) >= 1
    pairs = torch.nonzero(grid_centers[:, :, 3] >= 0)
    bi, ki = pairs[:, 0], pairs[:, 1]
    centers = grid_centers[bi, ki, :3].contiguous()
    with torch.no_grad():
        cn, _ = pose.project_layer.get_voxel(hms, meta, pose.grid_size, centers, pose.cube_size, want_grids=False, sample_of=bi)
        cp, _ = planar.get_voxel(hms, meta, pose.grid_size, centers, pose.cube_size, want_grids=False, sample_of=bi)
        want_n = _pose_from_cubes(pose, cn, centers)
        want_p = _pose_from_cubes(pose, cp, centers)
    assert torch.equal(poses[bi, ki], want_n)
    assert float((poses[bi, ki] - want_p).abs().max()) <= 0.05                   # mm


def test_graphed_root_net_replay_equals_eager(dev):
    from selfpose3d_amd.graphs import GraphedRootNet
    B = 4
    cfg, root, _ = _nets(dev)
    hms, meta = _people_heatmaps(cfg, B, seed=12)
    static = [h.to(dev).contiguous() for h in hms]
    with torch.no_grad():
        eager_cubes, eager_centers = root(static, meta)
        eager_cubes, eager_centers = eager_cubes.clone(), eager_centers.clone()
    g = GraphedRootNet(root, static, meta)
    out_cubes, out_centers = g()
    torch.cuda.synchronize()
    assert torch.equal(out_cubes, eager_cubes) and torch.equal(out_centers, eager_centers)
    # new heat-maps through the same graph
    hms2, _ = _people_heatmaps(cfg, B, seed=13)
    for s, h in zip(g.static_hms, hms2):
        s.copy_(h.to(dev))
    out_cubes, out_centers = g()
    torch.cuda.synchronize()
    with torch.no_grad():
        out_cubes, out_centers = out_cubes.clone(), out_centers.clone()
        e2, c2 = root([h.to(dev) for h in hms2], meta)
    assert torch.equal(out_cubes, e2) and torch.equal(out_centers, c2)


def test_eval_launches_no_planar_unprojection(dev, monkeypatch):
    from selfpose3d_amd.models import get_multi_person_pose_net
    B = 2
    cfg = load_config(YAML["campus_synthetic"], POSE_RESNET__NUM_LAYERS=18, MULTI_PERSON__THRESHOLD=-1e9,
                      MULTI_PERSON__MAX_PEOPLE_NUM=4)
    hms, meta = _people_heatmaps(cfg, B, seed=14)
    model = get_multi_person_pose_net(cfg, is_train=False).to(dev).eval()
    calls = wide_calls(monkeypatch)
    with torch.no_grad():
        out = model(meta=meta, input_heatmaps=[h.to(dev) for h in hms])
    assert calls and all(l == _lib.LAYOUT_NHWC and jp == 32 for l, jp in calls), calls
    assert len(calls) >= 2                                          # root net and pose net
    assert out[0].shape[2] == 17
    # a heat-map gradient keeps the planar kernel (the pass mask is 16 bits per voxel), and an explicit NHWC request says so
    layer = ProjectLayer(cfg)
    hg = [h.to(dev).requires_grad_(True) for h in hms]
    space = [float(v) for v in cfg.MULTI_PERSON.SPACE_SIZE]
    calls.clear()
    cubes, _ = layer(hg, meta, space, [list(cfg.MULTI_PERSON.SPACE_CENTER)], [16, 16, 8])
    assert calls == [(_lib.LAYOUT_PLANAR, 0)]
    cubes.sum().backward()
    with pytest.raises(_lib.Sp3dError, match="16 joints"):
        ProjectLayer(cfg, mode="nhwc")(hg, meta, space, [list(cfg.MULTI_PERSON.SPACE_CENTER)], [16, 16, 8])


# ---- 8. validation on both configurations -----------------------------------------------------------------------------
@pytest.mark.parametrize("rig", ["campus_synthetic", "shelf_synthetic"])
def test_validate_3d_runs(rig, tmp_path):
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "validate_3d.py"), "--cfg", YAML[rig], "--random-init",
                        "--frames", "4"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
