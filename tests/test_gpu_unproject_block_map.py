"""The unprojection at the shapes the V2V nets run, whole volume, bit-exact against the CPU oracle.

The block map (octants at B = 1, blocks at B = 2 / 4; selfpose3d_amd/csrc/sp3d_device.h:413-440) has been the brick kernels'
default since round 6; tests/test_xcd_block_map.py checks its algebra on the host, this file checks the kernels: every voxel of
every cube equal to the oracle's (np.array_equal), with the destination prefilled with NaN (through ``out=``) or the
allocator's free blocks filled with NaN, so that a tile no workgroup writes cannot pass.  The fused unprojection / z-DFT is
compared with the z-spectrum of the ORACLE's whole-volume cubes (tests/test_gpu_fused_zdft.py compares it with the two-kernel
HIP path)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_v2v_plan_f64 import poison_free_blocks

pytestmark = pytest.mark.gpu

IMG, HM, V = (960, 512), (240, 128), 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _scene(B, J, seed, centers=None):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    meta = syn.make_meta(B, V, list(IMG))
    hms = syn.random_heatmaps(B, V, J, HM[1], HM[0], seed=seed)
    cam = pack_cameras(meta, B, list(IMG))
    if centers is None:
        centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), B, 0)
    return meta, hms, cam, centers


def _oracle(hms, cam, centers, valid, grid_size, cube, sample_of=None):
    from oracle import oracle
    hs = [h.numpy() for h in hms]
    if sample_of is not None:
        hs = [h[sample_of] for h in hs]
        cam = cam[sample_of]
    c, _ = oracle.unproject_fwd(hs, cam, centers, valid, grid_size, cube, list(IMG), want_grids=False)
    return c


def _views(dev, hms, jp):
    from selfpose3d_amd import _lib
    packed = _lib.pack_heatmaps([h.to(dev) for h in hms], jp=jp)
    return [packed[c] for c in range(len(hms))]


def test_roothm_root_input_whole_volume(dev):
    """(a) NETWORK.ROOTNET_ROOTHM: what CuboidProposalNet hands its V2VNet(1, 1) - the root-joint channel sliced with
    .contiguous() (cuboid_proposal_net.py:77), channels-last padded cubes - at 80 x 80 x 20, B = 1, 2, 4, 5 x 240 x 128"""
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
    cfg = load_config(None, NETWORK__ROOTNET_ROOTHM=True)
    net = CuboidProposalNet(cfg).eval().to(dev).use_channels_last(True)
    for B, seed in ((1, 801), (2, 802), (4, 803)):
        meta, hms, cam, centers = _scene(B, 15, seed, np.repeat(np.asarray([net.grid_center], np.float32), B, 0))
        got = {}
        inner = net.project_layer.get_voxel

        def spy(*a, **k):
            c, g = inner(*a, **k)
            got["cubes"] = c.clone()
            return c, g
        net.project_layer.get_voxel = spy
        try:
            poison_free_blocks(dev)
            with torch.no_grad():
                net([h.to(dev) for h in hms], meta)
            torch.cuda.synchronize(dev)
        finally:
            del net.project_layer.get_voxel
        c = got["cubes"]
        assert tuple(c.shape) == (B, 4, 80, 80, 20), c.shape
        rid = net.root_id
        want = _oracle([h[:, rid:rid + 1].contiguous() for h in hms], cam, centers, np.ones(B, np.uint8), net.grid_size,
                       net.cube_size)
        g = c.cpu().numpy()
        assert np.array_equal(g[:, :1], want), (B, float(np.nanmax(np.abs(g[:, :1] - want))))
        assert not np.any(g[:, 1:]), B                                   # padded channels: zero, not NaN
        assert float(want.max()) > 0.5


# (B, J, cube, channels_last): the block map on odd and non-square column grids; planar output takes the brick kernel only
# for Z % 32 == 0 (default variant 56), channels-last always (120), with J a multiple of 4
BLOCK_SHAPES = [
    (2, 12, (76, 60, 20), True),       # 19 x 15 columns, quadrants
    (2, 15, (76, 60, 32), False),
    (4, 8, (68, 44, 20), True),        # 17 x 11 columns, halves
    (4, 15, (68, 44, 64), False),
    (1, 16, (40, 40, 12), True),       # 10 x 10 columns: octants with h = 5
    (1, 15, (40, 40, 32), False),
    (1, 4, (88, 88, 8), True),         # 22 x 22 columns: octants with h = 11
    (1, 15, (88, 88, 32), False),
]


@pytest.mark.parametrize("B,J,cube,cl", BLOCK_SHAPES)
def test_block_map_shapes_whole_volume(dev, B, J, cube, cl):
    """(b) the brick kernels under the block map, every voxel against the oracle"""
    from selfpose3d_amd import _lib
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.project_layer import ProjectLayer
    seed = 810 + B * 7 + cube[2]
    meta, hms, cam, centers = _scene(B, J, seed)
    jp = ProjectLayer.jp_for(J)
    views = _views(dev, hms, jp)
    valid = np.ones(B, np.uint8)
    args = (torch.from_numpy(cam).to(dev), torch.from_numpy(centers).to(dev), torch.from_numpy(valid).to(dev))
    X, Y, Z = cube
    if cl:
        poison_free_blocks(dev)
        c, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, jp, *args, B, J, HM[1], HM[0], cube, syn.SPACE_SIZE, IMG, False,
                                  channels_last=True)
        assert c.is_contiguous(memory_format=torch.channels_last_3d)
    else:
        out = torch.full((B, J, X, Y, Z), float("nan"), device=dev)
        c, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, jp, *args, B, J, HM[1], HM[0], cube, syn.SPACE_SIZE, IMG, False,
                                  out=out)
    torch.cuda.synchronize(dev)
    got = c.cpu().numpy()
    want = _oracle(hms, cam, centers, valid, syn.SPACE_SIZE, cube)
    assert np.array_equal(got, want), (B, J, cube, cl, float(np.nanmax(np.abs(got - want))), int(np.isnan(got).sum()))
    assert float(want.max()) > 0.5


@pytest.mark.parametrize("P", [2, 3, 4])
def test_person_cubes_through_sample_of(dev, P):
    """(c) 64^3 person cubes read from rows sample_of[p] (P = 2, 4: block map; P = 3: chunk map), one of them invalid:
    written into a strided view of a NaN-filled padded buffer (what PoseRegressionNet.forward_batched hands the unprojection,
    planar, brick default 56) and as channels-last 16-channel cubes (120)"""
    from selfpose3d_amd import _lib
    from selfpose3d_amd.config import load_config
    cfg = load_config(None)
    cube = [int(v) for v in cfg.PICT_STRUCT.CUBE_SIZE]
    gs = [float(v) for v in cfg.PICT_STRUCT.GRID_SIZE]
    assert cube == [64, 64, 64]
    B, J = 2, 15
    meta, hms, cam, _ = _scene(B, J, 830 + P)
    rng = np.random.default_rng(P)
    sample_of = np.array([p % B for p in range(P)][::-1], np.int64)
    centers = np.stack([rng.uniform(-1500, 1500, P), rng.uniform(-1500, 1500, P), rng.uniform(700, 1100, P)], 1).astype(np.float32)
    valid = np.ones(P, np.uint8)
    valid[P // 2] = 0
    want = _oracle(hms, cam, centers, valid, gs, cube, sample_of=sample_of)
    assert not np.any(want[P // 2]) and float(want.max()) > 0.5
    views = _views(dev, hms, 16)
    so = torch.from_numpy(sample_of.astype(np.int32)).to(dev)
    args = (torch.from_numpy(cam).to(dev), torch.from_numpy(centers).to(dev), torch.from_numpy(valid).to(dev))
    S = 72                                                        # the opening conv's FFT length for 64 (v2v_net._fft_shape)
    buf = torch.full((4, J, S, S, S), float("nan"), device=dev)
    view = buf[:P, :, :64, :64, :64]
    _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, 16, *args, P, J, HM[1], HM[0], cube, gs, IMG, False, sample_of=so, out=view)
    torch.cuda.synchronize(dev)
    got = view.cpu().numpy()
    assert np.array_equal(got, want), (P, float(np.nanmax(np.abs(got - want))), int(np.isnan(got).sum()))
    rest = buf.clone()
    rest[:P, :, :64, :64, :64] = float("nan")
    assert bool(torch.isnan(rest).all()), "the kernel wrote outside its view of the padded buffer"
    poison_free_blocks(dev)
    c, _ = _lib.unproject_fwd(views, _lib.LAYOUT_NHWC, 16, *args, P, 16, HM[1], HM[0], cube, gs, IMG, False,
                              channels_last=True, sample_of=so)
    torch.cuda.synchronize(dev)
    got = c.cpu().numpy()
    assert np.array_equal(got[:, :J], want), (P, float(np.nanmax(np.abs(got[:, :J] - want))))
    assert not np.any(got[:, J:])


@pytest.mark.parametrize("B", [1, 2, 4])
def test_fused_zspectrum_vs_oracle_cubes(dev, B):
    """(d) sp3d_unproject_fwd_zdft at 80 x 80 x 20 against zdft_fwd_cl of the oracle's whole-volume cubes (same z-DFT code,
    so the difference is the cubes' fp32 rounding carried through a 28-point transform) and against numpy's float64 rfft"""
    from selfpose3d_amd import _lib
    from selfpose3d_amd import synthetic as syn
    J, cube, SZ = 15, (80, 80, 20), 28
    X, Y, Z = cube
    meta, hms, cam, centers = _scene(B, J, 850 + B)
    valid = np.ones(B, np.uint8)
    views = _views(dev, hms, 16)
    args = (torch.from_numpy(cam).to(dev), torch.from_numpy(centers).to(dev), torch.from_numpy(valid).to(dev))
    poison_free_blocks(dev)
    spec = _lib.unproject_fwd_zdft(views, 16, *args, B, J, HM[1], HM[0], cube, syn.SPACE_SIZE, IMG, SZ)
    torch.cuda.synchronize(dev)
    got = spec.view(B, J, SZ // 2 + 1, X // 4, Y // 4, 4, 4).permute(0, 1, 2, 3, 5, 4, 6).reshape(B, J, SZ // 2 + 1, X, Y)
    want_c = _oracle(hms, cam, centers, valid, syn.SPACE_SIZE, cube)
    oc = torch.zeros((B, X, Y, Z, 16), device=dev)
    oc[..., :J] = torch.from_numpy(want_c).to(dev).permute(0, 2, 3, 4, 1)
    ref = _lib.zdft_fwd_cl(oc.permute(0, 4, 1, 2, 3), J, (88, 88, SZ))[..., :X, :Y]
    d = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    assert scale > 10.0
    assert d <= 1e-6 * scale, (B, d, scale)
    f64 = np.fft.rfft(want_c.astype(np.float64), n=SZ, axis=4).transpose(0, 1, 4, 2, 3)
    d64 = float(np.abs(got.cpu().numpy() - f64).max())
    assert d64 <= 2e-6 * scale, (B, d64, scale)
