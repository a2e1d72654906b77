"""Cases and CPU reference of the randomised backward sweep (tests/test_bwd_sweep_reference.py pins this side on the CPU,
tests/test_gpu_bwd_random_sweep.py compares every device form of the unprojection backward and the pass mask of the
training forward against it).  Plain helper module: no pytest hooks, no GPU, every input generated from fixed seeds.

A case is (P, B, V, J, (w, h), cube, grid): P cubes over B samples (sample_of: identity when P == B, random otherwise),
V views, J joints, a w x h heat-map of a 4w x 4h image, and a grid that is
  "space"        the 8000 x 8000 x 2000 mm root grid at SPACE_CENTER,
  "fine"         a cube of 500..3000 mm edge at a random centre per cube,
  ("pitch", mm)  grid size = pitch * (cube - 1) at a random centre per cube (<= 50 mm: SCATTER_AUTO picks the merge).
The oracle has no sample_of: it is called on the gathered batch (hms[c][sample_of], cam[sample_of]) of P samples and its P
gradient rows are added into their B samples in float64.
"""
import functools
import math

import numpy as np

FIXED = [  # (P, B, V, J, (w, h), cube, grid)
    (1, 1, 1, 1, (2, 2), (1, 1, 1), "fine"),                           # one voxel on a 2x2 map
    (2, 2, 16, 16, (9, 7), (5, 3, 7), "space"),                        # V = 16, J = 16: thousands of taps per pixel
    (2, 2, 5, 15, (96, 72), (17, 13, 9), "space"),
    (2, 2, 7, 4, (5, 64), (4, 4, 33), "fine"),                         # 5 pixels wide, Z = 33
    (3, 3, 4, 12, (40, 30), (19, 18, 23), ("pitch", 40.0)),            # dense, ragged block counts on all three axes
    (5, 2, 5, 15, (240, 128), (20, 18, 13), ("pitch", 32.0)),          # the person-cube pitch, P = 5 over B = 2
    (1, 1, 3, 7, (480, 256), (16, 16, 8), ("pitch", 100.0)),           # a block's footprint far above one patch window
    (4, 4, 2, 9, (33, 17), (8, 8, 4), "space"),
    (7, 3, 10, 15, (48, 36), (9, 10, 11), "fine"),                     # P = 7 over B = 3
    (2, 2, 3, 17, (16, 12), (8, 8, 4), "space"),                       # J > 16: planar kernel only
    (3, 2, 2, 20, (33, 17), (6, 6, 6), "fine"),
]
NUM_RANDOM = 16
EXTRA = [  # appended after the random cases, so that those keep their indices (the index seeds a case's inputs)
    (4, 2, 3, 8, (31, 22), (6, 5, 32), ("pitch", 45.0)),               # Z % 32 == 0: the planar training forward takes the brick kernel
]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(2025)
    out = list(FIXED)
    for _ in range(NUM_RANDOM):
        B = int(rng.integers(1, 5))
        P = B if rng.random() < 0.5 else int(rng.integers(1, 7))
        kind = ["space", "fine", ("pitch", float(rng.uniform(15, 60)))][int(rng.integers(3))]
        out.append((P, B, int(rng.integers(1, 9)), int(rng.integers(1, 17)), (int(rng.integers(2, 80)), int(rng.integers(2, 60))),
                    (int(rng.integers(1, 20)), int(rng.integers(1, 20)), int(rng.integers(1, 24))), kind))
    return tuple(out + EXTRA)


def case_id(idx):
    P, B, V, J, (w, h), cube, kind = cases()[idx]
    k = kind if isinstance(kind, str) else "pitch%g" % round(kind[1], 1)
    return "%02d-P%dB%dV%dJ%d-%dx%d-%dx%dx%d-%s" % (idx, P, B, V, J, w, h, cube[0], cube[1], cube[2], k)


def channel_strides(idx, J):
    """packed channel strides a case runs at: the smallest of 4 / 8 / 12 / 16 that holds J, and 16 as well on every third case
    with J <= 12 (pad channels beyond the smallest stride); none for J > 16"""
    if J > 16:
        return []
    jp = 4 * ((J + 3) // 4)
    return [jp, 16] if (idx % 3 == 0 and J <= 12) else [jp]


def auto_takes_merge(cube, grid_size):
    """the rule of include/sp3d.h for SP3D_SCATTER_AUTO: pitch <= 50 mm on every axis (and at least 2 voxels on each)"""
    return all(c >= 2 for c in cube) and all(float(g) / (c - 1) <= 50.0 for g, c in zip(grid_size, cube))


class Case:
    """inputs of one case (numpy, host) and, lazily, its CPU reference"""

    def __init__(self, idx):
        import torch
        from selfpose3d_amd import synthetic as syn
        from selfpose3d_amd.camera_pack import pack_cameras
        self.idx = idx
        P, B, V, J, (w, h), cube, kind = cases()[idx]
        self.P, self.B, self.V, self.J, self.w, self.h, self.cube, self.kind = P, B, V, J, w, h, tuple(cube), kind
        self.N = cube[0] * cube[1] * cube[2]
        rng = np.random.default_rng(5000 + idx)
        self.img = img = (w * 4, h * 4)
        meta = syn.random_meta(B, V, img, seed=100 + idx, augment=(idx % 2 == 0), ssv_style=(idx % 3 == 0))
        flip = torch.from_numpy(rng.random(B) < 0.4) if idx % 2 == 0 else None
        self.cam = pack_cameras(meta, B, img, flip)
        self.hms = [(rng.random((B, J, h, w), dtype=np.float32) * 1.6 - 0.3) for _ in range(V)]     # the clamp blocks on both sides
        self.sample_of = (np.arange(P) % B if P == B else rng.integers(0, B, P)).astype(np.int32)
        if kind == "space":
            self.centers = np.repeat(np.asarray([syn.SPACE_CENTER], np.float32), P, 0)
            self.grid_size = [float(s) for s in syn.SPACE_SIZE]
        else:
            self.centers = np.stack([rng.uniform(-1500, 1500, P), rng.uniform(-2000, 1000, P), rng.uniform(200, 1500, P)],
                                    1).astype(np.float32)
            self.grid_size = [float(rng.uniform(500, 3000))] * 3 if kind == "fine" else [kind[1] * max(c - 1, 1) for c in cube]
        self.valid = (rng.random(P) < 0.8).astype(np.uint8)
        self.valid[0] = 1
        # channels of very different magnitude, as tests/test_gpu_bwd_merge.py::_setup
        self.grad = (rng.standard_normal((P, J, *cube)) * np.exp(rng.uniform(-6, 3, (P, J, 1, 1, 1)))).astype(np.float32)
        # gathered batch of P samples for the oracle
        self.hms_p = [x[self.sample_of] for x in self.hms]
        self.cam_p = self.cam.reshape(B, V, 64)[self.sample_of]
        self.cubes_per_sample = np.bincount(self.sample_of, minlength=B)
        self.owns_valid = np.bincount(self.sample_of, weights=self.valid, minlength=B) > 0      # samples with a valid cube
        # additions a pixel can receive: 4 taps of every voxel of every cube on its sample
        self.T = 4 * self.N * int(self.cubes_per_sample.max())
        # one step of the deterministic forms' fixed point (_lib.unproject_bwd_packed: scale = 2^(40 - ceil(log2 max|g|)))
        self.det_step = 2.0 ** (math.ceil(math.log2(float(np.abs(self.grad).max()))) - 40)
        self.border = np.zeros((h, w), bool)
        self.border[[0, -1]] = True
        self.border[:, [0, -1]] = True

    # ---- CPU reference -------------------------------------------------------------------------------------------
    def oracle_fwd(self, hms_p):
        from oracle import oracle
        return oracle.unproject_fwd(hms_p, self.cam_p, self.centers, self.valid, self.grid_size, self.cube, self.img,
                                    want_grids=False)[0]

    def oracle_bwd_rows(self, hms_p, grad):
        """(V, P, J, h, w) float64: the oracle's gradient rows of the gathered batch"""
        from oracle import oracle
        return np.stack(oracle.unproject_bwd(hms_p, self.cam_p, self.centers, self.valid, grad, self.grid_size, self.cube,
                                             self.img))

    def to_samples(self, rows):
        """add the P gradient rows into their B samples (float64)"""
        out = np.zeros((self.V, self.B) + rows.shape[2:], np.float64)
        np.add.at(out, (slice(None), self.sample_of), rows)
        return out

    @functools.cached_property
    def fwd(self):
        """(P, J, X, Y, Z) float32: the oracle's forward"""
        return self.oracle_fwd(self.hms_p)

    @functools.cached_property
    def fwd_quarter(self):
        return self.oracle_fwd([0.25 * x for x in self.hms_p])

    @functools.cached_property
    def fwd_negated(self):
        return self.oracle_fwd([-0.25 * x for x in self.hms_p])

    @functools.cached_property
    def seen(self):
        """(P, X, Y, Z) bool: at least one view sees the voxel (all-ones maps give a positive value exactly there)"""
        return self.oracle_fwd([np.ones_like(x) for x in self.hms_p])[:, 0] > 0

    @functools.cached_property
    def expected_pass(self):
        """(P, J, X, Y, Z) bool: the pass bit, from the oracle's forward alone.  Scaling the maps by a power of two commutes
        with every fp32 rounding of the forward, so with q = fwd(hm / 4) and m = fwd(-hm / 4):  pre > 1 <=> 4 q > 1  and
        pre < 0 <=> m > 0  (tests/test_bwd_sweep_reference.py proves both per case)."""
        ok = self.valid[:, None, None, None, None] > 0
        return ok & ~(4.0 * self.fwd_quarter > 1.0) & ~(self.fwd_negated > 0.0)

    @functools.cached_property
    def expected_mask(self):
        """(P, N) uint16 words as sp3d_unproject_fwd_train writes them (J <= 16: the packed forms' limit)"""
        assert self.J <= 16
        bits = self.expected_pass.reshape(self.P, self.J, self.N).astype(np.uint32)
        word = np.zeros((self.P, self.N), np.uint32)
        for j in range(self.J):
            word |= bits[:, j] << j
        return word.astype(np.uint16)

    @functools.cached_property
    def ref(self):
        """(V, B, J, h, w) float64: the reference gradient"""
        return self.to_samples(self.oracle_bwd_rows(self.hms_p, self.grad))

    @functools.cached_property
    def S(self):
        """(V, B, J, h, w) float64: per pixel the sum of the absolute contributions (tap weights are non-negative)"""
        return self.to_samples(self.oracle_bwd_rows(self.hms_p, np.abs(self.grad)))

    def largest_block_footprint(self):
        """pixels of the largest bounding rectangle that an 8x8x4 block of voxels of a valid cube has in one view (an estimate
        from the projected voxel centres, the crop affine and the stride of 4; the merge kernel windows it by 256 pixels)"""
        from oracle import oracle
        ax = [oracle.linspace(self.grid_size[i], self.cube[i]) for i in range(3)]
        best = 0.0
        for p in np.flatnonzero(self.valid):
            for bx in range(0, self.cube[0], 8):
                for by in range(0, self.cube[1], 8):
                    for bz in range(0, self.cube[2], 4):
                        X, Y, Z = np.meshgrid(ax[0][bx:bx + 8], ax[1][by:by + 8], ax[2][bz:bz + 4], indexing="ij")
                        pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1) + self.centers[p]
                        for c in range(self.V):
                            px = oracle.project_points(self.cam_p[p, c], pts).astype(np.float64)
                            A = self.cam_p[p, c, 21:27].reshape(2, 3).astype(np.float64)
                            q = (px @ A[:, :2].T + A[:, 2]) / 4.0
                            inb = (q[:, 0] >= 0) & (q[:, 0] <= self.w - 1) & (q[:, 1] >= 0) & (q[:, 1] <= self.h - 1)
                            if inb.sum() < 2:
                                continue
                            qq = np.floor(q[inb])
                            best = max(best, (qq[:, 0].max() - qq[:, 0].min() + 2) * (qq[:, 1].max() - qq[:, 1].min() + 2))
        return best


@functools.lru_cache(maxsize=None)
def get(idx):
    return Case(idx)
