"""Cases of the one-channel training pair (sp3d_unproject_one_fwd_train / sp3d_unproject_one_bwd[_det]): every case of
tests/bwd_sweep_cases.py seen as a ONE-channel case, plus one case of its own with V = 12 (the 12-view-slot instantiation of
the one-channel kernel has no sweep case).  Plain helper module: no pytest hooks, no GPU.

Channel rid = idx % J of a case's (B,J,h,w) maps is the "channel of a wider tensor".  The unprojection treats channels
independently, so the reference is that channel of the case's own arrays - fwd[:, rid], expected_pass[:, rid] as bit 0,
ref[:, :, rid], S[:, :, rid] - and only grad[:, rid] is given (tests/test_one_channel_grad_host.py proves the slicing on the
oracle).  T is unchanged; det_step is recomputed from max|grad[:, rid]| (the binding builds the scale from the one channel).
"""
import functools
import math

import numpy as np

from tests import bwd_sweep_cases as sweep

OWN_IDX = 100                                                   # index (= seed) of the V = 12 case, outside the sweep's range
OWN = (3, 2, 12, 3, (37, 23), (7, 9, 10), "space")             # (P, B, V, J, (w, h), cube, grid), as a sweep case


class _OwnCase(sweep.Case):
    """a sweep Case for a specification that is not in sweep.cases(): the recipe of sweep.Case.__init__, statement for
    statement, with `spec` in the place of cases()[idx]"""

    def __init__(self, idx, spec):
        import torch
        from selfpose3d_amd import synthetic as syn
        from selfpose3d_amd.camera_pack import pack_cameras
        self.idx = idx
        P, B, V, J, (w, h), cube, kind = spec
        self.P, self.B, self.V, self.J, self.w, self.h, self.cube, self.kind = P, B, V, J, w, h, tuple(cube), kind
        self.N = cube[0] * cube[1] * cube[2]
        rng = np.random.default_rng(5000 + idx)
        self.img = img = (w * 4, h * 4)
        meta = syn.random_meta(B, V, img, seed=100 + idx, augment=(idx % 2 == 0), ssv_style=(idx % 3 == 0))
        flip = torch.from_numpy(rng.random(B) < 0.4) if idx % 2 == 0 else None
        self.cam = pack_cameras(meta, B, img, flip)
        self.hms = [(rng.random((B, J, h, w), dtype=np.float32) * 1.6 - 0.3) for _ in range(V)]
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
        self.grad = (rng.standard_normal((P, J, *cube)) * np.exp(rng.uniform(-6, 3, (P, J, 1, 1, 1)))).astype(np.float32)
        self.hms_p = [x[self.sample_of] for x in self.hms]
        self.cam_p = self.cam.reshape(B, V, 64)[self.sample_of]
        self.cubes_per_sample = np.bincount(self.sample_of, minlength=B)
        self.owns_valid = np.bincount(self.sample_of, weights=self.valid, minlength=B) > 0
        self.T = 4 * self.N * int(self.cubes_per_sample.max())
        self.det_step = 2.0 ** (math.ceil(math.log2(float(np.abs(self.grad).max()))) - 40)
        self.border = np.zeros((h, w), bool)
        self.border[[0, -1]] = True
        self.border[:, [0, -1]] = True


def indices():
    """every index of the sweep, then the V = 12 case"""
    return list(range(len(sweep.cases()))) + [OWN_IDX]


def case_id(idx):
    if idx != OWN_IDX:
        return sweep.case_id(idx)
    P, B, V, J, (w, h), cube, kind = OWN
    return "%02d-P%dB%dV%dJ%d-%dx%d-%dx%dx%d-%s" % (idx, P, B, V, J, w, h, cube[0], cube[1], cube[2], kind)


@functools.lru_cache(maxsize=None)
def base(idx):
    """the J-channel sweep case behind a one-channel case (shared with the sweep's own tests: one reference per case)"""
    return sweep.get(idx) if idx != OWN_IDX else _OwnCase(OWN_IDX, OWN)


class OneCase:
    """channel rid of a sweep case as a case with J = 1; the attributes tests/test_gpu_bwd_random_sweep.py's checks read
    (ref, S, T, owns_valid, det_step, ...) are the one channel's"""

    def __init__(self, idx):
        b = self.base = base(idx)
        self.idx, self.rid, self.Jt, self.J = idx, idx % b.J, b.J, 1
        for k in ("P", "B", "V", "w", "h", "cube", "kind", "N", "img", "cam", "sample_of", "centers", "grid_size", "valid",
                  "cam_p", "cubes_per_sample", "owns_valid", "T", "border", "hms"):
            setattr(self, k, getattr(b, k))
        r = self.rid
        self.grad = np.ascontiguousarray(b.grad[:, r:r + 1])                                     # (P,1,X,Y,Z)
        self.det_step = 2.0 ** (math.ceil(math.log2(float(np.abs(self.grad).max()))) - 40)
        self.hms_one = [np.ascontiguousarray(x[:, r:r + 1]) for x in b.hms]                      # the channel, contiguous

    @functools.cached_property
    def fwd(self):
        return np.ascontiguousarray(self.base.fwd[:, self.rid:self.rid + 1])

    @functools.cached_property
    def seen(self):
        return self.base.seen

    @functools.cached_property
    def expected_mask(self):
        """(P, N) uint16: bit 0 = the channel's pass bit, nothing above it, zero rows for invalid cubes"""
        return self.base.expected_pass[:, self.rid].reshape(self.P, self.N).astype(np.uint16)

    @functools.cached_property
    def ref(self):
        return np.ascontiguousarray(self.base.ref[:, :, self.rid:self.rid + 1])

    @functools.cached_property
    def S(self):
        return np.ascontiguousarray(self.base.S[:, :, self.rid:self.rid + 1])


@functools.lru_cache(maxsize=None)
def get(idx):
    return OneCase(idx)
