"""Cases of the 17..32-joint training pair (SP3D_HM_WIDE_MASK / SP3D_SCATTER_WIDE): tests/test_wide_grad_host.py pins the
cases themselves on the CPU, tests/test_gpu_wide_grad.py runs the device forms against them.  Plain helper module: no pytest
hooks, no GPU.

The inputs are those of tests/bwd_sweep_cases.Case - the same class, the same recipe - with idx = 100 + k, so that the seeds
(5000 + idx for the inputs, 100 + idx for the rig) collide with no case of that sweep.  What this module adds is the two-plane
pass mask: plane 0 holds channels 0-15, plane 1 channels 16..J-1, bit (j mod 16) each.
"""
import functools

import numpy as np

from tests import bwd_sweep_cases as sweep

FIRST = 100
WIDE = {  # idx: (P, B, V, J, (w, h), cube, grid)
    100: (1, 1, 1, 17, (2, 2), (1, 1, 1), "fine"),                      # one voxel
    101: (2, 2, 3, 17, (16, 12), (8, 8, 4), "space"),                   # group 1 is one channel
    102: (3, 2, 2, 20, (33, 17), (6, 6, 6), "fine"),                    # P != B
    103: (2, 2, 5, 32, (24, 18), (9, 10, 11), ("pitch", 40.0)),         # both groups full, merge, ragged blocks
    104: (5, 2, 4, 21, (40, 30), (20, 18, 13), ("pitch", 32.0)),        # width 8, merge, an invalid cube
    105: (1, 1, 16, 25, (9, 7), (5, 3, 7), "space"),                    # V = 16, width 12
    106: (4, 2, 3, 29, (31, 22), (6, 5, 32), ("pitch", 45.0)),          # Z % 32 == 0: the brick training forward; a sample that owns no valid cube
    107: (4, 4, 5, 17, (96, 72), (17, 13, 9), "space"),
}
CASES = sorted(WIDE)
GRAPH_CASE = 104


def case_id(idx):
    P, B, V, J, (w, h), cube, kind = WIDE[idx]
    k = kind if isinstance(kind, str) else "pitch%g" % round(kind[1], 1)
    return "%03d-P%dB%dV%dJ%d-%dx%d-%dx%dx%d-%s" % (idx, P, B, V, J, w, h, cube[0], cube[1], cube[2], k)


class WideCase(sweep.Case):
    """sweep.Case built from WIDE[idx] instead of the sweep's own list, plus the two-plane mask"""

    def __init__(self, idx):
        # Case.__init__ looks its tuple up as cases()[idx]: hand it this module's table for the duration of the call
        own = sweep.cases
        sweep.cases = lambda: WIDE
        try:
            super().__init__(idx)
        finally:
            sweep.cases = own

    @functools.cached_property
    def expected_mask_planes(self):
        """(2, P, N) uint16 as sp3d_unproject_fwd_train writes it with SP3D_HM_WIDE_MASK, built from expected_pass"""
        bits = self.expected_pass.reshape(self.P, self.J, self.N).astype(np.uint32)
        planes = np.zeros((2, self.P, self.N), np.uint32)
        for j in range(self.J):
            planes[j // 16] |= bits[:, j] << (j % 16)
        return planes.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def get(idx):
    return WideCase(idx)
