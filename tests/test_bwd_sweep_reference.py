"""The reference side of the randomised backward sweep (tests/bwd_sweep_cases.py), pinned on the CPU so that
tests/test_gpu_bwd_random_sweep.py compares the device against something that was itself checked:
  * the exact pass mask derived from the oracle's FORWARD alone (power-of-two scalings of the heat-maps) is the mask the
    oracle's BACKWARD applies: the two gradients are array-equal in float64;
  * S, the per-pixel sum of absolute contributions that scales the GPU test's error bounds, dominates |reference|;
  * the cases reach what they are there for (non-zero gradients, border pixels, unseen voxels, the clamp on both sides,
    blocks whose footprint in a view needs several patch windows of the merge kernel) - conditions on the reference only.
"""
import numpy as np
import pytest

from tests import bwd_sweep_cases as sweep

CASES = list(range(len(sweep.cases())))


def test_case_list_is_the_fixed_one():
    cs = sweep.cases()
    assert len(cs) == 28 and list(cs[:11]) == sweep.FIXED and list(cs[27:]) == sweep.EXTRA
    assert cs == sweep.cases.__wrapped__()                                      # generated from a fixed seed
    assert sum(1 for c in cs if c[3] > 16) == 2 and sum(1 for c in cs if c[0] != c[1]) >= 5
    strides = [jp for idx, c in enumerate(cs) for jp in sweep.channel_strides(idx, c[3])]
    assert {4, 8, 12, 16} <= set(strides) and len(strides) > sum(1 for c in cs if c[3] <= 16)   # some cases at two strides


@pytest.mark.parametrize("idx", CASES, ids=sweep.case_id)
def test_pass_mask_from_the_forward_is_the_backwards_own(idx):
    c = sweep.get(idx)
    o = c.fwd
    inside = (o > 0) & (o < 1)
    # scaling by 1/4 commutes with every rounding: 4 q is the forward itself wherever the clamp did not act
    assert np.array_equal((4.0 * c.fwd_quarter)[inside], o[inside])
    exp = c.expected_pass
    assert np.all(exp[inside]) and not exp[c.valid == 0].any()
    # a voxel that no view sees has pre = 0, which is inside [0, 1]: its bit is set (and reaches no gradient)
    unseen = ~c.seen & (c.valid[:, None, None, None] > 0)
    assert np.all(exp.transpose(1, 0, 2, 3, 4)[:, unseen]) and not o.transpose(1, 0, 2, 3, 4)[:, unseen].any()
    # with all-zero maps every voxel passes: the oracle's backward of (zero maps, grad * mask) equals its backward of
    # (maps, grad) exactly iff the derived mask is the one the oracle applies
    ref_rows = c.oracle_bwd_rows(c.hms_p, c.grad)
    alt_rows = c.oracle_bwd_rows([np.zeros_like(x) for x in c.hms_p], c.grad * exp)
    assert ref_rows.dtype == np.float64 and np.array_equal(ref_rows, alt_rows)
    assert np.array_equal(c.to_samples(ref_rows), c.ref)
    # the mask words of sp3d_unproject_fwd_train: bit j = channel j, nothing at or above J
    if c.J > 16:
        return
    m = c.expected_mask
    assert m.dtype == np.uint16 and m.shape == (c.P, c.N)
    for j in range(c.J):
        assert np.array_equal(((m >> j) & 1).astype(bool), exp[:, j].reshape(c.P, c.N))
    assert not (m.astype(np.uint32) >> c.J).any()


@pytest.mark.parametrize("idx", CASES, ids=sweep.case_id)
def test_sum_of_absolute_contributions_bounds_the_reference(idx):
    c = sweep.get(idx)
    assert c.S.shape == c.ref.shape == (c.V, c.B, c.J, c.h, c.w)
    assert np.all(c.S >= np.abs(c.ref))
    assert not c.S[:, ~c.owns_valid].any()                                      # samples that own no valid cube get nothing
    assert c.T >= 4 * c.N and c.det_step >= 2.0 ** -40 * float(np.abs(c.grad).max()) > c.det_step / 2


def test_sweep_is_not_vacuous():
    nonzero = border = unseen = blocked = 0
    for idx in CASES:
        c = sweep.get(idx)
        nz = c.ref != 0
        nonzero += bool(nz.any())
        border += bool(nz[..., c.border].any())
        ok = c.valid > 0
        unseen += bool((~c.seen[ok]).any())
        blocked += bool(1.0 - c.expected_pass[ok].mean() > 1e-3)
    assert nonzero >= 25, nonzero
    assert border >= 20, border
    assert unseen >= 8, unseen
    assert blocked >= 15, blocked
    # samples that own no valid cube, invalid cubes, P != B: each present more than once
    assert sum(1 for i in CASES if not sweep.get(i).owns_valid.all()) >= 2
    assert sum(1 for i in CASES if not sweep.get(i).valid.all()) >= 5


def test_some_blocks_need_several_patch_windows():
    """the merge kernel merges a block's taps per view in windows of 256 pixels: at least two cases have an 8x8x4 block whose
    bounding rectangle in some view is larger (dense cases only: they are the ones a merge is built for)"""
    big = {}
    for idx in CASES:
        if isinstance(sweep.cases()[idx][6], tuple):
            big[idx] = sweep.get(idx).largest_block_footprint()
    assert sum(1 for v in big.values() if v > 256) >= 2, big
    assert big[6] > 50 * 256 and 256 < big[5] < 4 * 256 and big[4] <= 256, big   # hundreds of windows / two or three / one
