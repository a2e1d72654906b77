"""Host side of the pooled forms of the two residual convs (SP3D_CONV3_POOL2X on the CS of sp3d_conv3_split_skip and of
sp3d_wino_fused_split64_skip): the flag, the refusals of the C entries before anything reaches the GPU runtime (no GPU needed:
every call below is refused, the dummy pointers are never dereferenced), the coverage predicate, the buffer convention of the
bindings and the plan's hand-over from _res to _pool.

The exported set and the ABI version are pinned (tests/test_host_cabi.py), so the form is a flag bit, as SP3D_CONV3_WINO_YZ is."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_host_cabi import ROOT

OK, EINVAL, ENULL, ERANGE, EUNSUPPORTED = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from selfpose3d_amd import _lib, build as sbuild
    sbuild.build()
    return _lib.load()


def test_flag_is_the_headers_and_collides_with_nothing():
    from selfpose3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sp3d.h")).read()
    m = re.search(r"#define\s+SP3D_CONV3_POOL2X\s+(0x[0-9a-fA-F]+)", hdr)
    assert m and int(m.group(1), 16) == _lib.CONV3_POOL2X == 0x200
    assert _lib.CONV3_POOL2X & _lib.CONV3_WINO_YZ == 0
    assert _lib.CONV3_POOL2X & (16 | 32) == 0                            # disjoint from the skip widths it rides on
    assert _lib.ABI_VERSION == 3


def test_flagged_calls_refuse_before_any_launch(lib):
    from selfpose3d_amd import _lib
    P, YZ = _lib.CONV3_POOL2X, _lib.CONV3_WINO_YZ
    d, off4 = C.c_void_p(0x1000), C.c_void_p(0x1004)

    def direct(x=d, w=d, y=d, shift=d, xs=d, ws=d, B=1, X=16, Y=8, Z=4, Cin=32, O=32, CS=16, flag=P):
        return lib.sp3d_conv3_split_skip(x, w, y, shift, xs, ws, B, X, Y, Z, Cin, O, CS | flag, None)

    def wino(x=d, w=d, y=d, shift=d, xs=d, ws=d, B=1, X=8, Y=8, Z=2, Cin=64, O=64, CS=32, flag=P):
        return lib.sp3d_wino_fused_split64_skip(x, w, y, shift, xs, ws, B, X, Y, Z, Cin, O, CS | flag, None)

    # a grid that is not whole blocks: refused with the flag, in every axis
    for kw in (dict(X=20), dict(X=24), dict(Y=12), dict(Z=6), dict(X=40, Y=40, Z=10), dict(X=48, Y=48, Z=10), dict(X=15), dict(Z=3)):
        assert direct(**kw) == EUNSUPPORTED, kw
    for kw in (dict(X=12), dict(Y=10), dict(Z=3), dict(X=9, Y=9, Z=9)):
        assert wino(**kw) == EUNSUPPORTED, kw
        assert wino(flag=P | YZ, **kw) == EUNSUPPORTED, kw
    for f in (direct, wino):
        for dim in ("B", "X", "Y", "Z"):
            assert f(**{dim: 0}) == EINVAL and f(**{dim: -1}) == EINVAL, dim
        for ptr in ("x", "w", "y", "shift", "xs", "ws"):
            assert f(**{ptr: None}) == ENULL, ptr
        assert f(xs=off4) == EUNSUPPORTED and f(ws=off4) == EUNSUPPORTED
        # the order of the rules is that of the calls without the flag
        assert f(B=0, x=None, O=48) == EINVAL
        assert f(x=None, O=48) == ENULL and f(x=None, X=20, Z=3) == ENULL
    # a wrong CS under the flag
    assert direct(CS=32) == EUNSUPPORTED and direct(CS=8) == EUNSUPPORTED and direct(CS=0) == EUNSUPPORTED
    assert wino(CS=16) == EUNSUPPORTED and wino(CS=64) == EUNSUPPORTED and wino(CS=0) == EUNSUPPORTED
    assert direct(flag=P | YZ) == EUNSUPPORTED                           # the direct kernel has no y,z form
    assert direct(flag=P | 0x400) == EUNSUPPORTED and wino(flag=P | 0x400) == EUNSUPPORTED
    assert direct(Cin=16) == EUNSUPPORTED and direct(O=64) == EUNSUPPORTED and wino(Cin=32) == EUNSUPPORTED
    # the range rule behind a whole grid
    assert direct(X=4096, Y=4096, Z=4) == ERANGE and wino(X=4096, Y=4096, Z=4) == ERANGE
    assert wino(flag=P | YZ, X=4096, Y=4096, Z=4) == ERANGE


def test_unflagged_calls_answer_as_before(lib):
    """the table of tests/test_host_cabi.py and tests/test_wino_yz_host.py for the two entries, flag off: a ragged grid is no
    refusal there (the first failing rule of these calls is a later one), everything else is what it was"""
    from selfpose3d_amd import _lib
    YZ = _lib.CONV3_WINO_YZ
    d, off4 = C.c_void_p(0x1000), C.c_void_p(0x1004)
    big = dict(B=1 << 20, X=1024, Y=1024, Z=1024)

    def direct(x=d, w=d, y=d, shift=d, xs=d, ws=d, B=1, X=8, Y=8, Z=8, Cin=32, O=32, CS=16):
        return lib.sp3d_conv3_split_skip(x, w, y, shift, xs, ws, B, X, Y, Z, Cin, O, CS, None)

    def wino(x=d, w=d, y=d, shift=d, xs=d, ws=d, B=1, X=8, Y=8, Z=8, Cin=64, O=64, CS=32):
        return lib.sp3d_wino_fused_split64_skip(x, w, y, shift, xs, ws, B, X, Y, Z, Cin, O, CS, None)

    for f in (direct, wino):
        for dim in ("B", "X", "Y", "Z"):
            assert f(**{dim: 0}) == EINVAL and f(**{dim: -1}) == EINVAL, dim
        for ptr in ("x", "w", "y", "shift", "xs", "ws"):
            assert f(**{ptr: None}) == ENULL, ptr
        assert f(xs=off4) == EUNSUPPORTED and f(ws=off4) == EUNSUPPORTED and f(w=off4, **big) == EUNSUPPORTED
        assert f(**big) == ERANGE
        # ragged grids pass every rule up to the range check without the flag
        assert f(X=4095, Y=4097, Z=5, B=1 << 10) == ERANGE and f(x=None, X=13, Y=7, Z=3) == ENULL
    assert direct(CS=32) == EUNSUPPORTED and direct(CS=16 | YZ) == EUNSUPPORTED and wino(CS=16) == EUNSUPPORTED
    assert wino(CS=32 | YZ, X=4096, Y=4096, Z=4) == ERANGE and wino(CS=64 | YZ) == EUNSUPPORTED
    # no other entry takes the bit
    for name in ("sp3d_wino_fused", "sp3d_wino_fused_split", "sp3d_wino_fused_split64", "sp3d_conv3_split"):
        assert getattr(lib, name)(d, d, d, d, None, _lib.CONV3_POOL2X, 1, 8, 8, 8, 32, 32, None) == EINVAL, name


def test_pool_fold_covers():
    from selfpose3d_amd import _lib
    cov = _lib.pool_fold_covers
    assert cov("conv3_split_", 80, 80, 20) and cov("conv3_split_", 64, 64, 64) and cov("conv3_split_", 16, 8, 4)
    assert cov("wino_fused_conv3d_", 40, 40, 10) and cov("wino_fused_conv3d_", 32, 32, 32) and cov("wino_fused_conv3d_", 8, 8, 2)
    # 48x48x12 IS whole 16x8x4 blocks (3 x 6 x 3), so the rule "whole blocks" covers it; the ragged grids next to it are not
    assert cov("conv3_split_", 48, 48, 12)
    assert not cov("conv3_split_", 48, 48, 10) and not cov("conv3_split_", 40, 48, 12) and not cov("conv3_split_", 48, 44, 12)
    assert not cov("conv3_split_", 40, 40, 10) and not cov("conv3_split_", 80, 80, 18) and not cov("conv3_split_", 80, 84, 20)
    assert cov("wino_fused_conv3d_", 24, 24, 6) and not cov("wino_fused_conv3d_", 20, 20, 5)
    for odd in ((15, 8, 4), (16, 7, 4), (16, 8, 3), (81, 80, 20)):
        assert not cov("conv3_split_", *odd), odd
    for odd in ((7, 8, 2), (8, 9, 2), (8, 8, 1), (41, 40, 10)):
        assert not cov("wino_fused_conv3d_", *odd), odd
    for route in ("conv3_split128_", "wino_conv3d_", "library", ""):
        assert not cov(route, 80, 80, 20) and not cov(route, 64, 64, 64), route
    assert not cov("conv3_split_", 0, 8, 4) and not cov("wino_fused_conv3d_", 8, 8, 0)


def test_covers_is_what_the_entries_accept(lib):
    """predicate and C entries agree on every small grid: the flagged call of a grid the predicate covers passes the grid rule
    (it is refused later, for a misaligned pointer), one it does not cover is never launched"""
    from selfpose3d_amd import _lib
    P = _lib.CONV3_POOL2X
    d = C.c_void_p(0x1000)
    for X in range(1, 34):
        for Y, Z in ((8, 4), (16, 2), (12, 6), (7, 3)):
            rd = lib.sp3d_conv3_split_skip(None, d, d, d, d, d, 1, X, Y, Z, 32, 32, 16 | P, None)
            rw = lib.sp3d_wino_fused_split64_skip(None, d, d, d, d, d, 1, X, Y, Z, 64, 64, 32 | P, None)
            assert rd == ENULL and rw == ENULL                           # the pointer rule comes first: nothing is launched
            rd = lib.sp3d_conv3_split_skip(d, d, d, d, d, d, 1 << 20, X, Y * 512, Z * 512, 32, 32, 16 | P, None)
            # (2^30 samples of at least two blocks: more blocks than a launch takes, the range rule behind the grid rule)
            rw = lib.sp3d_wino_fused_split64_skip(d, d, d, d, d, d, 1 << 30, X, Y, Z, 64, 64, 32 | P, None)
            assert rd == (ERANGE if _lib.pool_fold_covers("conv3_split_", X, Y * 512, Z * 512) else EUNSUPPORTED), (X, Y, Z)
            assert rw == (ERANGE if _lib.pool_fold_covers("wino_fused_conv3d_", X, Y, Z) else EUNSUPPORTED), (X, Y, Z)


def test_switch(monkeypatch):
    from selfpose3d_amd import _lib
    monkeypatch.delenv("SP3D_FOLD_POOL", raising=False)
    assert _lib.pool_fold_enabled() == _lib.POOL_FOLD_DEFAULT
    monkeypatch.setenv("SP3D_FOLD_POOL", "0")
    assert not _lib.pool_fold_enabled()
    monkeypatch.setenv("SP3D_FOLD_POOL", "1")
    assert _lib.pool_fold_enabled()


def test_one_buffer_two_views():
    from selfpose3d_amd import _lib
    x = torch.zeros(2, 32, 16, 8, 4).contiguous(memory_format=torch.channels_last_3d)
    n, npool = 2 * 16 * 8 * 4 * 32, 2 * 8 * 4 * 2 * 32
    y, yp = _lib._result_pooled(None, 2, 32, 16, 8, 4, x, "t")
    assert tuple(y.shape) == (2, 32, 16, 8, 4) and tuple(yp.shape) == (2, 32, 8, 4, 2)
    assert y.is_contiguous(memory_format=torch.channels_last_3d) and yp.is_contiguous(memory_format=torch.channels_last_3d)
    assert yp.data_ptr() == y.data_ptr() + 4 * n                          # the pooled tensor directly behind the full one
    buf = torch.empty(n + npool)
    y, yp = _lib._result_pooled(buf, 2, 32, 16, 8, 4, x, "t")
    assert y.data_ptr() == buf.data_ptr() and yp.data_ptr() == buf.data_ptr() + 4 * n
    for bad in (torch.empty(n + npool + 1), torch.empty(n), torch.empty(n + npool, dtype=torch.float64),
                torch.empty(2, (n + npool) // 2), torch.empty(2 * (n + npool))[::2]):
        with pytest.raises(_lib.Sp3dError):
            _lib._result_pooled(bad, 2, 32, 16, 8, 4, x, "t")


def test_maxpool2x_have_is_checked_and_returned():
    from selfpose3d_amd import _lib
    cl = torch.channels_last_3d
    x = torch.zeros(2, 8, 4, 6, 2).contiguous(memory_format=cl)
    have = torch.ones(2, 8, 2, 3, 1).contiguous(memory_format=cl)
    assert _lib.maxpool2x(x, have=have) is have                          # no launch: these tensors live on the CPU
    for bad in (torch.ones(2, 8, 2, 3, 2).contiguous(memory_format=cl), torch.ones(2, 4, 2, 3, 1).contiguous(memory_format=cl),
                have.double(), torch.ones(2, 8, 4, 3, 1).contiguous(memory_format=cl)[:, :, ::2],
                torch.ones(2, 8, 2, 3, 1, device="meta")):
        with pytest.raises(_lib.Sp3dError):
            _lib.maxpool2x(x, have=bad)


class _Stub:
    """what _pool looks at in a tensor, without one"""

    def __init__(self, shape=(1, 32, 16, 8, 4)):
        self.shape, self.is_cuda, self.dtype = shape, True, torch.float32

    def is_contiguous(self, memory_format=torch.contiguous_format):
        return memory_format == torch.channels_last_3d


def test_pool_takes_the_stash_only_for_the_identical_tensor(monkeypatch):
    from selfpose3d_amd import _lib
    from selfpose3d_amd.v2v_net import V2VNet, _FoldedV2V, _Res
    assert "pooled" in _Res._fields and _Res(None, None, None).pooled is False
    plan = _FoldedV2V(V2VNet(15, 1))
    assert plan.pooled is None
    calls = []

    def fake(x, have=None):
        calls.append((x, have))
        return have if have is not None else "launched"
    monkeypatch.setattr(_lib, "maxpool2x", fake)
    y, yp, other = _Stub(), _Stub((1, 32, 8, 4, 2)), _Stub()
    plan.pooled = (y, yp)
    assert plan._pool(y) is yp and calls[-1] == (y, yp) and plan.pooled is None
    assert plan._pool(y) == "launched" and calls[-1] == (y, None)        # used once
    plan.pooled = (y, yp)
    assert plan._pool(other) == "launched" and calls[-1] == (other, None) and plan.pooled is None     # equal is not identical
    assert len(calls) == 3                                               # one call of maxpool2x per _pool


def test_build_marks_the_two_blocks_the_tail_pools():
    from selfpose3d_amd.v2v_net import V2VNet
    plan = V2VNet(15, 1).eval()._get_plan()
    plan._ensure_built()
    marked = {name for name, r in plan.layers.items() if getattr(r, "pooled", False)}
    assert marked == {"front_res", "encoder_res1"}
