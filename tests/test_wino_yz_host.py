"""Host side of the half-resolution fused Winograd kernel's y,z form (SP3D_CONV3_WINO_YZ on sp3d_wino_fused_split64 and
sp3d_wino_fused_split64_skip): the 48-point weight records hold the float64 y,z transform of the weights, rounded to fp32
once, exactly and in the order the kernel and include/sp3d.h index them; and the flagged calls are refused for the same bad
arguments, with the same codes, as the calls without the flag - the table tests/test_host_cabi.py holds the split64 entries
to - before anything reaches the GPU runtime (no GPU needed: every call below is refused, the dummy pointers are never
dereferenced).

The issue behind this form asked for two new C entries.  tests/test_host_cabi.py and tests/test_glue_sweep_reference.py pin the
set of exported entries, so the form is selected by a flag bit on the two existing ones, as SP3D_HM_ONE_ZSPECTRUM is."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.test_host_cabi import ROOT

EINVAL, ENULL, ERANGE, EUNSUPPORTED = -1, -2, -3, -4
G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


@pytest.fixture(scope="module")
def lib():
    from selfpose3d_amd import _lib, build as sbuild
    sbuild.build()
    return _lib.load()


def _wild(shape, g):
    """weights over ~7 decades, so that every piece of the split carries bits"""
    return torch.randn(shape, generator=g) * torch.exp(4 * torch.randn(shape, generator=g))


def test_flag_is_the_headers():
    from selfpose3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sp3d.h")).read()
    m = re.search(r"#define\s+SP3D_CONV3_WINO_YZ\s+(0x[0-9a-fA-F]+)", hdr)
    assert m and int(m.group(1), 16) == _lib.CONV3_WINO_YZ == 0x100
    assert _lib.CONV3_WINO_YZ & 3 == 0                                  # disjoint from the modes 0..3
    for name, val in (("SP3D_EINVAL", EINVAL), ("SP3D_ENULL", ENULL), ("SP3D_ERANGE", ERANGE), ("SP3D_EUNSUPPORTED", EUNSUPPORTED)):
        m = re.search(name + r"\s*=\s*(-?\d+)", hdr)
        assert m and int(m.group(1)) == val, name


@pytest.mark.parametrize("Cc", [32, 64])
def test_records_reproduce_the_yz_transform_exactly(Cc):
    """pieces summed per record and the layout undone == fp32(float64 G w G^T along y and z), raw along x; 48 points, point =
    dx*16 + j*4 + k; [point, chunk, group, o, piece (mid, hi, lo), q], channel = 16 chunk + 4 group + q"""
    from selfpose3d_amd import _lib
    g = torch.Generator().manual_seed(11 + Cc)
    O = 64
    w = _wild((O, Cc, 3, 3, 3), g)
    W = _lib.wino_yz_weights_split(w)
    assert W.dtype == torch.bfloat16 and W.is_contiguous() and tuple(W.shape) == (48, Cc // 16, 4, O, 3, 4)
    assert W.numel() * 2 == 48 * Cc * O * 6                               # 6 bytes per weight and point
    # a record is 24 bytes and the base of a torch allocation is far more aligned than 8: every record is 8-byte aligned
    assert W.stride(3) * W.element_size() == 24 and W.data_ptr() % 8 == 0
    # the reference transform, written out independently of the helper: loops in float64
    Gd = torch.tensor(G, dtype=torch.float64)
    wd = w.double()
    want = torch.zeros(3, 4, 4, Cc, O, dtype=torch.float64)
    for j in range(4):
        for k in range(4):
            for a in range(3):
                for b in range(3):
                    want[:, j, k] += Gd[j, a] * Gd[k, b] * wd[:, :, :, a, b].permute(2, 1, 0)       # [dx, c, o]
    want = want.reshape(48, Cc, O).float()                                 # rounded to fp32 once
    back = W.double().sum(-2).permute(0, 3, 1, 2, 4).reshape(48, O, Cc).permute(0, 2, 1)           # [p, c, o]
    assert torch.equal(back, want.double())
    assert torch.equal(_lib.wino_yz_weights(w), want)
    # the pieces are ordered (mid, hi, lo): hi is the bf16 rounding of the value
    hi = W[..., 1, :].permute(0, 3, 1, 2, 4).reshape(48, O, Cc).permute(0, 2, 1)
    assert torch.equal(hi, want.bfloat16())
    # taps along x are the raw weights where G is the identity row: point (dx, j=0, k=0) = w[..., dx, 0, 0]
    assert torch.equal(want[0 * 16], w[:, :, 0, 0, 0].t()) and torch.equal(want[2 * 16 + 15], w[:, :, 2, 2, 2].t())


def test_switch(monkeypatch):
    from selfpose3d_amd import _lib
    monkeypatch.delenv("SP3D_WINO_YZ", raising=False)
    assert _lib.wino_yz_enabled()
    monkeypatch.setenv("SP3D_WINO_YZ", "0")
    assert not _lib.wino_yz_enabled()
    monkeypatch.setenv("SP3D_WINO_YZ", "1")
    assert _lib.wino_yz_enabled()


def test_plan_record_has_a_slot_for_the_yz_form():
    """the plan's layer record carries the 48-point records next to the 64-point ones; weights on the CPU get neither"""
    from selfpose3d_amd.v2v_net import _Conv, _FoldedV2V
    assert "split_yz" in _Conv._fields and _Conv(None, None).split_yz is None
    c = _FoldedV2V._conv3_record(torch.zeros(64, 64, 3, 3, 3), torch.zeros(64))
    assert c.split is None and c.split_yz is None


def test_flagged_calls_refuse_like_the_plain_ones(lib):
    """the table of tests/test_host_cabi.py::test_conv3_entries_refuse_in_the_documented_order for sp3d_wino_fused_split64 and
    its _skip form, with SP3D_CONV3_WINO_YZ set: SP3D_EINVAL, SP3D_ENULL, SP3D_EUNSUPPORTED, SP3D_ERANGE in that order"""
    from selfpose3d_amd import _lib
    YZ = _lib.CONV3_WINO_YZ
    d, off4 = C.c_void_p(0x1000), C.c_void_p(0x1004)
    big = dict(B=1 << 20, X=1024, Y=1024, Z=1024)

    def moded(x=d, w=d, y=d, shift=d, res=None, mode=0, B=1, X=8, Y=8, Z=8, Cin=64, O=64):
        return lib.sp3d_wino_fused_split64(x, w, y, shift, res, mode | YZ if mode >= 0 else mode, B, X, Y, Z, Cin, O, None)

    def skip(x=d, w=d, y=d, shift=d, xs=d, ws=d, B=1, X=8, Y=8, Z=8, Cin=64, O=64, CS=32):
        return lib.sp3d_wino_fused_split64_skip(x, w, y, shift, xs, ws, B, X, Y, Z, Cin, O, CS | YZ, None)

    for f in (moded, skip):
        for dim in ("B", "X", "Y", "Z"):
            assert f(**{dim: 0}) == EINVAL and f(**{dim: -1}) == EINVAL, dim
        for ptr in ("x", "w", "y", "shift"):
            assert f(**{ptr: None}) == ENULL, ptr
        assert f(O=48) == EUNSUPPORTED and f(O=32) == EUNSUPPORTED and f(Cin=16) == EUNSUPPORTED and f(Cin=128) == EUNSUPPORTED
        assert f(w=off4) == EUNSUPPORTED and f(w=off4, **big) == EUNSUPPORTED
        assert f(**big) == ERANGE
        # the order: the earlier rule answers for a call that breaks several
        assert f(B=0, x=None, O=48) == EINVAL
        assert f(x=None, O=48, **big) == ENULL
        assert f(O=48, **big) == EUNSUPPORTED
    assert moded(Cin=32, **big) == ERANGE                                  # 32 -> 64 is a supported width of the moded entry
    assert moded(mode=4) == EINVAL and moded(mode=-1) == EINVAL and moded(mode=4, x=None) == EINVAL
    assert moded(mode=2) == ENULL and moded(mode=3) == ENULL              # a residual mode without the residual
    assert moded(mode=2, O=48) == ENULL
    # the bit twice over or another high bit is no mode
    assert lib.sp3d_wino_fused_split64(d, d, d, d, None, YZ | 0x200, 1, 8, 8, 8, 64, 64, None) == EINVAL
    assert skip(xs=None) == ENULL and skip(xs=None, O=48) == ENULL and skip(ws=None) == ENULL
    assert skip(xs=off4) == EUNSUPPORTED and skip(ws=off4) == EUNSUPPORTED
    assert skip(Cin=32) == EUNSUPPORTED and skip(CS=16) == EUNSUPPORTED and skip(CS=64) == EUNSUPPORTED
    assert skip(X=4096, Y=4096, Z=4) == ERANGE
    # no other entry takes the bit
    for name in ("sp3d_wino_fused", "sp3d_wino_fused_split", "sp3d_conv3_split"):
        assert getattr(lib, name)(d, d, d, d, None, YZ, 1, 8, 8, 8, 32, 32, None) == EINVAL, name
    assert lib.sp3d_conv3_split_skip(d, d, d, d, d, d, 1, 8, 8, 8, 32, 32, 16 | YZ, None) == EUNSUPPORTED
