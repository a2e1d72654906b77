"""Host side of the folded 1x1x1 skip projections (sp3d_conv3_split_skip, sp3d_wino_fused_split64_skip): the weight records
hold the projection exactly in the order the kernels and include/sp3d.h index them, and both entries refuse bad arguments
before anything reaches the GPU runtime (no GPU needed: every call below is refused, the dummy pointers are never
dereferenced)."""
import ctypes as C
import os

import pytest
import torch

from tests.test_host_cabi import ROOT

EINVAL, ENULL, ERANGE, EUNSUPPORTED = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from selfpose3d_amd import _lib, build as sbuild
    sbuild.build()
    return _lib.load()


def test_error_codes_are_the_headers():
    import re
    src = open(os.path.join(ROOT, "include", "sp3d.h")).read()
    for name, val in (("SP3D_EINVAL", EINVAL), ("SP3D_ENULL", ENULL), ("SP3D_ERANGE", ERANGE), ("SP3D_EUNSUPPORTED", EUNSUPPORTED)):
        m = re.search(name + r"\s*=\s*(-?\d+)", src)
        assert m and int(m.group(1)) == val, name


def _wild(shape, g):
    """weights over ~7 decades, so that every piece of the split carries bits"""
    return torch.randn(shape, generator=g) * torch.exp(4 * torch.randn(shape, generator=g))


def test_direct_skip_records_reproduce_the_weight_exactly():
    """(32,16,1,1,1) -> one tap of the 48-byte records of sp3d_conv3_split: [chunk, half, o, operand, q]; the 27-tap form is
    what it was"""
    from selfpose3d_amd import _lib
    g = torch.Generator().manual_seed(3)
    O, Cc = 32, 16
    w = _wild((O, Cc, 1, 1, 1), g)
    W = _lib.conv_weights_split(w)
    assert W.dtype == torch.bfloat16 and W.is_contiguous() and tuple(W.shape) == (1, Cc // 8, 2, O, 6, 4)
    assert W.numel() * 2 == Cc * O * 12                               # 12 bytes per weight: 6 144 B
    f = W.float()
    hi, lo, mid = f[..., 0, :], f[..., 1, :], f[..., 4, :]
    assert torch.equal(f[..., 2, :], hi) and torch.equal(f[..., 3, :], hi) and torch.equal(f[..., 5, :], mid)
    back = (hi.double() + mid.double() + lo.double())[0].permute(2, 0, 1, 3).reshape(O, Cc)      # [o, 8 chunk + 4 half + q]
    assert torch.equal(back, w.reshape(O, Cc).double())
    w27 = _wild((O, 2 * Cc, 3, 3, 3), g)
    W27 = _lib.conv_weights_split(w27)
    assert tuple(W27.shape) == (27, 2 * Cc // 8, 2, O, 6, 4)
    f = W27.float()
    back = (f[..., 0, :].double() + f[..., 1, :].double() + f[..., 4, :].double()).permute(3, 1, 2, 4, 0).reshape(O, 2 * Cc, 27)
    assert torch.equal(back, w27.permute(0, 1, 4, 3, 2).reshape(O, 2 * Cc, 27).double())          # tap = kz*9 + ky*3 + kx


def test_winograd_skip_records_reproduce_the_weight_exactly():
    """(64,32,1,1,1) as the plan hands it over -> one point of the 24-byte records of sp3d_wino_fused_split64:
    [chunk, group, o, piece (mid, hi, lo), q]"""
    from selfpose3d_amd import _lib
    g = torch.Generator().manual_seed(4)
    O, Cc = 64, 32
    w = _wild((O, Cc, 1, 1, 1), g)
    W = _lib.wino_weights_split(w.reshape(O, Cc).t().reshape(1, Cc, O).contiguous(), 16)
    assert W.dtype == torch.bfloat16 and W.is_contiguous() and tuple(W.shape) == (1, Cc // 16, 4, O, 3, 4)
    assert W.numel() * 2 == Cc * O * 6                                # 6 bytes per weight: 12 288 B
    f = W.double()
    back = f.sum(-2)[0].permute(2, 0, 1, 3).reshape(O, Cc)                                        # [o, 16 chunk + 4 group + q]
    assert torch.equal(back, w.reshape(O, Cc).double())


def test_skip_fold_switch(monkeypatch):
    from selfpose3d_amd import _lib
    monkeypatch.delenv("SP3D_FOLD_SKIP", raising=False)
    assert _lib.skip_fold_enabled()
    monkeypatch.setenv("SP3D_FOLD_SKIP", "0")
    assert not _lib.skip_fold_enabled()
    monkeypatch.setenv("SP3D_FOLD_SKIP", "1")
    assert _lib.skip_fold_enabled()


def test_refusals_before_any_launch(lib):
    """the refusals of sp3d_conv3_split / sp3d_wino_fused_split64, null and alignment checks on xs and the skip records,
    SP3D_EUNSUPPORTED for every other (C, O, CS)"""
    p, odd8, odd4 = C.c_void_p(0x10000), C.c_void_p(0x10008), C.c_void_p(0x10004)
    f = lib.sp3d_conv3_split_skip
    ok = dict(x=p, W3=p, y=p, shift=p, xs=p, WS=p, B=1, X=16, Y=8, Z=4, C=32, O=32, CS=16)

    def call(fn, base, **kw):
        a = dict(base, **kw)
        return fn(a["x"], a["W3"], a["y"], a["shift"], a["xs"], a["WS"], a["B"], a["X"], a["Y"], a["Z"], a["C"], a["O"], a["CS"], None)
    for dim in ("B", "X", "Y", "Z"):
        assert call(f, ok, **{dim: 0}) == EINVAL, dim
    for ptr in ("x", "W3", "y", "shift", "xs", "WS"):
        assert call(f, ok, **{ptr: None}) == ENULL, ptr
    for ptr in ("W3", "y", "xs", "WS"):
        assert call(f, ok, **{ptr: odd8}) == EUNSUPPORTED, ptr
    for widths in (dict(C=16), dict(O=64), dict(CS=32), dict(CS=8), dict(C=64, O=64, CS=32)):
        assert call(f, ok, **widths) == EUNSUPPORTED, widths
    assert call(f, ok, X=2048, Y=2048, Z=16) == ERANGE

    f = lib.sp3d_wino_fused_split64_skip
    ok = dict(ok, C=64, O=64, CS=32)
    for dim in ("B", "X", "Y", "Z"):
        assert call(f, ok, **{dim: -1}) == EINVAL, dim
    for ptr in ("x", "W3", "y", "shift", "xs", "WS"):
        assert call(f, ok, **{ptr: None}) == ENULL, ptr
    assert call(f, ok, W3=odd4) == EUNSUPPORTED and call(f, ok, WS=odd4) == EUNSUPPORTED and call(f, ok, xs=odd8) == EUNSUPPORTED
    for widths in (dict(C=32), dict(O=32), dict(CS=16), dict(CS=64), dict(C=32, O=32, CS=16)):
        assert call(f, ok, **widths) == EUNSUPPORTED, widths
    assert call(f, ok, X=4096, Y=4096, Z=4) == ERANGE
