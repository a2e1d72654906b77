"""CPU-side tests of the quarter-resolution direct convolution behind sp3d_conv3_split with O = 128 (csrc/sp3d_conv3_quarter.hip): its refusals, all before
the first HIP call (the dummy pointers are never dereferenced), the rule that routes shapes to it, and the records it reads."""
import ctypes as C
import os
import re

import pytest
import torch

from selfpose3d_amd import _lib, build as sbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def test_entry_refuses_in_the_documented_order(lib):
    hdr = open(os.path.join(ROOT, "include", "sp3d.h")).read()
    EINVAL, ENULL, ERANGE, EUNSUPPORTED = (int(re.search(name + r"\s*=\s*(-?\d+)", hdr).group(1))
                                           for name in ("SP3D_EINVAL", "SP3D_ENULL", "SP3D_ERANGE", "SP3D_EUNSUPPORTED"))
    d, off4 = C.c_void_p(0x1000), C.c_void_p(0x1004)
    big = dict(B=1 << 20, X=1024, Y=1024, Z=1024)

    def f(x=d, w=d, y=d, shift=d, res=None, mode=0, B=1, X=5, Y=5, Z=5, Cin=128, O=128):
        return lib.sp3d_conv3_split(x, w, y, shift, res, mode, B, X, Y, Z, Cin, O, None)
    assert f(B=0) == EINVAL and f(Z=0) == EINVAL and f(mode=4) == EINVAL and f(mode=-1) == EINVAL
    for name in ("x", "w", "y", "shift"):
        assert f(**{name: None}) == ENULL, name
    assert f(mode=2) == ENULL and f(mode=3) == ENULL and f(mode=2, res=d) != ENULL
    # widths: (64 | 128) -> 128 only
    for cin, o in ((32, 128), (128, 64), (96, 128), (128, 32), (64, 32), (256, 128), (0, 128)):
        assert f(Cin=cin, O=o) == EUNSUPPORTED, (cin, o)
    for name in ("x", "w", "y", "shift"):
        assert f(**{name: off4}) == EUNSUPPORTED, name
    assert f(mode=2, res=off4) == EUNSUPPORTED
    # 2^31 elements in a sample, or more workgroups than a launch takes
    assert f(**big) == ERANGE and f(Cin=64, **big) == ERANGE
    assert f(X=2048, Y=2048, Z=4) == ERANGE and f(B=1 << 30, X=5, Y=5, Z=5) == ERANGE
    # the order: the earlier rule answers for a call that breaks several
    assert f(B=0, x=None, O=48) == EINVAL and f(x=None, O=48, **big) == ENULL and f(O=48, **big) == EUNSUPPORTED


def test_routing_rule_and_switch(monkeypatch):
    """conv3_route gives the direct kernel the two widths on grids of at most 64 whole 5x5x5 blocks; SP3D_QUARTER_DIRECT=0 none"""
    cov = _lib.quarter_direct_covers
    assert cov(4, 128, 128, 20, 20, 5) and cov(4, 64, 128, 20, 20, 5) and cov(1, 128, 128, 20, 20, 5) and cov(1, 64, 128, 10, 10, 5)
    assert not cov(2, 128, 128, 40, 40, 10) and not cov(5, 128, 128, 20, 20, 5)          # more than one workgroup per CU
    assert not cov(1, 128, 128, 12, 12, 3) and not cov(8, 128, 128, 16, 16, 16) and not cov(4, 128, 128, 20, 20, 6)
    assert not cov(4, 32, 128, 20, 20, 5) and not cov(4, 128, 64, 20, 20, 5)
    monkeypatch.delenv("SP3D_QUARTER_DIRECT", raising=False)
    assert _lib.quarter_direct_enabled()
    monkeypatch.setenv("SP3D_QUARTER_DIRECT", "0")
    assert not _lib.quarter_direct_enabled()
    monkeypatch.setenv("SP3D_QUARTER_DIRECT", "1")
    assert _lib.quarter_direct_enabled()


def test_records_the_kernel_reads():
    """conv_weights_split24 of a (128, C, 3, 3, 3) weight: per (tap, chunk, 32 outputs) 1536 bytes, [half][t] x {hi,lo} then
    [half][t] x {mid}; hi + mid + lo is the weight exactly, and the pieces are those of conv_weights_split"""
    g = torch.Generator().manual_seed(1)
    for Cin in (64, 128):
        w = torch.randn((128, Cin, 3, 3, 3), generator=g)
        r = _lib.conv_weights_split24(w)
        assert tuple(r.shape) == (27, Cin // 8, 4, 768) and r.dtype == torch.bfloat16 and r.is_contiguous()
        assert r.element_size() * 768 == 1536
        old = _lib.conv_weights_split(w)                                   # (27, C/8, 2, O, 6, 4): {hi,lo} {hi,hi} {mid,mid}
        for tap, chunk, half, o in ((9 * 2 + 3 * 1 + 0, Cin // 8 - 1, 1, 97), (0, 0, 0, 0), (13, 3, 0, 127)):   # kz = 2, ky = 1, kx = 0
            og, t = divmod(o, 32)
            blk = r[tap, chunk, og]
            hl, mid = blk[:512].reshape(2, 32, 2, 4)[half, t], blk[512:].reshape(2, 32, 4)[half, t]
            assert torch.equal(hl[0], old[tap, chunk, half, o, 0]) and torch.equal(hl[1], old[tap, chunk, half, o, 1])
            assert torch.equal(mid, old[tap, chunk, half, o, 4])
            kz, ky, kx = tap // 9, (tap // 3) % 3, tap % 3
            assert torch.equal((hl[0].float() + mid.float()) + hl[1].float(), w[o, 8 * chunk + 4 * half:8 * chunk + 4 * half + 4, kx, ky, kz])
    with pytest.raises(Exception):
        _lib.conv_weights_split24(torch.zeros(48, 64, 3, 3, 3))            # O % 32


def test_plan_builds_the_records_for_the_quarter_layers_only_on_the_gpu():
    """_conv3_record on CPU weights makes no GPU forms (the library runs such a net); the widths it would add records for"""
    from selfpose3d_amd.v2v_net import _FoldedV2V
    rec = _FoldedV2V._conv3_record(torch.zeros(128, 64, 3, 3, 3), torch.zeros(128))
    assert rec.u is None and rec.direct is None and rec.direct24 is None
    # the routes the record is built for: the probe reaches the direct kernel for the two widths it covers, and only those
    for (o, c), want in (((128, 64), True), ((128, 128), True), ((64, 64), False), ((32, 16), False)):
        routes = _FoldedV2V._conv3_routes(c, o)
        assert ("conv3_split128_" in routes) == want, (o, c, routes)
        assert ("conv3_split_" in routes) == ((o, c) == (32, 16)), (o, c, routes)
    assert "wino_conv3d_" in _FoldedV2V._conv3_routes(64, 128)          # the fallback form keeps its weights too
