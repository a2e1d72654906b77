"""_lib.upconv_weights_split (host side of sp3d_upconv2x_fused): the records hold the GEMM-form weight exactly, in the order
the kernel and include/sp3d.h index them."""
import torch


def test_upconv_weight_records_reproduce_the_weight_exactly():
    from selfpose3d_amd import _lib
    g = torch.Generator().manual_seed(2)
    for Cin, O in ((64, 32), (128, 64)):
        wg = torch.randn(Cin, 8 * O, generator=g) * torch.exp(4 * torch.randn(Cin, 8 * O, generator=g))
        W3 = _lib.upconv_weights_split(wg)
        assert W3.dtype == torch.bfloat16 and W3.is_contiguous() and tuple(W3.shape) == (8, O // 32, Cin // 8, 2, 32, 6, 4)
        assert W3.numel() * 2 == Cin * 8 * O * 12                      # 12 bytes per weight: 196 608 B and 786 432 B
        f = W3.float()
        hi, lo, mid = f[..., 0, :], f[..., 1, :], f[..., 4, :]
        assert torch.equal(f[..., 2, :], hi) and torch.equal(f[..., 3, :], hi) and torch.equal(f[..., 5, :], mid)
        # [tap, ob, chunk, half, o, q] -> wg[8 chunk + 4 half + q, tap*O + 32 ob + o]
        back = (hi.double() + mid.double() + lo.double()).permute(2, 3, 5, 0, 1, 4).reshape(Cin, 8 * O)
        assert torch.equal(back, wg.double())


def test_upconv_fused_switch(monkeypatch):
    from selfpose3d_amd import _lib
    monkeypatch.delenv("SP3D_FUSE_UPCONV", raising=False)
    assert _lib.upconv_fused_covers(64, 32, True) and _lib.upconv_fused_covers(128, 64, False)
    assert not _lib.upconv_fused_covers(64, 32, False) and not _lib.upconv_fused_covers(128, 64, True)
    assert not _lib.upconv_fused_covers(48, 32, True)
    monkeypatch.setenv("SP3D_FUSE_UPCONV", "0")
    assert not _lib.upconv_fused_covers(64, 32, True) and not _lib.upconv_fused_covers(128, 64, False)
