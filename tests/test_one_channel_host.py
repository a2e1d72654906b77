"""One heat-map channel unprojected in place (SP3D_HM_ONE_CHANNEL), without a GPU: the flag's value in the header and the
binding, the refusals of the C ABI (before any launch) and the stride classifier of ProjectLayer on CPU tensors."""
import ctypes as C
import os
import re

import pytest
import torch

from selfpose3d_amd import _lib, build as sbuild
from selfpose3d_amd.project_layer import ProjectLayer, nhwc_heatmap_views, one_channel_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_matches_header_and_collides_with_no_other_flag():
    with open(os.path.join(ROOT, "include", "sp3d.h")) as fh:
        text = fh.read()
    enum = dict((k, int(v, 0)) for k, v in re.findall(r"\b(SP3D_(?:HM|OUT|LAYOUT)_[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", text))
    assert enum["SP3D_HM_ONE_CHANNEL"] == 0x800 == _lib.HM_ONE_CHANNEL
    assert enum["SP3D_HM_BF16"] == _lib.HM_BF16 and enum["SP3D_OUT_BF16"] == _lib.OUT_BF16
    assert enum["SP3D_OUT_CHANNELS_LAST"] == _lib.OUT_CHANNELS_LAST
    flags = [v for k, v in enum.items() if not k.startswith("SP3D_LAYOUT_")]
    assert len(flags) >= 4
    for i, a in enumerate(flags):
        assert a & 0xff == 0 and a & (a - 1) == 0, hex(a)          # one bit each, above the layout byte
        for b in flags[i + 1:]:
            assert a & b == 0, (hex(a), hex(b))
    assert all(v < 0x100 for k, v in enum.items() if k.startswith("SP3D_LAYOUT_"))


@pytest.fixture(scope="module")
def lib():
    sbuild.build()
    return _lib.load()


def test_cabi_one_channel_refusals_before_any_launch(lib):
    """every call below must come back as SP3D_EUNSUPPORTED (-4) with pointers that are never dereferenced.  A library
    without the flag masks the bit off and LAUNCHES on these dummy pointers, so this runs only where no GPU is visible
    (tests/test_gpu_one_channel.py repeats the refusals with real tensors)."""
    if torch.cuda.is_available():
        pytest.skip("dummy-pointer refusals are checked only where no GPU is visible")
    one = _lib.HM_ONE_CHANNEL
    gs = (C.c_float * 3)(8000, 8000, 2000)
    views = (C.c_void_p * 2)(0x1000, 0x1000)
    d = C.c_void_p(0x1000)
    f, fi, fs = lib.sp3d_unproject_fwd, lib.sp3d_unproject_fwd_indexed, lib.sp3d_unproject_fwd_strided
    st = (C.c_int64 * 4)(4 * 64, 64, 16, 4)
    for layout, jp in ((_lib.LAYOUT_PLANAR, 15), (_lib.LAYOUT_NHWC, 16), (_lib.LAYOUT_NHWC, 17)):
        for J in (2, 3, 5, 16):                                                        # J is 1 or 4
            assert f(views, layout | one, jp, d, d, d, d, None, 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4, (layout, J)
            assert fi(views, layout | one, jp, d, None, d, d, d, None, 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
        assert fs(views, layout | one, jp, d, None, d, d, d, st, 1, 2, 2, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
        # a channels-last result has 4 channels
        assert f(views, layout | one | _lib.OUT_CHANNELS_LAST, jp, d, d, d, d, None, 1, 2, 1, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
        # fp32 storage only
        for J in (1, 4):
            assert f(views, layout | one | _lib.OUT_BF16, jp, d, d, d, d, None, 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
            assert f(views, layout | one | _lib.HM_BF16, jp, d, d, d, d, None, 1, 2, J, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
            # heat-maps of at least 2x2 pixels (arguments: h, w)
            assert f(views, layout | one, jp, d, d, d, d, None, 1, 2, J, 8, 1, 4, 4, 4, gs, 96, 72, None) == -4
            assert f(views, layout | one, jp, d, d, d, d, None, 1, 2, J, 1, 8, 4, 4, 4, gs, 96, 72, None) == -4
            assert fs(views, layout | one, jp, d, None, d, d, d, st, 1, 2, J, 8, 1, 4, 4, 4, gs, 96, 72, None) == -4
    # ... of at most 2^24 pixels
    assert f(views, _lib.LAYOUT_PLANAR | one, 1, d, d, d, d, None, 1, 2, 1, 4097, 4096, 4, 4, 4, gs, 96, 72, None) == -4
    # no pass mask: the training forward refuses the flag
    t = lib.sp3d_unproject_fwd_train
    assert t(views, _lib.LAYOUT_NHWC | one, 16, d, None, d, d, d, None, d, 1, 2, 1, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4
    assert t(views, _lib.LAYOUT_NHWC | one, 4, d, None, d, d, d, None, d, 1, 2, 4, 8, 8, 4, 4, 4, gs, 96, 72, None) == -4


def test_unproject_fwd_keeps_its_positional_signature():
    import inspect
    names = list(inspect.signature(_lib.unproject_fwd).parameters)
    assert names[-1] == "one_channel" and names[-2] == "out"
    assert inspect.signature(_lib.unproject_fwd).parameters["one_channel"].default is False


# ---- the stride classifier (shapes, dtypes and strides only: CPU tensors) ------------------------------------------------
H, W = 6, 10


def _planar(B, Jt=15):
    return [torch.zeros(B, Jt, H, W) for _ in range(3)]


@pytest.mark.parametrize("B", [1, 2, 4])
def test_classifier_planar_slice(B):
    hms = [a[:, 2:3] for a in _planar(B)]
    assert not hms[0].is_contiguous() or B == 1
    assert one_channel_source(hms) == (_lib.LAYOUT_PLANAR, 15 if B > 1 else 1)
    last = [a[:, 14:15] for a in _planar(B)]
    assert one_channel_source(last) == (_lib.LAYOUT_PLANAR, 15 if B > 1 else 1)


@pytest.mark.parametrize("B", [1, 3])
def test_classifier_contiguous_single_channel(B):
    hms = [torch.zeros(B, 1, H, W) for _ in range(5)]
    assert one_channel_source(hms) == (_lib.LAYOUT_PLANAR, 1)
    # the unbound views of one (V,B,1,h,w) tensor, as the synthetic root branch renders them
    assert one_channel_source(list(torch.zeros(5, B, 1, H, W).unbind(0))) == (_lib.LAYOUT_PLANAR, 1)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("J,ps", [(15, 16), (17, 32)])
def test_classifier_channels_last_slice(B, J, ps):
    assert ProjectLayer.jp_for(J) == ps
    packed = torch.zeros(3, B, H, W, ps)
    views = nhwc_heatmap_views(packed, J)
    for ch in (0, 2, J - 1):
        hms = [v[:, ch:ch + 1] for v in views]
        assert one_channel_source(hms) == (_lib.LAYOUT_NHWC, ps)
        assert hms[0].data_ptr() == packed[0].data_ptr() + 4 * ch           # a view of the producer's buffer, no copy


def test_classifier_odd_pixel_stride():
    buf = torch.zeros(2, H, W, 7)
    hms = [buf.permute(0, 3, 1, 2)[:, 3:4] for _ in range(2)]
    assert one_channel_source(hms) == (_lib.LAYOUT_NHWC, 7)


def test_classifier_rejections():
    B = 2
    ok = [a[:, 2:3] for a in _planar(B)]
    assert one_channel_source(ok) is not None
    assert one_channel_source([]) is None
    assert one_channel_source([a[:, 2:4] for a in _planar(B)]) is None                      # J != 1
    assert one_channel_source(_planar(B)) is None
    assert one_channel_source([a.double() for a in ok]) is None                             # not fp32
    assert one_channel_source([a.bfloat16() for a in ok]) is None
    assert one_channel_source([torch.zeros(1, 1, H, W).expand(B, 1, H, W)] * 2) is None      # stride 0 (samples)
    assert one_channel_source([torch.zeros(B, 1, H, 1).expand(B, 1, H, W)] * 2) is None      # stride 0 (pixels)
    assert one_channel_source([torch.zeros(B, 1, 1, W).expand(B, 1, H, W)] * 2) is None      # stride 0 (rows)
    assert one_channel_source([torch.zeros(B, 1, H, 3 * W)[..., ::2][..., :W]] * 2) is None  # row stride != w x pixel stride
    assert one_channel_source([torch.zeros(B, 1, H, W + 3)[..., :W]] * 2) is None            # cropped rows
    assert one_channel_source([torch.zeros(B, 1, 2 * H, W)[:, :, ::2]] * 2) is None          # every other row
    assert one_channel_source([torch.zeros(B, 1, W, H).transpose(2, 3)] * 2) is None         # transposed image
    assert one_channel_source([torch.zeros(B, 1, H * W + 1)[..., :H * W].view(B, 1, H, W)] * 2) is None   # sample stride not k*h*w
    assert one_channel_source([torch.zeros(2 * B, H, W, 8).permute(0, 3, 1, 2)[::2, 1:2]] * 2) is None    # NHWC, every other sample
    assert one_channel_source([torch.zeros(B, 1, H, 1)] * 2) is None                         # under 2x2 pixels
    assert one_channel_source([torch.zeros(B, 1, 1, W)] * 2) is None
    assert one_channel_source([ok[0], torch.zeros(B, 1, H, W)]) is None                      # views of different form
    assert one_channel_source([ok[0], torch.zeros(B, 16, H, W)[:, 2:3]]) is None
    assert one_channel_source([ok[0], torch.zeros(B, H, W, 16).permute(0, 3, 1, 2)[:, 2:3]]) is None
    assert one_channel_source([ok[0], torch.zeros(B, 15, H, W + 1)[:, 2:3]]) is None         # different shape
    assert one_channel_source([ok[0][0]]) is None                                            # not 4-d


def test_classifier_ignores_the_sample_stride_at_batch_one():
    """a dimension of size 1 carries an arbitrary stride: torch reports a (1,1,h,w) slice of (1,15,h,w) as contiguous"""
    a = torch.zeros(1, 15, H, W)[:, 2:3]
    assert a.stride(0) == 15 * H * W
    assert one_channel_source([a, torch.zeros(1, 1, H, W)]) == (_lib.LAYOUT_PLANAR, 1)
    b = torch.as_strided(torch.zeros(4 * H * W * 16), (1, 1, H, W), (12345, 1, W * 16, 16))
    assert one_channel_source([b]) == (_lib.LAYOUT_NHWC, 16)


def test_switch_default_and_environment(monkeypatch):
    from selfpose3d_amd.config import load_config
    cfg = load_config(None)
    monkeypatch.delenv("SP3D_ONE_CHANNEL", raising=False)
    assert ProjectLayer(cfg).one_channel is False           # opt-in: no timing of the path is on record
    monkeypatch.setenv("SP3D_ONE_CHANNEL", "0")
    assert ProjectLayer(cfg).one_channel is False
    monkeypatch.setenv("SP3D_ONE_CHANNEL", "1")
    assert ProjectLayer(cfg).one_channel is True
