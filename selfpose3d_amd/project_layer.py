"""Drop-in replacement for the reference's ``models.project_layer.ProjectLayer``.

Same constructor and call signature as /root/reference/lib/models/project_layer.py:15-106

    ProjectLayer(cfg)
    forward(heatmaps, meta, grid_size, grid_center, cube_size, flip_xcoords=None) -> (cubes, grids)

but the batch x view Python loop of ~90 tiny kernels per (sample, view) is replaced by one
host-side camera-table pack (cached while ``meta`` is unchanged) and one or two launches of
the hand-written gfx950 kernels behind the C ABI in include/sp3d.h.  There is no CPU path:
tensors must live on the GPU and libsp3d.so must be built, otherwise this raises.
"""
from __future__ import annotations

import contextlib
import weakref
from typing import NamedTuple, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .camera_pack import meta_cache_key, pack_cameras


# Re-tiled heat-maps are shared by every projection of one forward pass (1 coarse + up to
# MAX_PEOPLE_NUM fine calls read the same maps).  An entry is valid only while the very same
# tensor OBJECTS are alive and unmodified (weak references + version counters): a freed tensor
# whose address the allocator hands to the next batch can therefore never produce a false hit.
_PACK_CACHE: "list[tuple]" = []


def packed_heatmaps(hms: Sequence[torch.Tensor], jp: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    if any(h.is_inference() for h in hms):      # inference tensors carry no version counter: nothing to key on
        return _lib.pack_heatmaps([x.detach() for x in hms], jp=jp, out_dtype=dtype)
    for refs, versions, cjp, packed in _PACK_CACHE:
        if cjp == (jp, dtype) and len(refs) == len(hms) and \
                all(r() is h and v == h._version for r, v, h in zip(refs, versions, hms)):
            return packed
    packed = _lib.pack_heatmaps([x.detach() for x in hms], jp=jp, out_dtype=dtype)
    _PACK_CACHE.append((tuple(weakref.ref(h) for h in hms), tuple(h._version for h in hms), (jp, dtype), packed))
    while len(_PACK_CACHE) > 2:
        _PACK_CACHE.pop(0)
    return packed


def clear_pack_cache():
    _PACK_CACHE.clear()


def nhwc_heatmap_views(packed: torch.Tensor, num_joints: int) -> "list[torch.Tensor]":
    """``packed`` (V,B,h,w,Jp), channels >= num_joints ZERO  ->  list[V] of (B,J,h,w) tensors that are strided views
    of it (no copy).  This is how a producer that already works channels-last (``PoseResNet.forward_views``: the
    1x1 head emits jp_for(J) channels - 16 or 32 - the filters beyond J being zero) hands its heat-maps over: every consumer sees the
    reference's ``list[V] of (B,J,h,w)`` and ``ProjectLayer`` recognises the views and skips its re-tiling pass -
    the kernel reads the producer's buffer directly (``SP3D_LAYOUT_NHWC`` takes per-view pointers)."""
    V, B, h, w, Jp = packed.shape
    if not packed.is_contiguous() or Jp != ProjectLayer.jp_for(num_joints):
        raise _lib.Sp3dError(f"nhwc_heatmap_views: need a contiguous (V,B,h,w,{ProjectLayer.jp_for(num_joints)}) buffer")
    views = []
    for c in range(V):
        t = packed[c].permute(0, 3, 1, 2)[:, :num_joints]
        t._sp3d_packed = (packed, c)
        views.append(t)
    return views


def _packed_source(hms: Sequence[torch.Tensor], jp: int, dtype: torch.dtype):
    """the (V,B,h,w,jp) buffer the heat-maps are views of (see nhwc_heatmap_views), or None"""
    tag = getattr(hms[0], "_sp3d_packed", None)
    if tag is None:
        return None
    base = tag[0]
    if base.dtype != dtype or base.shape[-1] != jp or base.shape[0] != len(hms):
        return None
    for c, h in enumerate(hms):
        t = getattr(h, "_sp3d_packed", None)
        if t is None or t[0] is not base or t[1] != c:
            return None
    return base


def one_channel_source(hms: Sequence[torch.Tensor], dtype: torch.dtype = torch.float32):
    """``list[V] of (B,1,h,w)`` tensors of ``dtype`` (fp32; bf16 for ``ProjectLayer.bf16_maps``, whose byte limits count 2-byte
    elements) that each are ONE channel of a wider tensor -> ``(layout, Jp)`` as the
    one-channel kernel addresses it (``SP3D_HM_ONE_CHANNEL``, include/sp3d.h), else ``None``.  Decided from shapes, dtypes
    and strides alone (no device access; CPU tensors classify the same way):

      * pixel stride 1, row stride w: a channel plane of a planar (B,Jp,h,w) tensor -> ``(LAYOUT_PLANAR, Jp)``, Jp = sample
        stride / (h*w) (a contiguous (B,1,h,w) tensor is the case Jp = 1);
      * pixel stride PS > 1, row stride w*PS, sample stride h*w*PS: a channel of a channels-last (B,h,w,PS) buffer (a slice
        of ``nhwc_heatmap_views``) -> ``(LAYOUT_NHWC, PS)``.

    A dimension of size 1 carries an arbitrary stride, so at B = 1 the sample stride is evidence of nothing and is not
    looked at (planar: Jp = 1, the kernel never leaves sample 0).  ``None`` for anything else: J != 1, another dtype,
    a stride of 0 (expanded tensors) or below 0, heat-maps under 2x2 or over 2^24 pixels, a row stride that is not
    w x pixel stride, a sample stride that fits neither form, views of different form."""
    if len(hms) == 0:
        return None
    first = None
    esize = 2 if dtype == torch.bfloat16 else 4
    for t in hms:
        if t.dim() != 4 or t.dtype != dtype or t.shape != hms[0].shape:
            return None
        B, J, h, w = t.shape
        if J != 1 or B < 1 or h < 2 or w < 2 or h * w > (1 << 24):
            return None
        sB, _, sH, sW = t.stride()
        if sW < 1 or sH != w * sW or (B > 1 and sB < 1):
            return None
        if sW == 1:
            if B == 1:
                form = (_lib.LAYOUT_PLANAR, 1)
            elif sB % (h * w) == 0:
                form = (_lib.LAYOUT_PLANAR, sB // (h * w))
            else:
                return None
        else:
            if B > 1 and sB != h * w * sW:
                return None
            # the limits resolve_one (csrc/sp3d_unproject.hip, the host plan) answers SP3D_EUNSUPPORTED for - 32-bit byte offsets, 24-bit
            # multiplies - so that such a buffer keeps the packed path instead of raising
            if h * w * sW * esize > 0x7fffffff or w * sW >= (1 << 24):
                return None
            form = (_lib.LAYOUT_NHWC, sW)
        if first is None:
            first = form
        elif form != first:
            return None
    return first


def unproject_path(J: int, grad_hm: bool, h: int, w: int, mode: str, wide_grad: bool) -> str:
    """Which kernels a ``get_voxel`` call takes: ``"nhwc"`` or ``"planar"``, or a raise for a ``mode="nhwc"`` request the
    NHWC path cannot differentiate.  Pure (no tensors): ``J`` joints, ``grad_hm`` = a heat-map gradient is wanted, an
    ``h`` x ``w`` map, the layer's ``mode`` and its ``wide_grad`` switch (already False for bf16 storage).
    17..32 joints (Jp = 32) run NHWC without a gradient; with one they keep the planar kernels - the pass mask of the
    packed backward holds 16 bits per voxel - unless ``wide_grad`` asks for the two-plane mask and the wide scatter."""
    wide = 16 < J <= 32
    wide_ok = wide and (not grad_hm or (wide_grad and w >= 2 and h >= 2))
    if mode == "auto":
        return "nhwc" if ((J <= 16 or wide_ok) and w >= 2 and h >= 2) else "planar"
    if mode == "nhwc" and J > 16 and grad_hm and not wide_ok:
        raise _lib.Sp3dError(f"ProjectLayer(mode='nhwc'): {J} joints with a heat-map gradient - the NHWC path "
                             "differentiates at most 16 joints (use mode='planar' or 'auto')")
    return mode


class Route(NamedTuple):
    """How one ``ProjectLayer`` call becomes a ``_lib`` call.  ``ProjectLayer.route`` fills it from the
    heat-maps' shapes, strides and dtypes, the gradient request, the layer's switches and the requested result; the
    launchers below read the record and nothing else."""
    read: str                       # "planar" | "packed": (V,B,h,w,jp), see _packed_maps | "one": one channel where it lies
    layout: int                     # the _lib.LAYOUT_* the kernel is told
    jp: int                         # packed: channel stride; one: the stride one_channel_source classified; planar: 0
    elem: torch.dtype               # element type the kernel reads
    write: str                      # "cubes" | "zdft" | "zspectrum" | "one_zspectrum"
    J: int                          # channels the kernel writes
    channels_last: bool = False
    out: bool = False               # the caller's ``out`` receives the cubes
    backward: str = "none"          # "none" | "planar" | "mask16" | "mask2x16" (17..32 joints) | "one"
    autograd: bool = False          # the call goes through _UnprojectFn
    widen: bool = False             # bf16 maps are widened first: ``bf16_maps`` on a request no bf16 kernel covers


def _fp32_maps(hms):
    return [x if (x.is_contiguous() and x.dtype == torch.float32) else x.contiguous().float() for x in hms]


def _packed_maps(layer, heatmaps, jp: int, dtype: torch.dtype, fp32_copies: bool = False) -> torch.Tensor:
    """the ``dtype`` (V,B,h,w,jp) buffer of these maps: the producer's own (no re-tiling pass), else the cached pack, else a
    fresh pack (which rounds fp32 maps for a bf16 buffer; ``fp32_copies``: from contiguous fp32 copies, as the autograd
    path always packed)"""
    source = _packed_source(heatmaps, jp, dtype)
    if source is not None:
        return source.detach()
    if layer.cache_packs:
        return packed_heatmaps(heatmaps, jp, dtype)
    hms = [x.detach() for x in heatmaps]
    return _lib.pack_heatmaps(_fp32_maps(hms) if fp32_copies else hms, jp=jp, out_dtype=dtype)


def _launch_cubes(layer, route, cam, centers, valid, grid_size, cube_size, want_grids, sample_of, out, heatmaps):
    """the forward launch of a cubes route -> (cubes, grids | None, pass mask | None, the maps a planar backward reads)"""
    _, _, h, w = heatmaps[0].shape
    P = int(centers.shape[0])                 # number of output cubes (== batch unless `sample_of` is given)
    X, Y, Z = cube_size
    hms = [x.detach() for x in heatmaps]
    # when a gradient will be asked for, the kernel also emits the clamp pass mask: the backward then scatters without
    # re-reading any heat-map (17..32 joints: one 16-bit plane per channel group)
    planes = {"mask16": (), "mask2x16": (2,), "one": ()}.get(route.backward)
    mask = None if planes is None else torch.empty(planes + (P, X * Y * Z), dtype=torch.int16, device=cam.device)
    geom = (cam, centers, valid, P, route.J, h, w, cube_size, grid_size, layer.img_size)
    saved = ()
    if route.read == "one" and mask is None:
        # one channel of a wider tensor, read where it lies: no slice copy, no re-tiling pass, no pack-cache entry
        cubes, grids = _lib.unproject_fwd(hms, route.layout, route.jp, *geom, want_grids, channels_last=route.channels_last,
                                          sample_of=sample_of, out=out, one_channel=True)
    elif route.read == "one":
        cubes, grids = _lib.unproject_one_fwd_train(hms, route.layout, route.jp, *geom, mask, want_grids,
                                                    channels_last=route.channels_last, sample_of=sample_of)
    elif route.read == "packed":
        fp32 = route.elem == torch.float32
        packed = _packed_maps(layer, heatmaps, route.jp, route.elem, fp32_copies=fp32 and route.autograd)
        # pad_channels (route.J == jp): the padded channels are zero in `packed`, the extra output channels exact zeros
        cubes, grids = _lib.unproject_fwd([packed[c] for c in range(len(hms))], _lib.LAYOUT_NHWC, route.jp, *geom, want_grids,
                                          channels_last=route.channels_last, sample_of=sample_of, out_dtype=layer.io_dtype,
                                          pass_mask=mask, out=out, wide_mask=route.backward == "mask2x16")
        if route.backward == "planar":
            saved = _fp32_maps(hms) if fp32 and _packed_source(heatmaps, route.jp, route.elem) is None else hms
    else:
        saved = hms = _fp32_maps(hms)
        cubes, grids = _lib.unproject_fwd(hms, _lib.LAYOUT_PLANAR, 0, *geom, want_grids, sample_of=sample_of)
    return cubes, grids, mask, saved


class _UnprojectFn(torch.autograd.Function):
    """autograd seam: gradient flows to the heat-maps only."""

    @staticmethod
    def forward(ctx, layer, route, cam, centers, valid, grid_size, cube_size, want_grids, sample_of, out, *heatmaps):
        cubes, grids, mask, saved = _launch_cubes(layer, route, cam, centers, valid, grid_size, cube_size, want_grids, sample_of,
                                                  out, heatmaps)
        # float64 callers (the mixed-precision pins of tests/test_gpu_reference_pins_r3.py: a float64 model around THIS fp32
        # path): the kernels compute and store fp32, the results travel on in the caller's type
        ctx.wide = heatmaps[0].dtype == torch.float64
        if ctx.wide:
            cubes = cubes.double()
            grids = grids.double() if grids is not None else None
        ctx.layer, ctx.route, ctx.mask, ctx.sample_of = layer, route, mask, sample_of
        ctx.dims = (int(heatmaps[0].shape[0]), len(heatmaps)) + tuple(int(v) for v in heatmaps[0].shape[1:])
        ctx.geom = (tuple(grid_size), tuple(cube_size))
        ctx.save_for_backward(cam, centers, valid, *saved)        # the masked backwards read no heat-map
        if grids is None:
            grids = torch.empty(0, device=cubes.device)
        ctx.mark_non_differentiable(grids)
        return cubes, grids

    @staticmethod
    def backward(ctx, grad_cubes, _grad_grids):
        cam, centers, valid, *hms = ctx.saved_tensors
        grid_size, cube_size = ctx.geom
        route, layer = ctx.route, ctx.layer
        batch, nv, J, h, w = ctx.dims
        if ctx.wide:
            grad_cubes = grad_cubes.float()
            wide = lambda gs: tuple(x.double() for x in gs)
        else:
            wide = tuple
        if route.backward == "one":
            one_args = (cam, centers, valid, grad_cubes, ctx.mask, batch, nv, h, w, cube_size, grid_size, layer.img_size)
            one_kw = dict(sample_of=ctx.sample_of, deterministic=layer.deterministic_backward)
            grads = _lib.unproject_one_bwd(*one_args, **one_kw) if route.elem == torch.float32 else \
                _lib.unproject_one_bwd_rounded(*one_args, **one_kw, out_dtype=route.elem)
        elif route.backward in ("mask16", "mask2x16"):
            grads = _lib.unproject_bwd_packed(cam, centers, valid, grad_cubes, ctx.mask, batch, nv, J, route.jp, h, w, cube_size,
                                              grid_size, layer.img_size, sample_of=ctx.sample_of,
                                              deterministic=layer.deterministic_backward, wide=route.backward == "mask2x16",
                                              out_dtype=route.elem)
        else:
            grads = _lib.unproject_bwd(hms, cam, centers, valid, grad_cubes, cube_size, grid_size, layer.img_size,
                                       sample_of=ctx.sample_of)
        return (None,) * 10 + wide(grads)


class ProjectLayer(nn.Module):
    """See module docstring.  ``mode``: "nhwc" (re-tile + fast kernel: J <= 16, and J <= 32 without a heat-map
    gradient - with one under ``wide_grad``), "planar" (direct kernel on the reference layout) or "auto" (nhwc wherever it
    applies)."""

    def __init__(self, cfg, mode: str = "auto", io_dtype: torch.dtype = torch.float32):
        super().__init__()
        # storage type of the re-tiled heat-maps and of the cubes: fp32 (reference) or bf16 ("mixed bf16",
        # BASELINE configs[4]); projection / interpolation / fusion arithmetic is fp32 either way
        self.io_dtype = io_dtype
        self.img_size = [int(v) for v in cfg.NETWORK.IMAGE_SIZE]        # project_layer.py:19
        self.heatmap_size = [int(v) for v in cfg.NETWORK.HEATMAP_SIZE]  # project_layer.py:20
        self.mode = mode
        self.cache_packs = True       # share the re-tiled heat-maps between the projections of one forward
        self._cam_key = None
        self._cam_dev = None
        self._static_cam = None       # see static_camera_table()
        self._cam_ring, self._cam_slot = [], 0     # pinned staging buffers of camera_table()
        # gradient scatter in 64-bit fixed point (bit-identical run to run) instead of fp32 atomics; SP3D_BWD_DETERMINISTIC=1
        self.deterministic_backward = _lib.env_switch("SP3D_BWD_DETERMINISTIC", False)
        # opt-in (SP3D_ONE_CHANNEL=1 / ``one_channel = True``): a (B,1,h,w) heat-map list that is one channel of a wider
        # tensor goes through the one-channel kernel, read in place (one_channel_source), instead of slice copy + re-tile +
        # packed kernel.  Same bits either way; off until tools/bench_roothm.py has recorded that it is faster
        self.one_channel = _lib.env_switch("SP3D_ONE_CHANNEL", False)
        # opt-in (SP3D_ONE_CHANNEL_GRAD=1 / ``one_channel_grad = True``), independent of ``one_channel``: the same kind of list
        # WITH a heat-map gradient trains through the one-channel pair (_lib.unproject_one_fwd_train / unproject_one_bwd)
        # instead of slice copy + re-tile + packed training forward + 4-channel scatter.  Same cubes, same deterministic
        # gradient bits; off until tools/bench_roothm_grad.py has recorded that it is faster
        self.one_channel_grad = _lib.env_switch("SP3D_ONE_CHANNEL_GRAD", False)
        # opt-in (SP3D_WIDE_GRAD=1 / ``wide_grad = True``): 17..32 joints (fp32 storage) WITH a heat-map gradient train through
        # the channels-last pair - training forward with a two-plane pass mask, wide packed scatter (fp32 or deterministic) -
        # instead of planar forward + planar backward.  Same cubes as the no-grad forward; off until tools/bench_wide_grad.py
        # has recorded that it is faster in every leg
        self.wide_grad = _lib.env_switch("SP3D_WIDE_GRAD", False)
        # opt-in (SP3D_WIDE_FRONT=1 / ``wide_zspectrum = True``, with ``V2VNet.wide_front``): ``get_voxel_zspectrum`` also takes
        # 17..32 joints - two launches, one per channel group of the 32-float pixel, into one z-spectrum - instead of raising.
        # Off until tools/bench_coco17.py has recorded that the root net is faster with it on both rigs
        self.wide_zspectrum = _lib.env_switch("SP3D_WIDE_FRONT", False)
        # opt-in (SP3D_ONE_FRONT=1 / ``one_zspectrum = True``, with ``V2VNet.one_front``): ``get_voxel_zspectrum`` also takes a
        # (B,1,h,w) list that is one channel of a wider tensor (one_channel_source) - read in place, one launch, the z-spectrum
        # of the one channel (SP3D_HM_ONE_ZSPECTRUM) - instead of raising.  Off until tools/bench_roothm_front.py has recorded
        # that the ROOTNET_ROOTHM root net is faster with it
        self.one_zspectrum = _lib.env_switch("SP3D_ONE_FRONT", False)
        # opt-in (SP3D_BF16_MAPS=1 / ``bf16_maps = True``; the model classes' ``use_bf16_heatmaps()``): the heat-maps are kept and
        # read as bf16, every result is fp32 ("mixed bf16", BASELINE configs[4], through the same fused fronts as fp32 maps:
        # SP3D_HM_BF16_IN).  bf16 producers are read in place, fp32 producers are rounded by the re-tiling pass.  Inference only:
        # a heat-map gradient ignores the switch, and a request no bf16 kernel covers widens the maps and takes the fp32 path.
        # Not to be combined with ``io_dtype`` (bf16 cubes), which keeps its meaning and its refusals.
        self.bf16_maps = _lib.env_switch("SP3D_BF16_MAPS", False)
        # opt-in (SP3D_BF16_TRAIN=1 / ``bf16_train = True``; the model classes' ``use_bf16_training()``): bf16 heat-maps WITH a
        # heat-map gradient are read as bf16 by the masked training forwards (SP3D_HM_BF16_TRAIN: fp32 cubes, the same pass
        # mask) and the gradient leaves as bf16, rounded once - instead of widening every view, packing fp32 pixels and having
        # autograd cast each fp32 gradient view back.  Acts only when every map is bf16, ``io_dtype`` is fp32 and the path is
        # NHWC, for 13..16 joints, 17..32 with ``wide_grad`` and one channel with ``one_channel_grad``; anything else takes
        # the route it took.  Same cubes and same deterministic gradient bits; off until tools/bench_bf16_train.py has
        # recorded that it is faster in every leg
        self.bf16_train = _lib.env_switch("SP3D_BF16_TRAIN", False)

    # -- the route: one pure decision (no device access; CPU tensors classify the same way) --------------
    def route(self, heatmaps, SZ=None, want_grids=True, pad_channels=False, channels_last=False, out=False) -> Route:
        """The ``Route`` of ``get_voxel(heatmaps, ..., want_grids, pad_channels, channels_last, out=<given>)`` or, with ``SZ``,
        of ``get_voxel_zspectrum(heatmaps, ..., SZ)`` (which has refused a heat-map gradient before it asks), or the
        ``Sp3dError`` that call raises.  ``sample_of`` changes no route.  DESIGN.md §4.0a is this function as a table."""
        fp32 = self.io_dtype == torch.float32
        if SZ is not None:
            if self.bf16_maps and not fp32:
                raise _lib.Sp3dError("ProjectLayer: bf16_maps (bf16 maps, fp32 results) and io_dtype (bf16 maps and cubes) exclude each other")
            route = self.spectrum_route(heatmaps)
            if route is None:
                raise _lib.Sp3dError("get_voxel_zspectrum: fp32 NHWC path with 13..16 joints only")
            return route
        _, J, h, w = heatmaps[0].shape
        grad_hm = torch.is_grad_enabled() and any(x.requires_grad for x in heatmaps)
        path = unproject_path(J, grad_hm, h, w, self.mode, self.wide_grad and fp32)
        jp = self.jp_for(J)
        bricks = jp in (16, 32) and J <= 32           # 13..32 joints: what the kernels that read bf16 pixels cover
        if not fp32 and (path != "nhwc" or not bricks):
            raise _lib.Sp3dError("bf16 storage needs the NHWC path with 13..32 joints")
        if path != "nhwc" or J > 16:
            pad_channels = channels_last = False
        if channels_last and not pad_channels and (J & 3):
            channels_last = False
        # the pass mask of a wanted gradient: the masked training forwards write fresh cubes only
        masked = path == "nhwc" and fp32 and grad_hm and w >= 2 and h >= 2 and (jp <= 16 or (jp == 32 and self.wide_grad))
        one_grad = path == "nhwc" and fp32 and grad_hm and J == 1 and self.one_channel_grad and one_channel_source(heatmaps)
        if out and (path != "nhwc" or want_grids or pad_channels or channels_last or masked or one_grad):
            raise _lib.Sp3dError("get_voxel(out=...): planar NHWC-path result without grids only")
        if self.bf16_maps and not fp32:
            raise _lib.Sp3dError("ProjectLayer: bf16_maps (bf16 maps, fp32 results) and io_dtype (bf16 maps and cubes) exclude each other")
        if path == "planar":
            return Route("planar", _lib.LAYOUT_PLANAR, 0, torch.float32, "cubes", J, backward="planar" if grad_hm else "none",
                         autograd=True, widen=self.bf16_maps and not grad_hm and heatmaps[0].dtype == torch.bfloat16)
        J_one = 4 if pad_channels else 1              # the one-channel kernels: the value + three zero channels
        widen, probe = False, heatmaps
        if self.bf16_maps and not grad_hm:            # bf16 pixels in, fp32 cubes out, no autograd
            one = one_channel_source(heatmaps, torch.bfloat16) if (J == 1 and self.one_channel) else None
            if one:
                return Route("one", one[0], one[1], torch.bfloat16, "cubes", J_one, channels_last, out)
            if J != 1 and bricks:
                return Route("packed", _lib.LAYOUT_NHWC, jp, torch.bfloat16, "cubes", jp if pad_channels else J, channels_last, out)
            # no bf16 kernel covers the request (fewer than 13 joints on the packed path): the fp32 routes below on the widened
            # maps - whose strides are what widening will give them, asked of meta tensors
            widen = heatmaps[0].dtype == torch.bfloat16
            if widen and J == 1 and self.one_channel:
                probe = [torch.empty_strided(tuple(x.shape), x.stride(), dtype=x.dtype, device="meta").float() for x in heatmaps]
        if self.bf16_train and fp32 and grad_hm and all(x.dtype == torch.bfloat16 for x in heatmaps):
            # bf16 pixels into the masked training forwards, the gradient out as bf16: no widened copy, no fp32 pack
            one = one_channel_source(heatmaps, torch.bfloat16) if (J == 1 and self.one_channel_grad) else None
            if one:
                return Route("one", one[0], one[1], torch.bfloat16, "cubes", J_one, channels_last, backward="one", autograd=True)
            if masked and jp in (16, 32):
                return Route("packed", _lib.LAYOUT_NHWC, jp, torch.bfloat16, "cubes", jp if pad_channels else J, channels_last,
                             backward="mask2x16" if jp == 32 else "mask16", autograd=True)
        if one_grad:
            return Route("one", one_grad[0], one_grad[1], torch.float32, "cubes", J_one, channels_last, backward="one", autograd=True)
        one = one_channel_source(probe) if (fp32 and J == 1 and self.one_channel and not grad_hm) else None
        if one:
            return Route("one", one[0], one[1], torch.float32, "cubes", J_one, channels_last, out, autograd=True, widen=widen)
        backward = ("mask2x16" if jp == 32 else "mask16") if masked else ("planar" if grad_hm else "none")
        return Route("packed", _lib.LAYOUT_NHWC, jp, self.io_dtype, "cubes", jp if pad_channels else J, channels_last, out, backward,
                     autograd=True, widen=widen)

    def spectrum_route(self, heatmaps):
        """the ``Route`` of ``get_voxel_zspectrum`` for these maps (inference: no gradient is looked at), or None where it
        refuses: 13..16 joints, 17..32 with ``wide_zspectrum``, one channel in place with ``one_zspectrum``; fp32 storage"""
        _, J, h, w = heatmaps[0].shape
        if self.io_dtype != torch.float32 or self.mode not in ("auto", "nhwc") or w < 2 or h < 2:
            return None
        if J == 1 and self.one_zspectrum:     # strides are looked at only here, behind every refusal that shapes alone decide
            dtype = torch.bfloat16 if (self.bf16_maps and heatmaps[0].dtype == torch.bfloat16) else torch.float32
            one = one_channel_source(heatmaps, dtype)
            if one:
                return Route("one", one[0], one[1], dtype, "one_zspectrum", 1)
        jp = self.jp_for(J)
        if jp == 16 or (jp == 32 and J <= 32 and self.wide_zspectrum):
            # bf16 pixels and 17..32 joints: the brick kernels with the z-spectrum result, one launch per channel group
            if self.bf16_maps:
                return Route("packed", _lib.LAYOUT_NHWC, jp, torch.bfloat16, "zspectrum", J)
            return Route("packed", _lib.LAYOUT_NHWC, jp, torch.float32, "zspectrum" if jp == 32 else "zdft", J)
        return None

    def takes_out(self, heatmaps) -> bool:
        """``get_voxel(heatmaps, ..., want_grids=False, out=...)`` writes into an ``out`` buffer: whoever owns one asks here"""
        try:
            return self.route(heatmaps, want_grids=False, out=True).out
        except _lib.Sp3dError:
            return False

    def _require_maps(self, heatmaps):
        if not heatmaps[0].is_cuda:
            raise _lib.Sp3dError("ProjectLayer: heat-maps must be on the GPU (no CPU fallback)")
        _, _, h, w = heatmaps[0].shape
        if [w, h] != self.heatmap_size:
            # the reference samples with cfg HEATMAP_SIZE (project_layer.py:50) whatever the tensor says
            raise _lib.Sp3dError(f"heat-map tensor is {w}x{h} but cfg.NETWORK.HEATMAP_SIZE is {self.heatmap_size}")

    @contextlib.contextmanager
    def static_camera_table(self, table: torch.Tensor):
        """Inside the context every call uses ``table`` (a device tensor the caller refreshes itself) and re-tiles
        the heat-maps on every call: what HIP-graph capture of a forward needs (graphs.py).  Everything is restored
        on exit, so eager calls after a capture behave as before."""
        _lib._require_cam(table, "static camera table")
        prev = (self._static_cam, self.cache_packs)
        self._static_cam, self.cache_packs = table, False
        try:
            yield self
        finally:
            self._static_cam, self.cache_packs = prev

    @staticmethod
    def jp_for(J: int) -> int:
        """channel stride of the packed heat-maps: ceil4(J) up to 16, then one 32-float (128-byte) pixel for 17..32"""
        return 4 if J <= 4 else (8 if J <= 8 else (12 if J <= 12 else (16 if J <= 16 else 32)))

    # -- host side -----------------------------------------------------------------------
    def camera_table(self, meta: Sequence[dict], batch: int, flip_xcoords, device) -> torch.Tensor:
        """(B,V,64) fp32 table on `device`; rebuilt only when `meta` / flip change.  The upload is one
        asynchronous copy from a small ring of pinned staging buffers (no host<->GPU synchronisation,
        unlike the ~6 blocking transfers per (sample, view) of the reference, transforms.py:67-72)."""
        if self._static_cam is not None:
            return self._static_cam
        key = (meta_cache_key(meta, flip_xcoords, self.img_size), batch, str(device))
        if key != self._cam_key:
            tab = torch.from_numpy(pack_cameras(meta, batch, self.img_size, flip_xcoords))
            if device.type == "cuda":
                ring, slot = self._cam_ring, self._cam_slot
                if len(ring) < 4 or ring[slot][0].shape != tab.shape:
                    entry = [torch.empty_like(tab).pin_memory(), torch.cuda.Event()]
                    if len(ring) < 4:
                        ring.append(entry)
                        slot = len(ring) - 1
                    else:
                        ring[slot] = entry
                else:
                    ring[slot][1].synchronize()          # the copy that last used this staging buffer is long done
                pinned, ev = ring[slot]
                pinned.copy_(tab)
                dev_tab = torch.empty(tab.shape, dtype=torch.float32, device=device)
                dev_tab.copy_(pinned, non_blocking=True)
                ev.record(torch.cuda.current_stream(device))
                self._cam_slot = (slot + 1) % 4
                self._cam_dev = dev_tab
            else:
                self._cam_dev = tab.to(device)
            self._cam_key = key
        return self._cam_dev

    _CONST_CENTERS: "dict[tuple, tuple]" = {}

    @staticmethod
    def centers_valid(grid_center, batch: int, device):
        """(centers (B,3) fp32, valid (B) uint8) following project_layer.py:54,58-61.  A host-side list
        centre (the shared coarse-grid centre from the config) is uploaded once and reused - no per-call
        host->device copy, which also keeps the call HIP-graph capturable."""
        if isinstance(grid_center, torch.Tensor):
            gc = grid_center.to(device=device, dtype=torch.float32)
            if gc.dim() == 1:
                gc = gc[None]
        else:
            arr = np.asarray(grid_center, dtype=np.float32)
            key = (arr.tobytes(), arr.shape, int(batch), str(device))
            hit = ProjectLayer._CONST_CENTERS.get(key)
            if hit is not None:
                return hit
            gc = torch.as_tensor(arr, device=device)
        rows, cols = gc.shape
        if cols == 3:                       # `len(grid_center[0]) == 3`: always valid
            valid = torch.ones(batch, dtype=torch.uint8, device=device)
        else:
            flag = gc[:, 3] >= 0
            valid = (flag if rows == batch else flag[:1].expand(batch)).to(torch.uint8)
        centers = gc[:, :3]
        if rows == 1 and batch > 1:         # `len(grid_center) == 1`: shared centre
            centers = centers.expand(batch, 3)
        out = (centers.contiguous(), valid.contiguous())
        if not isinstance(grid_center, torch.Tensor):
            if len(ProjectLayer._CONST_CENTERS) > 64:
                ProjectLayer._CONST_CENTERS.clear()
            ProjectLayer._CONST_CENTERS[key] = out
        return out

    # -- reference API -------------------------------------------------------------------
    def get_voxel(self, heatmaps, meta, grid_size, grid_center, cube_size, flip_xcoords=None, want_grids=True,
                  pad_channels=False, channels_last=False, sample_of=None, out=None):
        """Reference semantics (project_layer.py:42-102).  Extras for in-repo callers only:
        ``want_grids=False`` skips the (B,N,3) grid output, ``pad_channels`` returns
        ceil4(J) channels (zeros beyond J) and ``channels_last`` returns torch.channels_last_3d
        strides - both let MIOpen's 3D convolutions run their fast paths without a copy;
        ``sample_of`` (int (P,)) with ``grid_center`` (P,5|3): P cubes, cube p read from sample
        sample_of[p] (all person proposals of a batch in one launch); ``out``: a (P,J,X,Y,Z) view of a larger buffer
        (z contiguous) that receives the planar result directly - no grids, inference only."""
        self._require_maps(heatmaps)
        route = self.route(heatmaps, None, bool(want_grids), bool(pad_channels), bool(channels_last), out is not None)
        device, B = heatmaps[0].device, heatmaps[0].shape[0]
        cam = self.camera_table(meta, B, flip_xcoords, device)
        if sample_of is not None:
            sample_of = sample_of.to(device=device, dtype=torch.int32).contiguous()
            centers, valid = self.centers_valid(grid_center, int(sample_of.shape[0]), device)
        else:
            centers, valid = self.centers_valid(grid_center, B, device)
        if isinstance(cube_size, int):
            cube_size = [cube_size] * 3
        if isinstance(grid_size, (int, float)):
            grid_size = [grid_size] * 3
        if route.widen:      # the right answer from the fp32 path on the widened maps
            heatmaps = [x.float() if x.dtype == torch.bfloat16 else x for x in heatmaps]
        args = (self, route, cam, centers, valid, [float(v) for v in grid_size], [int(v) for v in cube_size], bool(want_grids),
                sample_of, out)
        if route.autograd:
            cubes, grids = _UnprojectFn.apply(*args, *heatmaps)
        else:
            cubes, grids, _, _ = _launch_cubes(*args, heatmaps)
        return cubes, (grids if want_grids else None)

    def get_voxel_zspectrum(self, heatmaps, meta, grid_size, grid_center, cube_size, SZ: int, flip_xcoords=None):
        """Inference only, root grid only (round 6): ``get_voxel`` FUSED with the z pass of the V2V net's frequency-domain
        opening conv - the cubes are never written.  Returns the (B, J, SZ//2+1, X/4, Y/4, 16) complex64 z-spectrum of the
        cubes ``get_voxel`` would return (bit-identical to ``_lib.zdft_fwd_cl`` of its channels-last result), in the
        4 x 4-tiled layout ``_lib.cfft2d_88_tiled`` reads.  Same reference semantics (project_layer.py:42-102).
        13..16 joints; 17..32 with ``wide_zspectrum``; with ``one_zspectrum`` a ``list[V] of (B,1,h,w)`` that
        ``one_channel_source`` classifies (a slice of a planar tensor, a slice of the (V,B,h,w,16|32) buffer of
        ``PoseResNet.forward_views``, a contiguous (B,1,h,w)), read in place.  With ``bf16_maps`` the same three routes read
        bf16 maps (SP3D_HM_BF16_IN: a bf16 producer's buffer or tensors in place, fp32 producers rounded by the re-tiling
        pass); the spectrum is fp32 and bit-identical to the fp32 route's on the widened maps."""
        if torch.is_grad_enabled() and any(h.requires_grad for h in heatmaps):
            raise _lib.Sp3dError("get_voxel_zspectrum is an inference path (no autograd); use get_voxel")
        self._require_maps(heatmaps)
        route = self.route(heatmaps, SZ)
        device = heatmaps[0].device
        B, J, h, w = heatmaps[0].shape
        cam = self.camera_table(meta, B, flip_xcoords, device)
        centers, valid = self.centers_valid(grid_center, B, device)
        geom = (cam, centers, valid, B)
        tail = (h, w, [int(v) for v in cube_size], [float(v) for v in grid_size], self.img_size, int(SZ))
        if route.read == "one":     # read where it lies: no slice copy, no re-tiling pass, no pack-cache entry
            return _lib.unproject_one_fwd_zspectrum([x.detach() for x in heatmaps], route.layout, route.jp, *geom, *tail)
        packed = _packed_maps(self, heatmaps, route.jp, route.elem)
        launch = _lib.unproject_fwd_zdft if route.write == "zdft" else _lib.unproject_fwd_zspectrum
        return launch([packed[c] for c in range(len(heatmaps))], route.jp, *geom, J, *tail)

    def forward(self, heatmaps, meta, grid_size, grid_center, cube_size, flip_xcoords=None):
        return self.get_voxel(heatmaps, meta, grid_size, grid_center, cube_size, flip_xcoords=flip_xcoords)
