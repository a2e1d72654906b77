"""ctypes binding of libsp3d.so (C ABI: include/sp3d.h).

There is NO CPU fallback behind this module: if the library is missing or a call fails,
an exception is raised.  torch is used only to obtain device pointers and the current HIP
stream (``torch.cuda.current_stream().cuda_stream``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB_PATH = os.path.join(_HERE, "libsp3d.so")
NOPK_LIB_PATH = os.path.join(_HERE, "libsp3d_nopk.so")       # the flavour without packed-fp32 instructions (shared GPUs)
# SP3D_LIB_PATH: a measurement / sanitizer build of the SAME sources instead of the shipped library (tools/sanitize_host.py)
LIB_PATH = os.environ.get("SP3D_LIB_PATH") or _DEFAULT_LIB_PATH

LAYOUT_PLANAR = 0
LAYOUT_NHWC = 1
OUT_CHANNELS_LAST = 0x100
HM_BF16 = 0x200
OUT_BF16 = 0x400
HM_ONE_CHANNEL = 0x800      # one channel of a wider tensor, read in place (include/sp3d.h)
HM_WIDE_MASK = 0x1000       # sp3d_unproject_fwd_train at Jp = 32: a (2, P, N) pass mask, one plane per channel group
OUT_ZSPECTRUM = 0x2000      # sp3d_unproject_fwd[_indexed]: the root grid's cubes leave as their z-spectrum (Jp = 16 or 32)
HM_ONE_ZSPECTRUM = 0x4000   # sp3d_unproject_fwd[_indexed]: one channel read in place, its cubes leave as their z-spectrum (J = 1)
HM_BF16_IN = 0x8000         # next to OUT_ZSPECTRUM, HM_ONE_CHANNEL or HM_ONE_ZSPECTRUM: the heat-maps are bf16, every result fp32
HM_BF16_TRAIN = 0x10000     # sp3d_unproject_fwd_train / sp3d_unproject_one_fwd_train: the heat-maps are bf16; fp32 results, the same pass mask
SCATTER_AUTO, SCATTER_PER_TAP, SCATTER_MERGE = 0, 2, 3     # include/sp3d.h: per-call scatter choice of unproject_bwd_packed
SCATTER_WIDE = 0x100        # OR-ed into that choice: 17..32 joints, 32-element pixels, the two-plane mask
CONV3_WINO_YZ = 0x100       # OR-ed into the mode of sp3d_wino_fused_split64 / the CS of its _skip form: Winograd in y,z, direct in x
CONV3_POOL2X = 0x200        # OR-ed into the CS of sp3d_conv3_split_skip / sp3d_wino_fused_split64_skip: the 2x max-pooled result behind y
MAX_VIEWS = 16
MAX_TOPK = 32
ABI_VERSION = 3

# The C ABI, one line per entry point: "<return>: <arguments>", one letter per type (blanks only group runs for the eye).
#   p  pointer - any parameter declared with * or [] (device pointers, host arrays, the stream): c_void_p
#   i  int / int32_t      l  int64_t      f  float      d  double      s  const char * (return only)
# tests/test_host_cabi.py parses the prototypes of the header and holds every line against it, both ways.
_CTYPES = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64, "f": C.c_float, "d": C.c_double, "s": C.c_char_p}

SIGNATURES = {                                  # include/sp3d.h, in the header's order
    "sp3d_abi_version": "i:",
    "sp3d_camera_finish": "i: p i",
    "sp3d_error_string": "s: i",
    "sp3d_pack_heatmaps": "i: pp iiiiii p",
    "sp3d_pack_heatmaps_ex": "i: pp iiiiiiii p",
    "sp3d_unproject_fwd": "i: p ii ppppp iiiiiiii p ii p",
    "sp3d_unproject_fwd_indexed": "i: p ii pppppp iiiiiiii p ii p",
    "sp3d_unproject_fwd_strided": "i: p ii pppppp iiiiiiii p ii p",
    "sp3d_unproject_bwd": "i: pppppp iiiiiiii p ii p",
    "sp3d_unproject_bwd_indexed": "i: ppppppp iiiiiiii p ii p",
    "sp3d_unproject_fwd_train": "i: p ii ppppppp iiiiiiii p ii p",
    "sp3d_unproject_bwd_packed": "i: ppppppp iiiiiiiiii p iii p",
    "sp3d_unproject_bwd_packed_det": "i: pppppppp iiiiiiiiii p iii p",
    "sp3d_fixed_to_float": "i: ppp l p",
    "sp3d_unproject_one_fwd_train": "i: p ii ppppppp iiiiiiii p ii p",
    "sp3d_unproject_one_bwd": "i: ppppp l pp iiiiiiii p ii p",
    "sp3d_unproject_one_bwd_det": "i: ppppp l ppp iiiiiiii p ii p",
    "sp3d_nms_topk_workspace_bytes": "l: iiiii",
    "sp3d_nms_topk": "i: p iiiii ppppppp",
    "sp3d_nms_proposals": "i: p iiiii pp f pppppp",
    "sp3d_soft_argmax": "i: ppp ii l f p",
    "sp3d_soft_argmax_grid": "i: ppp iii p ii f p",
    "sp3d_soft_argmax_grid_train": "i: ppp iii pp ii f p",
    "sp3d_soft_argmax_grid_bwd": "i: ppp iii pppp ii f p",
    "sp3d_channel_shift_act": "i: ppp i l i l i p",
    "sp3d_fetch_ring": "i: ppp ii p",
    "sp3d_maxpool2x_cl": "i: pp iiiii p",
    "sp3d_crop_shift_act_cl": "i: ppp iiiiiiiii p",
    "sp3d_rfft3d": "i: pp iiii p",
    "sp3d_irfft3d": "i: pp iiii p",
    "sp3d_cfft2d": "i: p iiii p",
    "sp3d_cfft2d_ex": "i: p iiiiii p",
    "sp3d_zdft_fwd_cl": "i: pp iiiiiiiii p",
    "sp3d_zdft_inv_cl": "i: ppp iiiiiiiii p",
    "sp3d_unproject_fwd_zdft": "i: p i pppp iiiiiiii p iii p",
    "sp3d_cfft2d_88_tiled": "i: pp iii p",
    "sp3d_freq_contract_ty": "i: pppp iiiii p",
    "sp3d_gaussian_target_3d": "i: p ii ppp iii f pp",
    "sp3d_render_root_heatmaps": "i: p ii p iii f pp",
    "sp3d_render_joints_fwd": "i: pp iiiii f pp",
    "sp3d_render_joints_bwd": "i: ppp iiiii f pp",
    "sp3d_freq_contract": "i: ppp iii l p",
    "sp3d_freq_contract_ex": "i: ppp iii lllll ii p",
    "sp3d_wino_input": "i: pp iiiii p",
    "sp3d_wino_output": "i: pppp iiiiii p",
    "sp3d_wino_fused": "i: ppppp iiiiiii p",
    "sp3d_wino_fused_split": "i: ppppp iiiiiii p",
    "sp3d_wino_fused_split64": "i: ppppp iiiiiii p",
    "sp3d_conv3_split": "i: ppppp iiiiiii p",
    "sp3d_conv3_split_skip": "i: pppppp iiiiiii p",
    "sp3d_wino_fused_split64_skip": "i: pppppp iiiiiii p",
    "sp3d_upsample2x_scatter": "i: pppp l iiii p",
    "sp3d_upsample2x_scatter_head": "i: pppppp l iiiii p",
    "sp3d_upconv2x_fused": "i: ppppppp l iiiiii p",
    "sp3d_gbn_workspace_bytes": "l: ii",
    "sp3d_gbn_forward": "i: pp i pp i l iii pppp dd i ppppppp",
    "sp3d_gbn_backward": "i: ppp i pp i l ii ppppp i ppppppp",
}
TUNING_SIGNATURES = {                           # selfpose3d_amd/csrc/sp3d_tuning.h: measurement builds only, declared when present
    "sp3d_unproject_fwd_variant": "i: p i ppppp iiiiiiii p iii p",
    "sp3d_unproject_fwd_plan": "i: iii p iiiiiiiii pppp",
    "sp3d_debug_set_timeline": "i: p",
    "sp3d_debug_stamp": "i: pp",
}
EXPORTS = list(SIGNATURES)

_lib = None


class Sp3dError(RuntimeError):
    pass


def env_switch(name: str, default: bool) -> bool:
    """an on/off environment variable, read at every call: unset -> ``default``; "0" and "" -> off; anything else -> on"""
    return os.environ.get(name, "1" if default else "0") not in ("0", "")


def shared_gpu() -> bool:
    """SP3D_SHARED_GPU=1 (or, when the variable is unset and NO *_VISIBLE_DEVICES variable narrows what this process sees,
    more local ranks than GPUs): this process is not alone on its GPU (another process, or a second stream of its own, may run
    kernels at the same time).  The conservative library flavour is loaded then, libsp3d_nopk.so - no packed-fp32
    instruction at all.  Background (profiles/r05_mfma_pk_hazard.md): ONE packed-fp32 instruction form is wrong on MI355X
    while another kernel's double-rate matrix instructions run on the same CU; the build removes that form from the default
    flavour too (selfpose3d_amd/pk_src1.py), and tests/test_gpu_shared_gpu.py asserts both flavours on two streams."""
    v = os.environ.get("SP3D_SHARED_GPU")
    if v is not None:
        return v.lower() in ("1", "true", "yes", "on")
    # not told: a launcher that starts more local ranks than there are GPUs (torchrun's LOCAL_WORLD_SIZE) makes ranks share.
    # Only when the device count is the NODE's: a launcher that hands every rank one GPU through HIP_/CUDA_/ROCR_VISIBLE_DEVICES
    # makes device_count() == 1 on a perfectly normal one-process-per-GPU job (round-5 advice) - nothing can be inferred then.
    if any(os.environ.get(k) not in (None, "") for k in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES",
                                                          "GPU_DEVICE_ORDINAL")):
        return False
    try:
        ranks = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
        if ranks > 1 and torch.cuda.is_available() and ranks > torch.cuda.device_count():
            import warnings
            warnings.warn(f"selfpose3d_amd: {ranks} local ranks on {torch.cuda.device_count()} GPU(s) - ranks share a GPU: loading "
                          "libsp3d_nopk.so (no packed-fp32 instructions; set SP3D_SHARED_GPU=0 to force the default flavour)")
            return True
    except ValueError:
        pass
    return False


def load():
    """dlopen libsp3d.so (building nothing: run `python -m selfpose3d_amd.build` first)."""
    global _lib, LIB_PATH
    if _lib is not None:
        return _lib
    if shared_gpu() and LIB_PATH == _DEFAULT_LIB_PATH:
        LIB_PATH = NOPK_LIB_PATH
    if not os.path.exists(LIB_PATH):
        raise Sp3dError(
            f"{LIB_PATH} not found - the HIP extension is not built. Run `python -m selfpose3d_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the unprojection path.")
    lib = C.CDLL(LIB_PATH)
    for table, required in ((SIGNATURES, True), (TUNING_SIGNATURES, False)):
        for name, sig in table.items():
            if required or hasattr(lib, name):
                ret, args = sig.split(":")
                fn = getattr(lib, name)
                fn.restype = _CTYPES[ret]
                fn.argtypes = [_CTYPES[a] for a in args.replace(" ", "")]
    if lib.sp3d_abi_version() != ABI_VERSION:
        raise Sp3dError(f"libsp3d.so ABI {lib.sp3d_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().sp3d_error_string(rc).decode()
        raise Sp3dError(f"{what} failed: {msg} (code {rc})")


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise Sp3dError(f"{name} must live on the GPU (got {t.device}); the unprojection path has no CPU fallback")


CAM_STRIDE = 64     # floats per (sample, view) record, ABI version 2 (include/sp3d.h: SP3D_CAM_STRIDE)


def _require_cam(cam: torch.Tensor, name: str = "cam"):
    """the kernels read 64-float records (fields 0..29 + the derived block 32..62 written by sp3d_camera_finish /
    camera_pack.finish): a legacy 32-float table, another dtype or a strided view would be read out of bounds or as
    garbage WITHOUT any error from the C ABI (it sees a pointer), so the binding refuses them"""
    _require_cuda(cam, name)
    if cam.dim() < 2 or cam.shape[-1] != CAM_STRIDE or cam.dtype != torch.float32 or not cam.is_contiguous():
        raise Sp3dError(f"{name} must be a contiguous float32 (..., {CAM_STRIDE}) camera table built by camera_pack.pack_cameras "
                        f"(+ camera_pack.finish after edits); got shape {tuple(cam.shape)}, {cam.dtype}, "
                        f"contiguous={cam.is_contiguous()}")


def _ptr_array(tensors: Sequence[torch.Tensor]):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _f3(vals):
    return (C.c_float * 3)(float(vals[0]), float(vals[1]), float(vals[2]))


def _opt(t: Optional[torch.Tensor]):
    """device pointer of an optional tensor (None -> NULL)"""
    return None if t is None else t.data_ptr()


def _empty_cl3d(B: int, Cc: int, X: int, Y: int, Z: int, device, dtype=torch.float32) -> torch.Tensor:
    """uninitialised (B,C,X,Y,Z) result with torch.channels_last_3d strides (memory (B,X,Y,Z,C))"""
    return torch.empty((B, X, Y, Z, Cc), dtype=dtype, device=device).permute(0, 4, 1, 2, 3)


def _require_cl3d_f32(x: torch.Tensor, who: str):
    if not x.is_contiguous(memory_format=torch.channels_last_3d) or x.dtype != torch.float32:
        raise Sp3dError(f"{who}: float32 channels_last_3d activations expected")


def _result_cl3d(out: Optional[torch.Tensor], B: int, Cc: int, X: int, Y: int, Z: int, x: torch.Tensor, who: str) -> torch.Tensor:
    """the (B,C,X,Y,Z) channels_last_3d fp32 result of an entry: a fresh uninitialised tensor, or the caller's ``out`` (a
    view of a larger buffer, say) once it is that shape, type and layout on x's device - the kernels see only its pointer"""
    if out is None:
        return _empty_cl3d(B, Cc, X, Y, Z, x.device)
    _require_cl3d_f32(out, who)
    if out.device != x.device or tuple(out.shape) != (B, Cc, X, Y, Z):
        raise Sp3dError(f"{who}: out must be ({B}, {Cc}, {X}, {Y}, {Z}) on {x.device}, got {tuple(out.shape)} on {out.device}")
    return out


def _result_dense(out: Optional[torch.Tensor], shape, dtype, device, who: str, align: int = 1, cl3d: bool = False) -> torch.Tensor:
    """the result of an entry of the opening conv: a fresh uninitialised tensor, or the caller's ``out`` (a view of a larger
    buffer, say) once it is that shape and type on that device, dense (``cl3d``: in channels_last_3d order) and aligned to
    the ``align`` bytes the C entry demands of its pointer - the kernels see only that pointer"""
    shape = tuple(int(v) for v in shape)
    if out is None:
        return _empty_cl3d(*shape, device, dtype) if cl3d else torch.empty(shape, dtype=dtype, device=device)
    dense = out.permute(0, 2, 3, 4, 1).is_contiguous() if cl3d and out.dim() == 5 else out.is_contiguous()
    if tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not dense or out.data_ptr() % align:
        raise Sp3dError(f"{who}: out must be a dense {dtype} {shape} tensor on {device}, {align}-byte aligned; got "
                        f"{tuple(out.shape)}, {out.dtype}, {out.device}, strides {tuple(out.stride())}, address % {align} = "
                        f"{out.data_ptr() % align}")
    return out


def _as_cl3d(t: torch.Tensor) -> torch.Tensor:
    """a residual / skip operand as the kernels read it, dense channels_last_3d like the result it is added to; copies
    only when it is not that already (.contiguous returns its argument otherwise, so one condition covers every case)"""
    return t if t.is_contiguous(memory_format=torch.channels_last_3d) else t.contiguous(memory_format=torch.channels_last_3d)


def pack_heatmaps(hms: Sequence[torch.Tensor], jp: int = 16, out: Optional[torch.Tensor] = None,
                  out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """list[V] of (B,J,h,w) fp32|bf16 contiguous -> (V,B,h,w,jp) channels-last (fp32|bf16), padded channels zero."""
    lib = load()
    h0 = hms[0]
    _require_cuda(h0, "heatmaps")
    B, J, h, w = h0.shape
    V = len(hms)
    in_dt = torch.bfloat16 if h0.dtype == torch.bfloat16 else torch.float32
    hms = [x if (x.is_contiguous() and x.dtype == in_dt) else x.contiguous().to(in_dt) for x in hms]
    out_dtype = out.dtype if out is not None else (out_dtype or torch.float32)
    if out is None:
        out = torch.empty((V, B, h, w, jp), dtype=out_dtype, device=h0.device)
    check(lib.sp3d_pack_heatmaps_ex(_ptr_array(hms), out.data_ptr(), int(in_dt == torch.bfloat16),
                                    int(out_dtype == torch.bfloat16), B, V, J, jp, h, w, _stream(h0.device)),
          "sp3d_pack_heatmaps")
    return out


def unproject_fwd(views: Sequence[torch.Tensor], layout: int, jp: int, cam: torch.Tensor, centers: torch.Tensor,
                  valid: torch.Tensor, B: int, J: int, h: int, w: int, cube_size, grid_size, img_size,
                  want_grids: bool = True, variant: Optional[int] = None, channels_last: bool = False,
                  sample_of: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32,
                  pass_mask: Optional[torch.Tensor] = None, wide_mask: bool = False, out: Optional[torch.Tensor] = None,
                  one_channel: bool = False):
    """-> (cubes (B,J,X,Y,Z), grids (B,N,3) | None).  With ``channels_last`` the cubes tensor has
    torch.channels_last_3d strides (memory (B,X,Y,Z,J), J % 4 == 0, NHWC input only).
    ``sample_of`` (int32, (B,)): output cube p reads heat-map/camera row sample_of[p] (B = #cubes).
    ``out``: a (B,J,X,Y,Z) VIEW of a larger buffer (z contiguous, e.g. the zero-padded FFT input of the opening
    conv): the planar result is written straight into it (sp3d_unproject_fwd_strided).
    ``one_channel`` (SP3D_HM_ONE_CHANNEL): ``views[c]`` is any fp32 tensor (or bf16: SP3D_HM_BF16_IN, derived from the dtype; the
    result stays fp32) whose ``data_ptr()`` is the wanted channel's first
    element of view c - a (B,1,h,w) slice of a planar (B,jp,h,w) tensor (``LAYOUT_PLANAR``, ``jp`` = its channel count) or
    of a channels-last (B,h,w,jp) buffer (``LAYOUT_NHWC``, ``jp`` = its pixel stride) - read in place; ``J`` = channels
    written, 1 or 4 (value + three zero channels; channels-last results: 4).
    ``wide_mask`` (SP3D_HM_WIDE_MASK, with ``pass_mask`` at ``jp`` = 32 only): ``pass_mask`` is a contiguous (2, B, X*Y*Z)
    int16 tensor, plane 0 for channels 0-15 and plane 1 for channels 16..J-1.
    bf16 ``views`` with a ``pass_mask`` (SP3D_HM_BF16_TRAIN, derived from the dtype; ``out_dtype`` stays fp32): bf16 pixels of
    ``jp`` = 16, or 32 with ``wide_mask``; cubes, grids and mask words are those of the call on the widened views."""
    lib = load()
    dev = cam.device
    _require_cam(cam)
    X, Y, Z = (int(c) for c in cube_size)
    V = len(views)
    one = HM_ONE_CHANNEL if one_channel else 0
    if one_channel:
        assert pass_mask is None and variant is None and out_dtype == torch.float32 and jp >= 1
        # bf16 maps (SP3D_HM_BF16_IN): read in place as well - 2-byte elements, fp32 result
        assert views[0].dtype in (torch.float32, torch.bfloat16) and all(v.dtype == views[0].dtype for v in views)
        if views[0].dtype == torch.bfloat16:
            one |= HM_BF16_IN
    if out is not None:
        assert (layout == LAYOUT_NHWC or one_channel) and not channels_last and not want_grids and pass_mask is None and variant is None
        assert tuple(out.shape) == (B, J, X, Y, Z) and out.stride(4) == 1 and out.dtype == out_dtype
        flags = (HM_BF16 if views[0].dtype == torch.bfloat16 and not one_channel else 0) | \
            (OUT_BF16 if out_dtype == torch.bfloat16 else 0) | one
        st = (C.c_int64 * 4)(*[int(v) for v in out.stride()[:4]])
        rc = lib.sp3d_unproject_fwd_strided(_ptr_array(views), layout | flags, jp, cam.data_ptr(), _opt(sample_of),
                                            centers.data_ptr(), valid.data_ptr(), out.data_ptr(), st, B, V, J, h, w, X, Y, Z,
                                            _f3(grid_size), int(img_size[0]), int(img_size[1]), _stream(dev))
        check(rc, "sp3d_unproject_fwd_strided")
        return out, None
    if channels_last:
        cubes = _empty_cl3d(B, J, X, Y, Z, dev, out_dtype)
    else:
        cubes = torch.empty((B, J, X, Y, Z), dtype=out_dtype, device=dev)
    bf16_in = views[0].dtype == torch.bfloat16 and not one_channel
    if pass_mask is not None and not all(v.dtype == views[0].dtype for v in views):
        raise Sp3dError("unproject_fwd(pass_mask=...): bf16 views or fp32 views expected, not a mixture")
    flags = (OUT_CHANNELS_LAST if channels_last else 0) | (OUT_BF16 if out_dtype == torch.bfloat16 else 0) | one | \
        ((HM_BF16 if pass_mask is None else HM_BF16_TRAIN) if bf16_in else 0)
    grids = torch.empty((B, X * Y * Z, 3), dtype=torch.float32, device=dev) if want_grids else None
    gs = _f3(grid_size)
    if wide_mask:
        if pass_mask is None or pass_mask.dtype != torch.int16 or not pass_mask.is_contiguous() or \
                pass_mask.numel() != 2 * B * X * Y * Z:
            raise Sp3dError("unproject_fwd(wide_mask=True): pass_mask must be a contiguous int16 (2, B, X*Y*Z) tensor")
        flags |= HM_WIDE_MASK
    if pass_mask is not None:
        rc = lib.sp3d_unproject_fwd_train(_ptr_array(views), layout | flags, jp, cam.data_ptr(), _opt(sample_of),
                                          centers.data_ptr(), valid.data_ptr(), cubes.data_ptr(), _opt(grids),
                                          pass_mask.data_ptr(), B, V, J, h, w, X, Y, Z, gs, int(img_size[0]),
                                          int(img_size[1]), _stream(dev))
    elif variant is None:
        rc = lib.sp3d_unproject_fwd_indexed(_ptr_array(views), layout | flags, jp, cam.data_ptr(), _opt(sample_of),
                                            centers.data_ptr(), valid.data_ptr(), cubes.data_ptr(), _opt(grids),
                                            B, V, J, h, w, X, Y, Z, gs, int(img_size[0]), int(img_size[1]), _stream(dev))
    else:
        assert layout == LAYOUT_NHWC
        rc = lib.sp3d_unproject_fwd_variant(_ptr_array(views), jp, cam.data_ptr(), centers.data_ptr(), valid.data_ptr(),
                                            cubes.data_ptr(), _opt(grids), B, V, J, h, w, X, Y, Z, gs, int(img_size[0]),
                                            int(img_size[1]), int(variant) | (0x1000000 if channels_last else 0), _stream(dev))
    check(rc, "sp3d_unproject_fwd")
    return cubes, grids


PLAN_ENTRIES = ("indexed", "strided", "train", "zdft", "variant", "one_train")      # SP3D_PLAN_* (csrc/sp3d_tuning.h)
PLAN_FIELDS = ("workgroups", "block", "lds", "nscalars", "s0", "s1", "s2", "s3", "J", "xcd_chunk", "xcd_order", "xm_mode", "xm_log2xps",
               "xm_log2K", "xm_rows", "xm_tiles", "xm_magic_tiles", "bk_nxy", "bk_nby", "bk_magic_nxy", "bk_magic_nby", "blk_log2py",
               "blk_w", "blk_h", "blk_nbx", "blk_nzc", "blk_magic_wh", "blk_magic_h", "view_off", "out_off", "grids")
PLAN_TUNING = ("unroll", "no_xcd_map", "pipe", "one_wave", "brick", "brick_own_wg", "z_fastest", "view_sync", "ballast", "forced_chunk",
               "plain_sweep", "chunk_map")


def unproject_fwd_plan(entry: str, layout: int, jp: int, B: int, V: int, J: int, h: int, w: int, cube_size, variant: int = 0,
                       out_strides=None):
    """Measurement only, no GPU: what the forward unprojection would launch for a request given as shapes
    (sp3d_unproject_fwd_plan) -> (rc, launches, tuning): per launch a dict of its kernel ``name`` and PLAN_FIELDS (magic
    numbers as unsigned), and the decoded tuning as a dict of PLAN_TUNING; ``launches`` is empty when rc is a refusal."""
    lib = load()
    names = C.create_string_buffer(2 * 96)
    fields, tuning, n = (C.c_int32 * (2 * len(PLAN_FIELDS)))(), (C.c_int32 * len(PLAN_TUNING))(), C.c_int32(0)
    st = (C.c_int64 * 4)(*[int(v) for v in out_strides]) if out_strides is not None else None
    X, Y, Z = (int(c) for c in cube_size)
    rc = lib.sp3d_unproject_fwd_plan(PLAN_ENTRIES.index(entry), layout, jp, st, B, V, J, h, w, X, Y, Z, int(variant), names, fields,
                                     tuning, C.byref(n))
    launches = []
    for i in range(n.value if rc == 0 else 0):
        f = fields[i * len(PLAN_FIELDS):(i + 1) * len(PLAN_FIELDS)]
        launches.append(dict(zip(PLAN_FIELDS, (v & 0xFFFFFFFF if "magic" in k else v for k, v in zip(PLAN_FIELDS, f))),
                             name=names.raw[i * 96:(i + 1) * 96].split(b"\0")[0].decode()))
    return rc, launches, dict(zip(PLAN_TUNING, tuning))


def unproject_bwd(hms: Sequence[torch.Tensor], cam, centers, valid, grad_cubes: torch.Tensor, cube_size, grid_size,
                  img_size, sample_of: Optional[torch.Tensor] = None):
    lib = load()
    dev = cam.device
    _require_cam(cam)
    B, J, h, w = hms[0].shape
    P = int(grad_cubes.shape[0])
    X, Y, Z = (int(c) for c in cube_size)
    V = len(hms)
    hms = [x if x.dtype == torch.float32 else x.float() for x in hms]
    grad_cubes = grad_cubes[:, :J].float().contiguous()
    grads = torch.zeros((V, B, J, h, w), dtype=torch.float32, device=dev)
    gviews = [grads[c] for c in range(V)]
    rc = lib.sp3d_unproject_bwd_indexed(_ptr_array(hms), cam.data_ptr(), _opt(sample_of), centers.data_ptr(),
                                        valid.data_ptr(), grad_cubes.data_ptr(), _ptr_array(gviews), P, V, J, h, w, X,
                                        Y, Z, _f3(grid_size), int(img_size[0]), int(img_size[1]), _stream(dev))
    check(rc, "sp3d_unproject_bwd")
    return gviews


def nms_proposals(root_cubes: torch.Tensor, k: int, grid_size, grid_center, threshold: float) -> torch.Tensor:
    """(B,X,Y,Z) -> grid_centers (B,k,5) = [x,y,z mm, (score > threshold) - 1, score]: NMS, top-k, index -> mm and the
    eval-mode proposal flags in the same two launches (no torch glue kernels)."""
    lib = load()
    _require_cuda(root_cubes, "root_cubes")
    rc_ = root_cubes.contiguous().float()
    B, X, Y, Z = rc_.shape
    dev = rc_.device
    out = torch.empty((B, k, 5), dtype=torch.float32, device=dev)
    scratch = torch.empty((B * k * (1 + 3) * 4 + B * k * 3 * 8,), dtype=torch.uint8, device=dev)
    vals = scratch[:B * k * 4].view(torch.float32)
    locs = scratch[B * k * 4:B * k * 16].view(torch.float32)
    idx = scratch[B * k * 16:].view(torch.int64)
    nbytes = lib.sp3d_nms_topk_workspace_bytes(B, X, Y, Z, k)
    ws = torch.empty((max(int(nbytes), 8),), dtype=torch.uint8, device=dev)
    rc = lib.sp3d_nms_proposals(rc_.data_ptr(), B, X, Y, Z, k, _f3(grid_size), _f3(grid_center), C.c_float(float(threshold)),
                                vals.data_ptr(), idx.data_ptr(), locs.data_ptr(), out.data_ptr(), ws.data_ptr(), _stream(dev))
    check(rc, "sp3d_nms_proposals")
    return out


def nms_topk(root_cubes: torch.Tensor, k: int, grid_size=None, grid_center=None):
    """(B,X,Y,Z) -> vals (B,k) fp32, idx (B,k,3) int64, locs (B,k,3) fp32 mm (None without grid_size)."""
    lib = load()
    _require_cuda(root_cubes, "root_cubes")
    rc_ = root_cubes.contiguous().float()
    B, X, Y, Z = rc_.shape
    dev = rc_.device
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    idx = torch.empty((B, k, 3), dtype=torch.int64, device=dev)
    locs = torch.empty((B, k, 3), dtype=torch.float32, device=dev) if grid_size is not None else None
    nbytes = lib.sp3d_nms_topk_workspace_bytes(B, X, Y, Z, k)
    ws = torch.empty((max(int(nbytes), 8),), dtype=torch.uint8, device=dev)
    rc = lib.sp3d_nms_topk(rc_.data_ptr(), B, X, Y, Z, k, _f3(grid_size) if grid_size is not None else None,
                           _f3(grid_center) if grid_center is not None else None, vals.data_ptr(), idx.data_ptr(),
                           _opt(locs), ws.data_ptr(), _stream(dev))
    check(rc, "sp3d_nms_topk")
    return vals, idx, locs


def soft_argmax(x: torch.Tensor, grids: torch.Tensor, beta: float) -> torch.Tensor:
    """x (Bv,J,X,Y,Z) or (Bv,J,N); grids (Bv,N,3) -> (Bv,J,3)"""
    lib = load()
    _require_cuda(x, "x")
    Bv, J = x.shape[:2]
    xc = x.contiguous().float().reshape(Bv, J, -1)
    N = xc.shape[2]
    gc = grids.contiguous().float()
    out = torch.empty((Bv, J, 3), dtype=torch.float32, device=x.device)
    if Bv == 0:
        return out
    check(lib.sp3d_soft_argmax(xc.data_ptr(), gc.data_ptr(), out.data_ptr(), Bv, J, N, float(beta), _stream(x.device)),
          "sp3d_soft_argmax")
    return out


def soft_argmax_grid(x: torch.Tensor, centers: torch.Tensor, grid_size, cube_size, beta: float) -> torch.Tensor:
    """soft-argmax with voxel centres regenerated in-kernel: x (P,J,X,Y,Z), centers (P,3) -> (P,J,3)"""
    lib = load()
    _require_cuda(x, "x")
    P, J = x.shape[:2]
    X, Y, Z = (int(c) for c in cube_size)
    xc = x.contiguous().float()
    cc = centers.contiguous().float()
    out = torch.empty((P, J, 3), dtype=torch.float32, device=x.device)
    if P == 0:
        return out
    check(lib.sp3d_soft_argmax_grid(xc.data_ptr(), cc.data_ptr(), _f3(grid_size), X, Y, Z, out.data_ptr(), P, J,
                                    float(beta), _stream(x.device)), "sp3d_soft_argmax_grid")
    return out


class _SoftArgmaxGridFn(torch.autograd.Function):
    """soft-argmax with in-kernel voxel centres under autograd (training pose net): forward = sp3d_soft_argmax_grid_train (also
    keeps max and sum per row), backward = ONE elementwise pass (sp3d_soft_argmax_grid_bwd) instead of the softmax / product /
    sum graph over a (P,J,N,3) temporary"""

    @staticmethod
    def forward(ctx, x, centers, grid_size, cube_size, beta):
        lib = load()
        _require_cuda(x, "x")
        P, J = int(x.shape[0]), int(x.shape[1])
        X, Y, Z = (int(c) for c in cube_size)
        xc = x.detach().contiguous().float()                      # planar (P,J,N)
        cc = centers.detach().contiguous().float()
        out = torch.empty((P, J, 3), dtype=torch.float32, device=x.device)
        stats = torch.empty((P, J, 2), dtype=torch.float32, device=x.device)
        check(lib.sp3d_soft_argmax_grid_train(xc.data_ptr(), cc.data_ptr(), _f3(grid_size), X, Y, Z, out.data_ptr(),
                                              stats.data_ptr(), P, J, float(beta), _stream(x.device)), "sp3d_soft_argmax_grid_train")
        ctx.save_for_backward(xc, cc, out, stats)
        ctx.geom = (tuple(float(v) for v in grid_size), (X, Y, Z), float(beta), x.is_contiguous(memory_format=torch.channels_last_3d)
                    and not x.is_contiguous())
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load()
        xc, cc, out, stats = ctx.saved_tensors
        grid_size, (X, Y, Z), beta, cl = ctx.geom
        P, J = int(xc.shape[0]), int(xc.shape[1])
        dx = torch.empty_like(xc)
        gc = g.contiguous().float()
        check(lib.sp3d_soft_argmax_grid_bwd(xc.data_ptr(), cc.data_ptr(), _f3(grid_size), X, Y, Z, out.data_ptr(), stats.data_ptr(),
                                            gc.data_ptr(), dx.data_ptr(), P, J, beta, _stream(xc.device)), "sp3d_soft_argmax_grid_bwd")
        if cl:
            dx = dx.contiguous(memory_format=torch.channels_last_3d)
        return dx, None, None, None, None


def soft_argmax_grid_autograd(x: torch.Tensor, centers: torch.Tensor, grid_size, cube_size, beta: float) -> torch.Tensor:
    """x (P,J,X,Y,Z) fp32 (gradient flows to it), centers (P,3) -> (P,J,3)"""
    if int(x.shape[0]) == 0:
        return x.new_zeros((0, int(x.shape[1]), 3))
    return _SoftArgmaxGridFn.apply(x, centers, grid_size, cube_size, beta)


def fetch_ring(ring: torch.Tensor, dst: torch.Tensor, counter: torch.Tensor):
    """graph-capturable: dst <- ring[counter % R] (ring: PINNED host tensor (R, ...)), counter += 1 (device int32)"""
    lib = load()
    assert ring.is_pinned() and ring.dtype == torch.float32 and dst.is_cuda and counter.is_cuda
    R = int(ring.shape[0])
    n = ring[0].numel()
    assert dst.numel() == n and dst.is_contiguous() and ring.is_contiguous()
    check(lib.sp3d_fetch_ring(ring.data_ptr(), dst.data_ptr(), counter.data_ptr(), R, n, _stream(dst.device)),
          "sp3d_fetch_ring")


def maxpool2x(x: torch.Tensor, have: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxPool3d(2,2) of a channels_last_3d tensor (B,C,X,Y,Z) -> channels_last_3d (B,C,X/2,Y/2,Z/2).  ``have``: the pooled
    tensor where the kernel that made x has already written it (conv3_split_ / wino_fused_conv3d_ with pool=True): checked
    against x (shape, device, type, layout) and returned, no launch."""
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    if have is not None:
        if tuple(have.shape) != (B, Cc, X // 2, Y // 2, Z // 2) or have.device != x.device or have.dtype != torch.float32 or \
                x.dtype != torch.float32 or not have.is_contiguous(memory_format=torch.channels_last_3d):
            raise Sp3dError(f"maxpool2x: have must be the float32 channels_last_3d ({B}, {Cc}, {X // 2}, {Y // 2}, {Z // 2}) pooled "
                            f"form of x on {x.device}; got {tuple(have.shape)}, {have.dtype}, {have.device}")
        return have
    lib = load()
    y = _empty_cl3d(B, Cc, X // 2, Y // 2, Z // 2, x.device)
    check(lib.sp3d_maxpool2x_cl(x.data_ptr(), y.data_ptr(), B, X, Y, Z, Cc, _stream(x.device)), "sp3d_maxpool2x_cl")
    return y


def rfft3d(x: torch.Tensor) -> torch.Tensor:
    """unnormalised rFFT over the last three dims of a dense fp32 (..., SX,SY,SZ) tensor -> complex64 (..., SX,SY,SZ//2+1);
    x is only read (no defensive clone, unlike torch.fft.rfftn on ROCm)"""
    lib = load()
    _require_cuda(x, "x")
    if not x.is_contiguous() or x.dtype != torch.float32 or x.dim() < 3:
        raise Sp3dError("rfft3d: x must be a dense fp32 tensor with >= 3 dims")
    SX, SY, SZ = (int(v) for v in x.shape[-3:])
    batch = int(x.numel() // (SX * SY * SZ))
    out = torch.empty(tuple(x.shape[:-1]) + (SZ // 2 + 1,), dtype=torch.complex64, device=x.device)
    check(lib.sp3d_rfft3d(x.data_ptr(), out.data_ptr(), batch, SX, SY, SZ, _stream(x.device)), "sp3d_rfft3d")
    return out


def irfft3d_(spec: torch.Tensor, SZ: int) -> torch.Tensor:
    """unnormalised inverse of rfft3d: complex64 (..., SX,SY,SZ//2+1) -> fp32 (..., SX,SY,SZ).  `spec` is scratch
    afterwards (the C2R plan may overwrite it)"""
    lib = load()
    _require_cuda(spec, "spec")
    if not spec.is_contiguous() or spec.dtype != torch.complex64 or spec.dim() < 3 or spec.shape[-1] != SZ // 2 + 1:
        raise Sp3dError("irfft3d_: spec must be a dense complex64 (..., SX,SY,SZ//2+1) tensor")
    SX, SY = (int(v) for v in spec.shape[-3:-1])
    batch = int(spec.numel() // (SX * SY * (SZ // 2 + 1)))
    out = torch.empty(tuple(spec.shape[:-1]) + (int(SZ),), dtype=torch.float32, device=spec.device)
    check(lib.sp3d_irfft3d(spec.data_ptr(), out.data_ptr(), batch, SX, SY, int(SZ), _stream(spec.device)), "sp3d_irfft3d")
    return out


ZDFT_SHAPES = {(20, 28, 16)}       # (Z, SZ, channels) the direct z-DFT kernels are built for


def cfft2d_(spec: torch.Tensor, inverse: bool, rows_in: Optional[int] = None, rows_out: Optional[int] = None,
             library: bool = False) -> torch.Tensor:
    """in-place unnormalised 2-D complex FFT over the last two dims of a dense complex64 tensor.  rows_in: only the first
    rows_in rows of each input plane are non-zero; rows_out: only the first rows_out rows of each result are needed (the
    rest is unspecified).  library=True forces the hipFFT plan (whole planes)."""
    lib = load()
    _require_cuda(spec, "spec")
    if not spec.is_contiguous() or spec.dtype != torch.complex64 or spec.dim() < 2:
        raise Sp3dError("cfft2d_: dense complex64 tensor with >= 2 dims expected")
    SX, SY = int(spec.shape[-2]), int(spec.shape[-1])
    batch = int(spec.numel() // (SX * SY))
    if library:
        check(lib.sp3d_cfft2d(spec.data_ptr(), batch, SX, SY, 1 if inverse else 0, _stream(spec.device)), "sp3d_cfft2d")
    else:
        check(lib.sp3d_cfft2d_ex(spec.data_ptr(), batch, SX, SY, 1 if inverse else 0, SX if rows_in is None else int(rows_in),
                                 SX if rows_out is None else int(rows_out), _stream(spec.device)), "sp3d_cfft2d_ex")
    return spec


def zdft_fwd_cl(x: torch.Tensor, cout: int, S, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """channels_last_3d (B,C,X,Y,Z) real -> (B,cout,SZ//2+1,SX,SY) complex64: z-DFT of the rows zero-padded to S"""
    lib = load()
    _require_cuda(x, "x")
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    if x.dtype != torch.float32 or not x.permute(0, 2, 3, 4, 1).is_contiguous():
        raise Sp3dError("zdft_fwd_cl: dense fp32 channels_last_3d cubes expected")
    SX, SY, SZ = (int(v) for v in S)
    spec = _result_dense(out, (B, int(cout), SZ // 2 + 1, SX, SY), torch.complex64, x.device, "zdft_fwd_cl")
    check(lib.sp3d_zdft_fwd_cl(x.data_ptr(), spec.data_ptr(), B, Cc, int(cout), X, Y, Z, SX, SY, SZ, _stream(x.device)),
          "sp3d_zdft_fwd_cl")
    return spec


def unproject_fwd_zdft(views: Sequence[torch.Tensor], jp: int, cam: torch.Tensor, centers: torch.Tensor, valid: torch.Tensor,
                       batch: int, J: int, h: int, w: int, cube_size, grid_size, img_size, SZ: int, *,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """root grid, inference: the unprojection's result as the z-spectrum of its cubes (include/sp3d.h,
    sp3d_unproject_fwd_zdft) -> (B, J, SZ//2+1, X/4, Y/4, 16) complex64, 4 x 4-tiled planes without padding"""
    lib = load()
    _require_cam(cam)
    X, Y, Z = (int(c) for c in cube_size)
    for v in views:
        _require_cuda(v, "heat-map view")
        if v.dtype != torch.float32 or not v.is_contiguous() or tuple(v.shape) != (batch, h, w, jp):
            raise Sp3dError("unproject_fwd_zdft: dense fp32 (B,h,w,16) heat-map views expected")
    if (Z, int(SZ), jp) not in ZDFT_SHAPES or X % 4 or Y % 4:
        raise Sp3dError(f"unproject_fwd_zdft: built for (Z, SZ, channels) in {sorted(ZDFT_SHAPES)} and X, Y multiples of 4")
    spec = _result_dense(out, (batch, J, int(SZ) // 2 + 1, X // 4, Y // 4, 16), torch.complex64, cam.device, "unproject_fwd_zdft", 128)
    check(lib.sp3d_unproject_fwd_zdft(_ptr_array(views), jp, cam.data_ptr(), centers.data_ptr(), valid.data_ptr(),
                                      spec.data_ptr(), batch, len(views), J, h, w, X, Y, Z, _f3(grid_size), int(img_size[0]),
                                      int(img_size[1]), int(SZ), _stream(cam.device)), "sp3d_unproject_fwd_zdft")
    return spec


def unproject_fwd_zspectrum(views: Sequence[torch.Tensor], jp: int, cam: torch.Tensor, centers: torch.Tensor, valid: torch.Tensor,
                            batch: int, J: int, h: int, w: int, cube_size, grid_size, img_size, SZ: int, *,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``unproject_fwd_zdft`` through the flag SP3D_OUT_ZSPECTRUM of sp3d_unproject_fwd (include/sp3d.h): packed pixels of
    ``jp`` = 16 (J <= 16, the same launch) or 32 (J <= 32, one launch per channel group) -> ONE
    (B, J, SZ//2+1, X/4, Y/4, 16) complex64 spectrum over all J channels"""
    lib = load()
    _require_cam(cam)
    X, Y, Z = (int(c) for c in cube_size)
    if jp not in (16, 32) or not 1 <= J <= jp:
        raise Sp3dError(f"unproject_fwd_zspectrum: packed pixels of 16 or 32 channels and J <= jp expected, got jp {jp}, J {J}")
    dt = views[0].dtype         # bf16 maps: SP3D_HM_BF16_IN (the brick-h kernels with the z-spectrum result), fp32 spectrum
    for v in views:
        _require_cuda(v, "heat-map view")
        if v.dtype not in (torch.float32, torch.bfloat16) or v.dtype != dt or not v.is_contiguous() or \
                tuple(v.shape) != (batch, h, w, jp):
            raise Sp3dError(f"unproject_fwd_zspectrum: dense fp32 or bf16 (B,h,w,{jp}) heat-map views expected")
    if (Z, int(SZ), 16) not in ZDFT_SHAPES or X % 4 or Y % 4:
        raise Sp3dError(f"unproject_fwd_zspectrum: built for (Z, SZ, channels) in {sorted(ZDFT_SHAPES)} and X, Y multiples of 4")
    spec = _result_dense(out, (batch, J, int(SZ) // 2 + 1, X // 4, Y // 4, 16), torch.complex64, cam.device,
                         "unproject_fwd_zspectrum", 128)
    flags = LAYOUT_NHWC | OUT_ZSPECTRUM | (HM_BF16_IN if dt == torch.bfloat16 else 0)
    check(lib.sp3d_unproject_fwd(_ptr_array(views), flags, jp, cam.data_ptr(), centers.data_ptr(),
                                 valid.data_ptr(), spec.data_ptr(), None, batch, len(views), J, h, w, X, Y, Z, _f3(grid_size),
                                 int(img_size[0]), int(img_size[1]), _stream(cam.device)), "sp3d_unproject_fwd (z-spectrum)")
    return spec


def unproject_one_fwd_zspectrum(views: Sequence[torch.Tensor], layout: int, jp: int, cam: torch.Tensor, centers: torch.Tensor,
                                valid: torch.Tensor, batch: int, h: int, w: int, cube_size, grid_size, img_size, SZ: int, *,
                                sample_of: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the one-channel read of ``unproject_fwd(one_channel=True)`` (``views``, ``layout`` and ``jp`` as documented there) with
    the result of ``unproject_fwd_zdft`` at J = 1 (SP3D_HM_ONE_ZSPECTRUM, include/sp3d.h): one launch, no cubes ->
    (P, 1, SZ//2+1, X/4, Y/4, 16) complex64, P = ``batch`` cubes (``sample_of``: cube p reads sample sample_of[p])"""
    lib = load()
    _require_cam(cam)
    X, Y, Z = (int(c) for c in cube_size)
    for v in views:
        _require_cuda(v, "heat-map view")
        if v.dtype not in (torch.float32, torch.bfloat16) or v.dtype != views[0].dtype:
            raise Sp3dError("unproject_one_fwd_zspectrum: fp32 or bf16 heat-map views of one type expected")
    if (Z, int(SZ)) != (20, 28) or X % 4 or Y % 4:
        raise Sp3dError("unproject_one_fwd_zspectrum: built for (Z, SZ) = (20, 28) and X, Y multiples of 4")
    spec = _result_dense(out, (batch, 1, int(SZ) // 2 + 1, X // 4, Y // 4, 16), torch.complex64, cam.device,
                         "unproject_one_fwd_zspectrum", 128)
    flags = layout | HM_ONE_ZSPECTRUM | (HM_BF16_IN if views[0].dtype == torch.bfloat16 else 0)
    check(lib.sp3d_unproject_fwd_indexed(_ptr_array(views), flags, jp, cam.data_ptr(), _opt(sample_of),
                                         centers.data_ptr(), valid.data_ptr(), spec.data_ptr(), None, batch, len(views), 1, h, w,
                                         X, Y, Z, _f3(grid_size), int(img_size[0]), int(img_size[1]), _stream(cam.device)),
          "sp3d_unproject_fwd_indexed (one-channel z-spectrum)")
    return spec


def cfft2d_88_tiled(spec: torch.Tensor, X: int, Y: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(..., X/4, Y/4, 16) complex64 tiled planes -> (..., 88, 88) complex64: forward x,y transform of the zero-padded planes"""
    lib = load()
    _require_cuda(spec, "spec")
    if spec.dtype != torch.complex64 or not spec.is_contiguous() or tuple(spec.shape[-3:]) != (X // 4, Y // 4, 16):
        raise Sp3dError("cfft2d_88_tiled: dense complex64 (..., X/4, Y/4, 16) expected")
    out = _result_dense(out, tuple(spec.shape[:-3]) + (88, 88), torch.complex64, spec.device, "cfft2d_88_tiled", 16)
    batch = out.numel() // (88 * 88)
    check(lib.sp3d_cfft2d_88_tiled(spec.data_ptr(), out.data_ptr(), batch, int(X), int(Y), _stream(spec.device)),
          "sp3d_cfft2d_88_tiled")
    return out


def zdft_inv_cl(spec: torch.Tensor, X: int, Y: int, Z: int, SZ: int, shift: torch.Tensor, relu: bool = True, *,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,O,SZ//2+1,SX,SY) complex64 -> channels_last_3d (B,O,X,Y,Z) = act(shift[o] + unnormalised C2R along z)"""
    lib = load()
    _require_cuda(spec, "spec")
    if not spec.is_contiguous() or spec.dtype != torch.complex64 or spec.dim() != 5 or spec.shape[2] != SZ // 2 + 1:
        raise Sp3dError("zdft_inv_cl: dense complex64 (B,O,SZ//2+1,SX,SY) spectrum expected")
    B, O, _, SX, SY = (int(v) for v in spec.shape)
    y = _result_dense(out, (B, O, X, Y, Z), torch.float32, spec.device, "zdft_inv_cl", 16, cl3d=True)
    check(lib.sp3d_zdft_inv_cl(spec.data_ptr(), y.data_ptr(), shift.data_ptr(), B, O, X, Y, Z, SX, SY, int(SZ),
                               1 if relu else 0, _stream(spec.device)), "sp3d_zdft_inv_cl")
    return y


def crop_shift_act_cl(src: torch.Tensor, X: int, Y: int, Z: int, shift: torch.Tensor, relu: bool = True, *,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """planar (B,C,SX,SY,SZ) -> channels_last_3d (B,C,X,Y,Z) = act(src[:, :, :X, :Y, :Z] + shift[c]) in one pass"""
    lib = load()
    _require_cuda(src, "src")
    if not src.is_contiguous() or src.dtype != torch.float32:
        raise Sp3dError("crop_shift_act_cl: src must be a dense fp32 (B,C,SX,SY,SZ) tensor")
    B, Cc, SX, SY, SZ = (int(v) for v in src.shape)
    y = _result_dense(out, (B, Cc, X, Y, Z), torch.float32, src.device, "crop_shift_act_cl", 16, cl3d=True)
    check(lib.sp3d_crop_shift_act_cl(src.data_ptr(), y.data_ptr(), shift.data_ptr(), B, Cc, X, Y, Z, SX, SY, SZ,
                                     1 if relu else 0, _stream(src.device)), "sp3d_crop_shift_act_cl")
    return y


def channel_shift_act_(y: torch.Tensor, shift: torch.Tensor, mode: int, residual: Optional[torch.Tensor] = None):
    """in place on a 5-D activation (B,C,D,H,W) that is dense in NCDHW or channels_last_3d order:
    mode 0 y+=shift[c]; 1 relu(y+shift); 2 relu(y+shift+residual); 3 relu(y+shift)+residual"""
    lib = load()
    _require_cuda(y, "y")
    B, Cc = int(y.shape[0]), int(y.shape[1])
    inner = int(y.numel() // max(1, B * Cc))
    if y.is_contiguous():
        cl = 0
    elif y.is_contiguous(memory_format=torch.channels_last_3d):
        cl = 1
    else:
        raise Sp3dError("channel_shift_act_: activation must be dense (NCDHW or channels_last_3d)")
    if residual is not None:
        if residual.shape != y.shape or residual.stride() != y.stride():
            residual = residual.contiguous(memory_format=torch.channels_last_3d if cl else torch.contiguous_format)
    check(lib.sp3d_channel_shift_act(y.data_ptr(), shift.data_ptr(), _opt(residual), int(mode), B, Cc, inner, cl,
                                     _stream(y.device)), "sp3d_channel_shift_act")
    return y


def _fixed_point_scale(gmax: torch.Tensor, taps: int) -> torch.Tensor:
    """the scale of the deterministic scatters, (1,) fp32 on the device (no host synchronisation): 2^(s - ceil(log2 max|g|)),
    so that 2^s steps span the largest gradient.  A pixel receives at most ``taps`` = 4 N P contributions (4 taps of every voxel
    of every cube), each below 2^s steps, and their sum must fit in 63 bits: s = 61 - ceil(log2 taps), at least 40 (what every
    call took before, and what the root grid at batch 4 and anything larger still takes: the same bits there) and at most 49
    (include/sp3d.h: the merge kernel's rounding needs every contribution below 2^50 steps).  Small calls get a finer step: a channel whose
    gradient is 2^-17 of the call's largest then still lands within the fp32 scatter's error bound."""
    s = max(40, min(49, 61 - max(int(taps) - 1, 1).bit_length()))
    k = torch.ceil(torch.log2(gmax.clamp_min(1e-30)))
    return torch.exp2((float(s) - k).clamp_max(126.0)).to(torch.float32).reshape(1)


def unproject_bwd_packed(cam, centers, valid, grad_cubes: torch.Tensor, pass_mask: torch.Tensor, batch: int,
                         num_views: int, J: int, jp: int, h: int, w: int, cube_size, grid_size, img_size,
                         sample_of: Optional[torch.Tensor] = None, deterministic: bool = False, return_packed: bool = False,
                         scatter: int = SCATTER_AUTO, wide: bool = False, out_dtype: torch.dtype = torch.float32):
    """line-coalesced scatter: -> list[V] of (B,J,h,w) gradient views into one (V,B,h,w,jp) channels-last buffer
    (``return_packed``: that buffer itself, pad channels zero).
    ``out_dtype`` = torch.bfloat16: the fp32 buffer (the atomics' sums, or the converted fixed-point sums) is rounded ONCE as a
    whole, by one dense pass, and the views returned are views of that bf16 buffer.
    ``deterministic``: accumulate in 64-bit fixed point (integer atomics): bit-identical run to run.
    ``scatter``: SCATTER_AUTO (by voxel pitch) / SCATTER_PER_TAP / SCATTER_MERGE - a per-call choice (include/sp3d.h).
    ``wide`` (SP3D_SCATTER_WIDE): 17..32 joints; ``jp`` must be 32, ``pass_mask`` the (2, P, X*Y*Z) mask of
    ``unproject_fwd(wide_mask=True)``; the buffer is (V,B,h,w,32)."""
    lib = load()
    dev = cam.device
    _require_cam(cam)
    P = int(grad_cubes.shape[0])
    X, Y, Z = (int(c) for c in cube_size)
    if wide:
        if pass_mask.numel() != 2 * P * X * Y * Z:
            raise Sp3dError("unproject_bwd_packed(wide=True): pass_mask must hold (2, P, X*Y*Z) words")
        scatter = int(scatter) | SCATTER_WIDE
    gc = grad_cubes[:, :J].float().contiguous()
    if deterministic:
        scale = _fixed_point_scale(gc.abs().amax(), 4 * P * X * Y * Z)
        fixed = torch.zeros((num_views, batch, h, w, jp), dtype=torch.int64, device=dev)
        rc = lib.sp3d_unproject_bwd_packed_det(cam.data_ptr(), _opt(sample_of), centers.data_ptr(), valid.data_ptr(),
                                               gc.data_ptr(), pass_mask.data_ptr(), fixed.data_ptr(), scale.data_ptr(),
                                               int(batch), P, num_views, J, jp, h, w, X, Y, Z, _f3(grid_size),
                                               int(img_size[0]), int(img_size[1]), int(scatter), _stream(dev))
        check(rc, "sp3d_unproject_bwd_packed_det")
        packed = torch.empty((num_views, batch, h, w, jp), dtype=torch.float32, device=dev)
        check(lib.sp3d_fixed_to_float(fixed.data_ptr(), packed.data_ptr(), scale.data_ptr(), fixed.numel(), _stream(dev)),
              "sp3d_fixed_to_float")
    else:
        packed = torch.zeros((num_views, batch, h, w, jp), dtype=torch.float32, device=dev)
        rc = lib.sp3d_unproject_bwd_packed(cam.data_ptr(), _opt(sample_of), centers.data_ptr(), valid.data_ptr(),
                                           gc.data_ptr(), pass_mask.data_ptr(), packed.data_ptr(), int(batch), P, num_views,
                                           J, jp, h, w, X, Y, Z, _f3(grid_size), int(img_size[0]), int(img_size[1]),
                                           int(scatter), _stream(dev))
        check(rc, "sp3d_unproject_bwd_packed")
    if out_dtype != torch.float32:
        packed = packed.to(out_dtype)
    return packed if return_packed else [packed[c].permute(0, 3, 1, 2)[:, :J] for c in range(num_views)]


def unproject_one_fwd_train(views: Sequence[torch.Tensor], layout: int, jp: int, cam: torch.Tensor, centers: torch.Tensor,
                            valid: torch.Tensor, B: int, J: int, h: int, w: int, cube_size, grid_size, img_size,
                            pass_mask: torch.Tensor, want_grids: bool = True, channels_last: bool = False,
                            sample_of: Optional[torch.Tensor] = None):
    """one-channel training forward (sp3d_unproject_one_fwd_train): ``views``, ``layout`` and ``jp`` as ``unproject_fwd`` takes
    them with ``one_channel=True``; ``J`` = channels written, 1 or 4 (channels-last: 4).  Also fills ``pass_mask`` ((B, X*Y*Z)
    int16, bit 0) for ``unproject_one_bwd``.  bf16 views (all of them: SP3D_HM_BF16_TRAIN, derived from the dtype) are read in
    place with 2-byte taps, ``jp`` counting bf16 elements; the results stay fp32.  -> (cubes, grids | None)"""
    lib = load()
    dev = cam.device
    _require_cam(cam)
    X, Y, Z = (int(c) for c in cube_size)
    if views[0].dtype not in (torch.float32, torch.bfloat16) or not all(v.dtype == views[0].dtype and v.is_cuda for v in views):
        raise Sp3dError("unproject_one_fwd_train: fp32 heat-map views or bf16 heat-map views (not a mixture) on the GPU expected")
    if pass_mask.dtype != torch.int16 or not pass_mask.is_contiguous() or pass_mask.numel() != B * X * Y * Z:
        raise Sp3dError("unproject_one_fwd_train: pass_mask must be a contiguous int16 (B, X*Y*Z) tensor")
    cubes = _empty_cl3d(B, J, X, Y, Z, dev) if channels_last else torch.empty((B, J, X, Y, Z), dtype=torch.float32, device=dev)
    grids = torch.empty((B, X * Y * Z, 3), dtype=torch.float32, device=dev) if want_grids else None
    flags = HM_ONE_CHANNEL | (OUT_CHANNELS_LAST if channels_last else 0) | (HM_BF16_TRAIN if views[0].dtype == torch.bfloat16 else 0)
    rc = lib.sp3d_unproject_one_fwd_train(_ptr_array(views), layout | flags, jp, cam.data_ptr(), _opt(sample_of),
                                          centers.data_ptr(), valid.data_ptr(), cubes.data_ptr(), _opt(grids),
                                          pass_mask.data_ptr(), B, len(views), J, h, w, X, Y, Z, _f3(grid_size),
                                          int(img_size[0]), int(img_size[1]), _stream(dev))
    check(rc, "sp3d_unproject_one_fwd_train")
    return cubes, grids


def unproject_one_bwd(cam, centers, valid, grad_cubes: torch.Tensor, pass_mask: torch.Tensor, batch: int, num_views: int,
                      h: int, w: int, cube_size, grid_size, img_size, sample_of: Optional[torch.Tensor] = None,
                      deterministic: bool = False):
    """one-channel scatter: channel 0 of ``grad_cubes`` (P,C,X,Y,Z) -> list[V] of (B,1,h,w) gradient views of one dense
    (V,B,h,w) buffer.  A contiguous planar fp32 gradient is read in place at its cube stride (C*N: no slice copy); anything
    else (channels-last, another dtype, a view) is reduced to channel 0 first.
    ``deterministic``: 64-bit fixed point with integer atomics, scale = ``_fixed_point_scale`` of that channel's max|g|, as
    ``unproject_bwd_packed`` builds it: bit-identical run to run, and to channel 0 of the packed deterministic scatter."""
    out = _unproject_one_bwd_dense(cam, centers, valid, grad_cubes, pass_mask, batch, num_views, h, w, cube_size, grid_size, img_size,
                                   sample_of, deterministic)
    return [out[c].unsqueeze(1) for c in range(num_views)]


def unproject_one_bwd_rounded(cam, centers, valid, grad_cubes: torch.Tensor, pass_mask: torch.Tensor, batch: int, num_views: int,
                              h: int, w: int, cube_size, grid_size, img_size, sample_of: Optional[torch.Tensor] = None,
                              deterministic: bool = False, out_dtype: torch.dtype = torch.bfloat16):
    """``unproject_one_bwd`` with a gradient of ``out_dtype``: the dense fp32 (V,B,h,w) buffer (the atomics' sums, or the
    converted fixed-point sums) is rounded ONCE as a whole, by one dense pass, and the (B,1,h,w) views returned are views of the
    rounded buffer - what a bf16 heat-map wants, with nothing left for the autograd engine to cast.  (A function of its own:
    the parameter list of ``unproject_one_bwd`` is pinned.)"""
    out = _unproject_one_bwd_dense(cam, centers, valid, grad_cubes, pass_mask, batch, num_views, h, w, cube_size, grid_size, img_size,
                                   sample_of, deterministic)
    if out_dtype != torch.float32:
        out = out.to(out_dtype)
    return [out[c].unsqueeze(1) for c in range(num_views)]


def _unproject_one_bwd_dense(cam, centers, valid, grad_cubes, pass_mask, batch, num_views, h, w, cube_size, grid_size, img_size,
                             sample_of, deterministic) -> torch.Tensor:
    """the scatter of ``unproject_one_bwd`` -> its dense fp32 (V,B,h,w) buffer"""
    lib = load()
    dev = cam.device
    _require_cam(cam)
    P = int(grad_cubes.shape[0])
    X, Y, Z = (int(c) for c in cube_size)
    N = X * Y * Z
    if grad_cubes.dtype == torch.float32 and grad_cubes.is_contiguous():
        gc, stride = grad_cubes, int(grad_cubes.shape[1]) * N
    else:
        gc, stride = grad_cubes[:, :1].float().contiguous(), N
    if deterministic:
        scale = _fixed_point_scale(gc[:, 0].abs().amax(), 4 * P * N)
        fixed = torch.zeros((num_views, batch, h, w), dtype=torch.int64, device=dev)
        rc = lib.sp3d_unproject_one_bwd_det(cam.data_ptr(), _opt(sample_of), centers.data_ptr(), valid.data_ptr(), gc.data_ptr(),
                                            stride, pass_mask.data_ptr(), fixed.data_ptr(), scale.data_ptr(), int(batch), P,
                                            num_views, h, w, X, Y, Z, _f3(grid_size), int(img_size[0]), int(img_size[1]),
                                            _stream(dev))
        check(rc, "sp3d_unproject_one_bwd_det")
        out = torch.empty((num_views, batch, h, w), dtype=torch.float32, device=dev)
        check(lib.sp3d_fixed_to_float(fixed.data_ptr(), out.data_ptr(), scale.data_ptr(), fixed.numel(), _stream(dev)),
              "sp3d_fixed_to_float")
    else:
        out = torch.zeros((num_views, batch, h, w), dtype=torch.float32, device=dev)
        rc = lib.sp3d_unproject_one_bwd(cam.data_ptr(), _opt(sample_of), centers.data_ptr(), valid.data_ptr(), gc.data_ptr(),
                                        stride, pass_mask.data_ptr(), out.data_ptr(), int(batch), P, num_views, h, w, X, Y, Z,
                                        _f3(grid_size), int(img_size[0]), int(img_size[1]), _stream(dev))
        check(rc, "sp3d_unproject_one_bwd")
    return out


def gaussian_target_3d(roots: torch.Tensor, gx: torch.Tensor, gy: torch.Tensor, gz: torch.Tensor, sigma: float):
    """roots (B,R,3), per-axis voxel centres -> (B,X,Y,Z) max-of-Gaussians target"""
    lib = load()
    _require_cuda(roots, "roots")
    B, R = roots.shape[:2]
    X, Y, Z = gx.numel(), gy.numel(), gz.numel()
    r = roots.contiguous().float()
    out = torch.empty((B, X, Y, Z), dtype=torch.float32, device=roots.device)
    check(lib.sp3d_gaussian_target_3d(r.data_ptr(), B, R, gx.data_ptr(), gy.data_ptr(), gz.data_ptr(), X, Y, Z, float(sigma),
                                      out.data_ptr(), _stream(roots.device)), "sp3d_gaussian_target_3d")
    return out


def render_root_heatmaps(roots: torch.Tensor, cam: torch.Tensor, h: int, w: int, stride: float):
    """roots (B,R,3), cam (B,V,64) -> (V,B,1,h,w) clipped sum of sigma-3 Gaussians at the projected roots"""
    lib = load()
    _require_cuda(roots, "roots")
    _require_cam(cam)
    B, R = roots.shape[:2]
    V = cam.shape[1]
    r = roots.contiguous().float()
    out = torch.empty((V, B, 1, h, w), dtype=torch.float32, device=roots.device)
    check(lib.sp3d_render_root_heatmaps(r.data_ptr(), B, R, cam.data_ptr(), V, h, w, float(stride), out.data_ptr(),
                                        _stream(roots.device)), "sp3d_render_root_heatmaps")
    return out


def freq_contract(Xf: torch.Tensor, Wf: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Xf (B,C,*F) complex64, Wf (O,C,*F) complex64 (contiguous) -> Yf (B,O,*F) = sum_c Xf * Wf"""
    lib = load()
    _require_cuda(Xf, "Xf")
    if Xf.dtype != torch.complex64 or Wf.dtype != torch.complex64 or Xf.shape[2:] != Wf.shape[2:] or Xf.shape[1] != Wf.shape[1]:
        raise Sp3dError("freq_contract: complex64 (B,C,*F) x (O,C,*F) expected")
    Xf, Wf = Xf.resolve_conj().contiguous(), Wf.resolve_conj().contiguous()      # data_ptr() ignores a lazy conj bit
    B, Cc = int(Xf.shape[0]), int(Xf.shape[1])
    O = int(Wf.shape[0])
    Fn = 1
    for d in Xf.shape[2:]:
        Fn *= int(d)
    Yf = _result_dense(out, (B, O) + tuple(Xf.shape[2:]), torch.complex64, Xf.device, "freq_contract")
    check(lib.sp3d_freq_contract(Xf.data_ptr(), Wf.data_ptr(), Yf.data_ptr(), B, Cc, O, Fn, _stream(Xf.device)),
          "sp3d_freq_contract")
    return Yf


def freq_contract_ty(Xf: torch.Tensor, T: torch.Tensor, tw: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Xf (B,C,KZ,SX,SY) complex64, T (KZ*SX, O, C, 14) fp32 (v2v_net._FoldedV2V._weights_ty), tw (SY,3,2) fp32
    -> (B,O,KZ,SX,SY) complex64: the forward contraction with W^ rebuilt per bin along y (include/sp3d.h)"""
    lib = load()
    _require_cuda(Xf, "Xf")
    B, Cc, KZ, SX, SY = (int(v) for v in Xf.shape)
    rows, O = int(T.shape[0]), int(T.shape[1])
    if Xf.dtype != torch.complex64 or not Xf.is_contiguous() or T.dtype != torch.float32 or not T.is_contiguous() or \
            tuple(T.shape) != (KZ * SX, O, Cc, 14) or tuple(tw.shape) != (SY, 3, 2) or not tw.is_contiguous():
        raise Sp3dError("freq_contract_ty: (B,C,KZ,SX,SY) complex64 x (KZ*SX,O,C,14) fp32 table expected")
    Yf = _result_dense(out, (B, O, KZ, SX, SY), torch.complex64, Xf.device, "freq_contract_ty")
    check(lib.sp3d_freq_contract_ty(Xf.data_ptr(), T.data_ptr(), tw.data_ptr(), Yf.data_ptr(), B, Cc, O, rows, SY,
                                    _stream(Xf.device)), "sp3d_freq_contract_ty")
    return Yf


def freq_contract_ex(Pf: torch.Tensor, Qf: torch.Tensor, mode: str, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the three products of the frequency-domain conv on contiguous complex64 (A,B,*F) operands:
    'fwd'  Pf = X (B,C,*F), Qf = W^ (O,C,*F)  -> (B,O,*F) = sum_c X conj(W^)
    'dx'   Pf = Gy (B,O,*F), Qf = W^ (O,C,*F) -> (B,C,*F) = sum_o Gy W^
    'dw'   Pf = Gy (B,O,*F), Qf = X (B,C,*F)  -> (O,C,*F) = sum_b conj(Gy) X"""
    lib = load()
    _require_cuda(Pf, "Pf")
    Pf, Qf = Pf.resolve_conj().contiguous(), Qf.resolve_conj().contiguous()
    if Pf.dtype != torch.complex64 or Qf.dtype != torch.complex64 or Pf.shape[2:] != Qf.shape[2:]:
        raise Sp3dError("freq_contract_ex: complex64 operands with equal frequency shape expected")
    Fn = 1
    for d in Pf.shape[2:]:
        Fn *= int(d)
    p0, p1, q0, q1 = int(Pf.shape[0]), int(Pf.shape[1]), int(Qf.shape[0]), int(Qf.shape[1])
    if mode == "fwd":       # i=b, k=c, j=o
        I, K, J = p0, p1, q0
        sPi, sPk, sQj, sQk, cp, cq = p1 * Fn, Fn, q1 * Fn, Fn, 0, 1
        ok = q1 == p1
    elif mode == "dx":      # i=b, k=o, j=c
        I, K, J = p0, p1, q1
        sPi, sPk, sQj, sQk, cp, cq = p1 * Fn, Fn, Fn, q1 * Fn, 0, 0
        ok = q0 == p1
    elif mode == "dw":      # i=o, k=b, j=c
        I, K, J = p1, p0, q1
        sPi, sPk, sQj, sQk, cp, cq = Fn, p1 * Fn, Fn, q1 * Fn, 1, 0
        ok = q0 == p0
    else:
        raise Sp3dError(f"freq_contract_ex: unknown mode {mode}")
    if not ok:
        raise Sp3dError("freq_contract_ex: contracted dimensions differ")
    Y = _result_dense(out, (I, J) + tuple(Pf.shape[2:]), torch.complex64, Pf.device, "freq_contract_ex")
    check(lib.sp3d_freq_contract_ex(Pf.data_ptr(), Qf.data_ptr(), Y.data_ptr(), I, J, K, Fn, sPi, sPk, sQj, sQk, cp, cq,
                                    _stream(Pf.device)), "sp3d_freq_contract_ex")
    return Y


_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def wino_weights(w: torch.Tensor) -> torch.Tensor:
    """(O,C,3,3,3) conv weights -> U (64, C, O) = G g G^T along each axis (Winograd F(2,3))"""
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    u = torch.einsum("ai,bj,ck,ozijk->abczo", G, G, G, w.double())
    return u.reshape(64, w.shape[1], w.shape[0]).float().contiguous()


def wino_weights_split(U: torch.Tensor, chunk: int = 8) -> torch.Tensor:
    """U (64,C,O) fp32 -> the bf16 three-piece records the split kernels read: (64, C/chunk, chunk/4, O, 3, 4) bfloat16
    with pieces ordered (mid, hi, lo) and channel = chunk*c + 4*group + q; hi + mid + lo == U exactly (24 mantissa bits).
    chunk = 8: sp3d_wino_fused_split (lane halves), chunk = 16: sp3d_wino_fused_split64 (lane quarters)"""
    P, Cc, O = (int(v) for v in U.shape)
    U = U.float()
    hi = U.bfloat16()
    r = U - hi.float()
    mid = r.bfloat16()
    lo = (r - mid.float()).bfloat16()
    pieces = torch.stack([mid, hi, lo], 0).reshape(3, P, Cc // chunk, chunk // 4, 4, O)   # [piece, p, chunk, group, q, o]
    return pieces.permute(1, 2, 3, 5, 0, 4).contiguous()                                  # [p, chunk, group, o, piece, q]


def wino_yz_weights(w: torch.Tensor) -> torch.Tensor:
    """(O,C,3,3,3) conv weights -> (48, C, O): G g G^T along y and z only, raw along x; point = dx*16 + j*4 + k.  Computed in
    float64 and rounded to fp32 once, as wino_weights does"""
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    u = torch.einsum("bj,ck,ozijk->ibczo", G, G, w.double())
    return u.reshape(48, w.shape[1], w.shape[0]).float().contiguous()


def wino_yz_weights_split(w: torch.Tensor) -> torch.Tensor:
    """(64,C,3,3,3) conv weights, C = 32 | 64 -> what sp3d_wino_fused_split64 reads under CONV3_WINO_YZ: the 24-byte records
    of wino_weights_split(., 16), (48, C/16, 4, 64, 3, 4) bfloat16, for the 48 points of wino_yz_weights"""
    return wino_weights_split(wino_yz_weights(w), 16)


def wino_yz_enabled() -> bool:
    """SP3D_WINO_YZ=0 keeps the half-resolution layers on the 64-point form of wino_fused16_kernel (x transformed too)"""
    return env_switch("SP3D_WINO_YZ", True)


def conv_weights_split(w: torch.Tensor) -> torch.Tensor:
    """(O,C,3,3,3) conv weights -> the bf16 operand records sp3d_conv3_split reads: (27, C/8, 2, O, 6, 4) bfloat16 = the
    three B operands {hi,lo} {hi,hi} {mid,mid} of 4 channels each, tap = kz*9 + ky*3 + kx, channel = 8*chunk + 4*half + q.
    A (O,C,1,1,1) weight gives the one-tap records (1, C/8, 2, O, 6, 4) of a folded skip projection."""
    O, Cc = int(w.shape[0]), int(w.shape[1])
    taps = int(w.shape[2]) * int(w.shape[3]) * int(w.shape[4])      # 27, or 1: the 1x1x1 skip projection (sp3d_conv3_split_skip)
    pc = wino_weights_split(w.float().permute(4, 3, 2, 1, 0).reshape(taps, Cc, O).contiguous(), 8)  # [.., piece (mid,hi,lo), 4]
    mid, hi, lo = pc[..., 0, :], pc[..., 1, :], pc[..., 2, :]
    return torch.stack([hi, lo, hi, hi, mid, mid], -2).contiguous()        # the B operands {bh,bl} {bh,bh} {bm,bm}


def conv_weights_split24(w: torch.Tensor) -> torch.Tensor:
    """(O,C,3,3,3) conv weights, O % 32 == 0 -> what sp3d_conv3_split reads for O = 128: (27, C/8, O/32, 768) bfloat16, per (tap, chunk,
    32 outputs) one block of 1 536 contiguous bytes = [half 2][output 32] x {hi,lo} of 4 channels (16 bytes) followed by
    [half 2][output 32] x {mid} of 4 channels (8 bytes); tap = kz*9 + ky*3 + kx, channel = 8*chunk + 4*half + q.  The three
    pieces once each (24 bytes per output and 4 channels): the kernel assembles {hi,hi} and {mid,mid} in registers."""
    O, Cc = int(w.shape[0]), int(w.shape[1])
    pc = wino_weights_split(w.float().permute(4, 3, 2, 1, 0).reshape(27, Cc, O).contiguous(), 8)   # [tap, chunk, half, o, piece (mid,hi,lo), 4]
    pc = pc.reshape(27, Cc // 8, 2, O // 32, 32, 3, 4).permute(0, 1, 3, 2, 4, 5, 6)                # [tap, chunk, og, half, t, piece, 4]
    hl = torch.stack([pc[..., 1, :], pc[..., 2, :]], -2).reshape(27, Cc // 8, O // 32, 512)
    mid = pc[..., 0, :].reshape(27, Cc // 8, O // 32, 256)
    return torch.cat([hl, mid], -1).contiguous()


def skip_fold_enabled() -> bool:
    """SP3D_FOLD_SKIP=0 keeps the 1x1x1 skip projections of the plan's residual blocks a library GEMM + residual epilogue"""
    return env_switch("SP3D_FOLD_SKIP", True)


def _require_skip(xs: torch.Tensor, skip_w: torch.Tensor, x: torch.Tensor, CS: int, numel: int, who: str):
    """the folded skip's operands: xs the block input (B,CS,X,Y,Z) channels_last_3d on x's grid, skip_w exactly the records
    the kernel reads behind the pointer"""
    _require_cl3d_f32(xs, who)
    if xs.device != x.device or tuple(xs.shape) != (x.shape[0], CS) + tuple(x.shape[2:]):
        raise Sp3dError(f"{who}: xs must be ({x.shape[0]}, {CS}, ...) on the grid and device of x, got {tuple(xs.shape)} on {xs.device}")
    if skip_w.device != x.device or skip_w.dtype != torch.bfloat16 or not skip_w.is_contiguous() or skip_w.numel() != numel:
        raise Sp3dError(f"{who}: skip_w must be the split records of the ({x.shape[1]}, {CS}, 1, 1, 1) weight on {x.device}; got "
                        f"{tuple(skip_w.shape)}, {skip_w.dtype}, {skip_w.device}, contiguous={skip_w.is_contiguous()}")


POOL_FOLD_DEFAULT = True


def pool_fold_enabled() -> bool:
    """SP3D_FOLD_POOL=0 keeps the plan's two MaxPool3d(2,2) launches of their own; on, the second conv of front_res and of
    encoder_res1 writes the pooled tensor from its accumulators where pool_fold_covers"""
    return env_switch("SP3D_FOLD_POOL", POOL_FOLD_DEFAULT)


def pool_fold_covers(route: str, X: int, Y: int, Z: int) -> bool:
    """the grids on which the kernel behind ``route`` (a name v2v_net.conv3_route gives) has a pooled form: whole output
    blocks only, 16x8x4 for conv3_split_ (80x80x20, 64^3, 48x48x12; not 40x40x10), 8x8x2 for wino_fused_conv3d_ (40x40x10,
    32^3; not 20x20x5) - what the C entries refuse otherwise"""
    X, Y, Z = int(X), int(Y), int(Z)
    if min(X, Y, Z) <= 0:
        return False
    if route == "conv3_split_":
        return X % 16 == 0 and Y % 8 == 0 and Z % 4 == 0
    if route == "wino_fused_conv3d_":
        return X % 8 == 0 and Y % 8 == 0 and Z % 2 == 0
    return False


def _result_pooled(out: Optional[torch.Tensor], B: int, O: int, X: int, Y: int, Z: int, x: torch.Tensor, who: str):
    """(y, y_pooled) of a pool=True call: channels_last_3d views (B,O,X,Y,Z) and (B,O,X/2,Y/2,Z/2) of ONE float32 buffer of
    B*X*Y*Z*O + B*(X/2)*(Y/2)*(Z/2)*O elements, the pooled tensor directly behind the full one (include/sp3d.h:
    SP3D_CONV3_POOL2X) - a fresh buffer, or the caller's dense 1-D ``out`` of exactly that size on x's device"""
    n, npool = B * X * Y * Z * O, B * (X // 2) * (Y // 2) * (Z // 2) * O
    if out is None:
        out = torch.empty(n + npool, dtype=torch.float32, device=x.device)
    elif out.dim() != 1 or out.numel() != n + npool or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise Sp3dError(f"{who}: with pool=True out must be a dense 1-D float32 buffer of {n} + {npool} elements on {x.device}, got "
                        f"{tuple(out.shape)}, {out.dtype}, {out.device}")
    return (out[:n].view(B, X, Y, Z, O).permute(0, 4, 1, 2, 3), out[n:].view(B, X // 2, Y // 2, Z // 2, O).permute(0, 4, 1, 2, 3))


def conv3_split_(x: torch.Tensor, W3: torch.Tensor, shift: torch.Tensor, mode: int,
                 residual: Optional[torch.Tensor] = None, *, xs: Optional[torch.Tensor] = None,
                 skip_w: Optional[torch.Tensor] = None, pool: bool = False, out: Optional[torch.Tensor] = None):
    """3x3x3 stride-1 'same' conv of channels_last_3d x with the fused epilogue, direct (implicit GEMM) on the bf16 matrix
    pipe with exact three-piece splits; W3 = conv_weights_split(w).  Returns the channels_last_3d result (B,O,X,Y,Z), written
    into ``out`` when given.
    (Round 3's chained form - split activations handed from layer to layer - measured no gain and was removed in round 4.)
    With xs (B,16,X,Y,Z) and skip_w = conv_weights_split of the (32,16,1,1,1) skip weight: relu(conv3(x) + skip_w . xs + shift)
    in the same kernel (sp3d_conv3_split_skip; mode must be 1 and residual None - the projection is the residual).
    pool=True (with the folded skip only, grids of whole 16x8x4 blocks: pool_fold_covers): returns (y, y_pooled), the result and
    its MaxPool3d(2,2) - bit for bit maxpool2x(y) - as channels_last_3d views of one buffer (``out``: that buffer, 1-D)."""
    lib = load()
    _require_cuda(x, "x")
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    _require_cl3d_f32(x, "conv3_split_")
    O = int(W3.shape[3])
    dev = x.device
    if pool:
        if xs is None or skip_w is None:
            raise Sp3dError("conv3_split_: pool=True is a form of the folded skip (xs and skip_w)")
        y, yp = _result_pooled(out, B, O, X, Y, Z, x, "conv3_split_")
    else:
        y = _result_cl3d(out, B, O, X, Y, Z, x, "conv3_split_")
    if xs is not None or skip_w is not None:
        if xs is None or skip_w is None or int(mode) != 1 or residual is not None:
            raise Sp3dError("conv3_split_: the folded skip takes xs AND skip_w, mode 1 and no residual")
        CS = 16
        _require_skip(xs, skip_w, x, CS, CS * O * 6, "conv3_split_")
        check(lib.sp3d_conv3_split_skip(x.data_ptr(), W3.data_ptr(), y.data_ptr(), shift.data_ptr(), xs.data_ptr(),
                                        skip_w.data_ptr(), B, X, Y, Z, Cc, O, CS | (CONV3_POOL2X if pool else 0), _stream(dev)),
              "sp3d_conv3_split_skip")
        return (y, yp) if pool else y
    if residual is not None:
        residual = _as_cl3d(residual)
    check(lib.sp3d_conv3_split(x.data_ptr(), W3.data_ptr(), y.data_ptr(), shift.data_ptr(), _opt(residual), int(mode),
                               B, X, Y, Z, Cc, O, _stream(dev)), "sp3d_conv3_split")
    return y


def quarter_direct_enabled() -> bool:
    """SP3D_QUARTER_DIRECT=0 keeps the quarter-resolution 3x3x3 layers on the three-launch Winograd form"""
    return env_switch("SP3D_QUARTER_DIRECT", True)


def quarter_direct_covers(B: int, C: int, O: int, X: int, Y: int, Z: int) -> bool:
    """the layers v2v_net.conv3_route gives to the direct kernel (conv3_split128_): the widths the
    kernel is built for, on grids its 5x5x5 output blocks tile without remainder, up to 64 blocks = 256 workgroups, one per
    CU of an MI355X: 20x20x5 at batch 1..4 (the headline root net; 42.3 against 56.9 us per layer at batch 4, 29.2 against
    36.6 at batch 1).  Measured and left to the three launches (profiles/r15_quarter_direct_shapes.json): 40x40x10 at batch
    2 (four rounds of workgroups: 150.0 against 147.0 us) and the ragged grids, where the kernel is correct but multiplies
    rows that are no outputs - 12x12x3 (38 % outputs: 27.9 against 22.2 us at batch 1, 31.4 against 31.9 at batch 4) and
    16^3 (51 %: 269 against 158 us for 8 cubes)."""
    blocks = B * (X // 5) * (Y // 5) * (Z // 5)
    return O == 128 and C in (64, 128) and X % 5 == 0 and Y % 5 == 0 and Z % 5 == 0 and blocks <= 64


def conv3_split128_(x: torch.Tensor, W3: torch.Tensor, shift: torch.Tensor, mode: int,
                    residual: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3x3 stride-1 'same' conv of channels_last_3d x, (C, O) = (64 | 128, 128), with the fused epilogue: the direct
    (implicit GEMM) kernel of the quarter-resolution layers on the bf16 matrix pipe with exact three-piece splits
    (sp3d_conv3_split with O = 128); W3 = conv_weights_split24(w).  Any grid: output blocks of 5x5x5 voxels, ragged edges included.
    Returns the channels_last_3d result (B,O,X,Y,Z), written into ``out`` when given."""
    lib = load()
    _require_cuda(x, "x")
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    _require_cl3d_f32(x, "conv3_split128_")
    O = 128
    if W3.device != x.device or W3.dtype != torch.bfloat16 or not W3.is_contiguous() or tuple(W3.shape) != (27, Cc // 8, O // 32, 768):
        raise Sp3dError(f"conv3_split128_: W3 must be conv_weights_split24 of the ({O}, {Cc}, 3, 3, 3) weight on {x.device}; got "
                        f"{tuple(W3.shape)}, {W3.dtype}, {W3.device}, contiguous={W3.is_contiguous()}")
    out = _result_cl3d(out, B, O, X, Y, Z, x, "conv3_split128_")
    if residual is not None:
        residual = _as_cl3d(residual)
    check(lib.sp3d_conv3_split(x.data_ptr(), W3.data_ptr(), out.data_ptr(), shift.data_ptr(), _opt(residual), int(mode),
                                  B, X, Y, Z, Cc, O, _stream(x.device)), "sp3d_conv3_split")
    return out


def wino_conv3d_(x: torch.Tensor, U: torch.Tensor, shift: torch.Tensor, mode: int,
                 residual: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3x3x3 stride-1 'same' conv of channels-last x (B,C,X,Y,Z as torch.channels_last_3d) fused with the layer epilogue:
    Winograd F(2,3) with pre-transformed weights U (64,C,O) in three launches - input transform, the library's batched fp32
    GEMM, output transform + epilogue.  Returns a channels_last_3d tensor (B,O,X,Y,Z), written into ``out`` when given."""
    lib = load()
    _require_cuda(x, "x")
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    _require_cl3d_f32(x, "wino_conv3d_")
    O = int(U.shape[2])
    if residual is not None:
        residual = _as_cl3d(residual)
    y = _result_cl3d(out, B, O, X, Y, Z, x, "wino_conv3d_")
    T = B * ((X + 1) // 2) * ((Y + 1) // 2) * ((Z + 1) // 2)
    V = torch.empty((64, T, Cc), dtype=torch.float32, device=x.device)
    check(lib.sp3d_wino_input(x.data_ptr(), V.data_ptr(), B, X, Y, Z, Cc, _stream(x.device)), "sp3d_wino_input")
    M = torch.bmm(V, U)         # the 64 products: the library's fp32 batched GEMM (an own split-bf16 GEMM was not faster: round 3)
    check(lib.sp3d_wino_output(M.data_ptr(), y.data_ptr(), shift.data_ptr(), _opt(residual), int(mode), B, X, Y, Z, O,
                               _stream(x.device)), "sp3d_wino_output")
    return y


def wino_fused_conv3d_(x: torch.Tensor, U: torch.Tensor, shift: torch.Tensor, mode: int,
                       residual: Optional[torch.Tensor] = None, U3: Optional[torch.Tensor] = None, *,
                       xs: Optional[torch.Tensor] = None, skip_w: Optional[torch.Tensor] = None,
                       U3yz: Optional[torch.Tensor] = None, pool: bool = False, out: Optional[torch.Tensor] = None):
    """one-launch Winograd 3x3x3 conv (C = 16 | 32 -> O = 32; with U3 also C = 32 | 64 -> O = 64) of channels_last_3d x
    with the fused epilogue; with U3 (wino_weights_split(U, 8 | 16)) the products run as exact three-piece bf16 splits
    on the bf16 matrix pipe.  With U3, xs (B,32,X,Y,Z) and skip_w = wino_weights_split of the (1,32,64) skip weight, chunk 16
    (C = O = 64): relu(conv3(x) + skip_w . xs + shift) in the same kernel (sp3d_wino_fused_split64_skip; mode 1, no residual).
    U3yz (wino_yz_weights_split(w); O = 64, next to U3): the same layer with Winograd in y and z only and the three x taps
    convolved directly - taken instead of U3 unless SP3D_WINO_YZ=0, which runs the U3 form bit for bit.
    The result is written into ``out`` when given.
    pool=True (with the folded skip only, grids of whole 8x8x2 blocks: pool_fold_covers): returns (y, y_pooled), the result and
    its MaxPool3d(2,2) - bit for bit maxpool2x(y) - as channels_last_3d views of one buffer (``out``: that buffer, 1-D)."""
    lib = load()
    _require_cuda(x, "x")
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    _require_cl3d_f32(x, "wino_fused_conv3d_")
    O = int(U.shape[2])
    if pool:
        if xs is None or skip_w is None:
            raise Sp3dError("wino_fused_conv3d_: pool=True is a form of the folded skip (U3, xs and skip_w)")
        y, yp = _result_pooled(out, B, O, X, Y, Z, x, "wino_fused_conv3d_")
    else:
        y = _result_cl3d(out, B, O, X, Y, Z, x, "wino_fused_conv3d_")
    yz = 0
    if U3yz is not None and U3 is not None and O == 64 and wino_yz_enabled():
        # the kernel reads 48 * C * 64 pieces of three bf16 behind this pointer: refuse anything that is not exactly that
        if U3yz.device != x.device or U3yz.dtype != torch.bfloat16 or not U3yz.is_contiguous() or U3yz.numel() != 48 * Cc * O * 3:
            raise Sp3dError(f"wino_fused_conv3d_: U3yz must be wino_yz_weights_split of the ({O}, {Cc}, 3, 3, 3) weight on {x.device}; "
                            f"got {tuple(U3yz.shape)}, {U3yz.dtype}, {U3yz.device}, contiguous={U3yz.is_contiguous()}")
        U3, yz = U3yz, CONV3_WINO_YZ
    if xs is not None or skip_w is not None:
        if xs is None or skip_w is None or U3 is None or int(mode) != 1 or residual is not None:
            raise Sp3dError("wino_fused_conv3d_: the folded skip takes U3, xs AND skip_w, mode 1 and no residual")
        CS = 32
        _require_skip(xs, skip_w, x, CS, CS * O * 3, "wino_fused_conv3d_")
        check(lib.sp3d_wino_fused_split64_skip(x.data_ptr(), U3.data_ptr(), y.data_ptr(), shift.data_ptr(), xs.data_ptr(),
                                               skip_w.data_ptr(), B, X, Y, Z, Cc, O, CS | yz | (CONV3_POOL2X if pool else 0),
                                               _stream(x.device)),
              "sp3d_wino_fused_split64_skip")
        return (y, yp) if pool else y
    if residual is not None:
        residual = _as_cl3d(residual)
    if U3 is None:
        name, weights = "sp3d_wino_fused", U
    else:
        name, weights = ("sp3d_wino_fused_split64" if O == 64 else "sp3d_wino_fused_split"), U3
    check(getattr(lib, name)(x.data_ptr(), weights.data_ptr(), y.data_ptr(), shift.data_ptr(), _opt(residual), int(mode) | yz,
                             B, X, Y, Z, Cc, O, _stream(x.device)), name)
    return y


def upconv_weights_split(w_gemm: torch.Tensor) -> torch.Tensor:
    """(Cin, 8*O) GEMM-form weights of a ConvTranspose3d(2, stride 2) [columns (i,j,k,o)] -> the bf16 operand records
    sp3d_upconv2x_fused reads: (8, O/32, Cin/8, 2, 32, 6, 4) bfloat16 = per (tap, 32 outputs) the three B operands {hi,lo}
    {hi,hi} {mid,mid} of 4 channels each, channel = 8*chunk + 4*half + q (the records of conv_weights_split)"""
    Cc, O = int(w_gemm.shape[0]), int(w_gemm.shape[1]) // 8
    U = w_gemm.float().reshape(Cc, 8 * O // 32, 32).permute(1, 0, 2).contiguous()      # [(tap, o/32), c, o%32]
    pc = wino_weights_split(U, 8)                                                       # [.., piece (mid,hi,lo), 4]
    mid, hi, lo = pc[..., 0, :], pc[..., 1, :], pc[..., 2, :]
    return torch.stack([hi, lo, hi, hi, mid, mid], -2).reshape(8, O // 32, Cc // 8, 2, 32, 6, 4).contiguous()


def _require_upconv_split(w_split: torch.Tensor, Cc: int, O: int, x: torch.Tensor):
    """the kernel reads Cc * 8 * O twelve-byte records behind this pointer: refuse anything that is not exactly that"""
    if w_split.device != x.device or w_split.dtype != torch.bfloat16 or not w_split.is_contiguous() or \
            w_split.numel() != Cc * 8 * O * 6:
        raise Sp3dError(f"w_split must be upconv_weights_split(w_gemm) of the ({Cc}, {8 * O}) weight on {x.device}; got "
                        f"{tuple(w_split.shape)}, {w_split.dtype}, {w_split.device}, contiguous={w_split.is_contiguous()}")


def upconv_fused_covers(Cc: int, O: int, head: bool) -> bool:
    """the shapes sp3d_upconv2x_fused has a kernel for; SP3D_FUSE_UPCONV=0 sends every shape down the GEMM + scatter path"""
    return env_switch("SP3D_FUSE_UPCONV", True) and (Cc, O, bool(head)) in ((64, 32, True), (128, 64, False))


def upsample2x_(x: torch.Tensor, w_gemm: torch.Tensor, shift: torch.Tensor, skip: torch.Tensor,
                w_split: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ConvTranspose3d(k=2,s=2) + shift + ReLU + skip on channels_last_3d activations.  With w_split
    (upconv_weights_split(w_gemm)) and a shape upconv_fused_covers: one kernel, sp3d_upconv2x_fused.  Otherwise: one rocBLAS
    GEMM on the (voxels, Cin) view with w_gemm (Cin, 8*O) [columns (i,j,k,o)] + sp3d_upsample2x_scatter.  The (B,O,2X,2Y,2Z)
    result is written into ``out`` when given."""
    lib = load()
    _require_cuda(x, "x")
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    _require_cl3d_f32(x, "upsample2x_")
    O = int(w_gemm.shape[1]) // 8
    out = _result_cl3d(out, B, O, 2 * X, 2 * Y, 2 * Z, x, "upsample2x_")
    skip = _as_cl3d(skip)
    if w_split is not None and upconv_fused_covers(Cc, O, False):
        _require_upconv_split(w_split, Cc, O, x)
        check(lib.sp3d_upconv2x_fused(x.data_ptr(), w_split.data_ptr(), shift.data_ptr(), skip.data_ptr(), None, None,
                                      out.data_ptr(), B, X, Y, Z, Cc, O, 0, _stream(x.device)), "sp3d_upconv2x_fused")
        return out
    G = torch.matmul(x.permute(0, 2, 3, 4, 1).reshape(-1, Cc), w_gemm)
    check(lib.sp3d_upsample2x_scatter(G.data_ptr(), out.data_ptr(), shift.data_ptr(), skip.data_ptr(), B, X, Y, Z, O,
                                      _stream(x.device)), "sp3d_upsample2x_scatter")
    return out


def upsample2x_head_(x: torch.Tensor, w_gemm: torch.Tensor, shift: torch.Tensor, skip: torch.Tensor, w_out: torch.Tensor,
                     b_out: torch.Tensor, w_split: Optional[torch.Tensor] = None, *,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """upsample2x_ fused with the 1x1x1 output conv that is its only consumer: returns (B,J,2X,2Y,2Z) as a permuted view
    of a (B,2X,2Y,2Z,J) tensor (for J = 1 that is also the dense NCDHW tensor).  With w_split (upconv_weights_split(w_gemm))
    and a shape upconv_fused_covers: one kernel, sp3d_upconv2x_fused.  The result is written into ``out`` when given."""
    lib = load()
    _require_cuda(x, "x")
    B, Cc, X, Y, Z = (int(v) for v in x.shape)
    _require_cl3d_f32(x, "upsample2x_head_")
    O = int(w_gemm.shape[1]) // 8
    J = int(w_out.shape[0])
    skip = _as_cl3d(skip)
    wo = w_out.reshape(J, O).contiguous().float()
    head = _result_cl3d(out, B, J, 2 * X, 2 * Y, 2 * Z, x, "upsample2x_head_")
    if w_split is not None and J <= 32 and upconv_fused_covers(Cc, O, True):
        _require_upconv_split(w_split, Cc, O, x)
        bo = None if b_out is None else b_out.contiguous().float()
        check(lib.sp3d_upconv2x_fused(x.data_ptr(), w_split.data_ptr(), shift.data_ptr(), skip.data_ptr(), wo.data_ptr(),
                                      _opt(bo), head.data_ptr(), B, X, Y, Z, Cc, O, J, _stream(x.device)), "sp3d_upconv2x_fused")
        return head
    G = torch.matmul(x.permute(0, 2, 3, 4, 1).reshape(-1, Cc), w_gemm)
    bo = (b_out if b_out is not None else torch.zeros(J, device=x.device)).contiguous().float()
    check(lib.sp3d_upsample2x_scatter_head(G.data_ptr(), head.data_ptr(), shift.data_ptr(), skip.data_ptr(), wo.data_ptr(),
                                           bo.data_ptr(), B, X, Y, Z, O, J, _stream(x.device)), "sp3d_upsample2x_scatter_head")
    return head


class _RenderJoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kps, count, h, w, sigma):
        lib = load()
        _require_cuda(kps, "kps")
        N, Pn, J = (int(v) for v in kps.shape[:3])
        k = kps.contiguous().float()
        cnt = None if count is None else count.to(device=kps.device, dtype=torch.int32).contiguous()
        out = torch.empty((N, J, h, w), dtype=torch.float32, device=kps.device)
        check(lib.sp3d_render_joints_fwd(k.data_ptr(), _opt(cnt), N, Pn, J, h, w, float(sigma), out.data_ptr(),
                                         _stream(kps.device)), "sp3d_render_joints_fwd")
        ctx.save_for_backward(k, cnt if cnt is not None else torch.empty(0, device=kps.device))
        ctx.geom = (h, w, float(sigma), cnt is not None, kps.dtype)
        return out if kps.dtype == torch.float32 else out.to(kps.dtype)      # float64 callers: fp32 kernel, caller's type

    @staticmethod
    def backward(ctx, gout):
        lib = load()
        k, cnt = ctx.saved_tensors
        h, w, sigma, has_cnt, in_dtype = ctx.geom
        N, Pn, J = (int(v) for v in k.shape[:3])
        g = gout.contiguous().float()
        gk = torch.empty_like(k)
        check(lib.sp3d_render_joints_bwd(k.data_ptr(), cnt.data_ptr() if has_cnt else None, g.data_ptr(), N, Pn, J, h, w,
                                         sigma, gk.data_ptr(), _stream(k.device)), "sp3d_render_joints_bwd")
        return gk.to(in_dtype), None, None, None, None


def render_joint_heatmaps(kps: torch.Tensor, count: Optional[torch.Tensor], h: int, w: int, sigma: float = 3.0):
    """kps (N,P,J,2) heat-map pixels, count (N,) people per entry or None -> (N,J,h,w), differentiable in kps"""
    return _RenderJoints.apply(kps, count, int(h), int(w), float(sigma))
