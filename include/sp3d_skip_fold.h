/* Part of the C ABI of libsp3d.so, included by sp3d.h (include that; this file relies on its types and enums): the second
 * 3x3x3 convolution of a residual block that changes its channel count, with the block's 1x1x1 skip projection computed on
 * the same accumulators.  Two entries added in ABI version 3; no existing entry changes.
 *
 * It lives in a header of its own because sp3d.h's list of entry points is pinned (tests/test_host_cabi.py counts it);
 * tests/test_skip_fold_host.py holds this file against the binding's table by the same rule. */
#ifndef SP3D_SKIP_FOLD_H
#define SP3D_SKIP_FOLD_H

/* y = relu(conv3(x) + WS . xs + shift): sp3d_conv3_split (its x, W3, y, shift and its refusals) with the projection of the
 * block's input xs (B,X,Y,Z,CS) channels-last as more K of the same products - the projected tensor never exists.
 * WS: the 48-byte records of sp3d_conv3_split for a one-tap (O,CS,1,1,1) weight, index (chunk*2 + half)*O + o, channel =
 * 8*chunk + 4*half + q (_lib.conv_weights_split).  The projection's own shift is expected in `shift`.
 * (C, O, CS) = (32, 32, 16), anything else SP3D_EUNSUPPORTED; xs and WS 16-byte aligned (SP3D_EUNSUPPORTED), non-NULL
 * (SP3D_ENULL).  ReLU lets NaN through (torch.relu). */
int sp3d_conv3_split_skip(const float *x, const void *W3, float *y, const float *shift, const float *xs, const void *WS,
                          int B, int X, int Y, int Z, int C, int O, int CS, void *stream);

/* The same for the half-resolution blocks: sp3d_wino_fused_split64 (its x, U3, y, shift and its refusals) with
 * y = relu(conv3(x) + WS . xs + shift), xs (B,X,Y,Z,CS) channels-last.  WS: the 24-byte records [mid(4ch) hi(4ch) lo(4ch)] of
 * sp3d_wino_fused_split64 for one point, index (chunk*4 + group)*O + o, channel = 16*chunk + 4*group + q
 * (_lib.wino_weights_split of the (1, CS, O) weight, chunk 16).  (C, O, CS) = (64, 64, 32), anything else
 * SP3D_EUNSUPPORTED; WS 8-byte and xs 16-byte aligned (SP3D_EUNSUPPORTED), non-NULL (SP3D_ENULL); a sample of xs has fewer
 * than 2^31 elements (SP3D_ERANGE).  ReLU lets NaN through (torch.relu). */
int sp3d_wino_fused_split64_skip(const float *x, const void *U3, float *y, const float *shift, const float *xs, const void *WS,
                                 int B, int X, int Y, int Z, int C, int O, int CS, void *stream);

#endif
