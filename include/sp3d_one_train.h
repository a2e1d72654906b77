/* Part of the C ABI of libsp3d.so, included by sp3d.h (include that; this file relies on its types and enums): the training
 * pair of the one-channel unprojection (SP3D_HM_ONE_CHANNEL) - the root-joint map of the ROOTNET_ROOTHM root nets with a
 * heat-map gradient.  Three entries added in ABI version 3; no existing entry changes.
 *
 * They live in a header of their own because sp3d.h's list of entry points is pinned (tests/test_host_cabi.py counts it);
 * tests/test_one_channel_grad_host.py holds this file against the binding's table by the same rule. */
#ifndef SP3D_ONE_TRAIN_H
#define SP3D_ONE_TRAIN_H

/*
 * sp3d_unproject_fwd_indexed with SP3D_HM_ONE_CHANNEL that also writes the pass mask.  The addressing is the one-channel
 * forward's: hm_layout = SP3D_LAYOUT_PLANAR or SP3D_LAYOUT_NHWC, optionally | SP3D_OUT_CHANNELS_LAST; SP3D_HM_ONE_CHANNEL is
 * accepted and implied; Jp as documented at SP3D_HM_ONE_CHANNEL.  The result forms are the same: J = 1 planar, J = 4 planar
 * (channels 1-3 zero) or channels-last (P,X,Y,Z,4); same bits.
 *   pass_mask  (P, X*Y*Z) uint16 in the format of sp3d_unproject_fwd_train at J = 1: bit 0 set where the pre-clamp value
 *              lies in [0,1] and the voxel is not NaN-zeroed (a voxel no view sees has a pre-clamp value of 0: set); bits
 *              1..15 zero; the words of a cube that `valid` skips are zero.  The words are those the packed training forward
 *              writes for the contiguous channel, so either forward's mask serves either backward.
 * SP3D_EUNSUPPORTED, before any launch, for J other than 1 or 4, a channels-last result with J = 1, either bf16 flag,
 * heat-maps narrower or lower than 2 pixels or of more than 2^24 pixels, a sample of more than 2^31 bytes; SP3D_EINVAL for
 * Jp < 1, V > SP3D_MAX_VIEWS, an unknown layout byte; SP3D_ENULL for a missing pointer (grids may be NULL).
 * sp3d_unproject_fwd_train itself keeps refusing SP3D_HM_ONE_CHANNEL.
 */
int sp3d_unproject_one_fwd_train(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                 const int32_t *sample_of, const float *centers, const uint8_t *valid, float *cubes,
                                 float *grids, uint16_t *pass_mask, int P, int V, int J, int h, int w, int X, int Y, int Z,
                                 const float *grid_size, int W_in, int H_in, void *stream);

/*
 * Gradient of that forward w.r.t. the one heat-map channel; reads no heat-map.  One lane per voxel, one memory atomic per
 * non-zero tap: no pad channels are scattered (sp3d_unproject_bwd_packed at Jp = 4 adds three zeros per value).
 *   grad_cubes        channel 0 of cube p is X*Y*Z contiguous floats at grad_cubes + p * grad_cube_stride: the stride is
 *                     X*Y*Z for a (P,1,X,Y,Z) gradient and 4*X*Y*Z for a planar (P,4,X,Y,Z) one (no slice copy);
 *                     SP3D_EINVAL below X*Y*Z
 *   pass_mask         (P, X*Y*Z) uint16, bit 0 read (sp3d_unproject_one_fwd_train's or sp3d_unproject_fwd_train's words)
 *   grad_hm           (V,B,h,w) fp32, dense, ZERO-FILLED by the caller: plane (c, sample_of[p]) receives cube p's taps in
 *                     view c (fp32 atomics: the summation order is the hardware's)
 * The products added are (grad / den) * w, formed as sp3d_unproject_bwd_packed forms them.
 * SP3D_EINVAL for a dimension <= 0 or V > SP3D_MAX_VIEWS, SP3D_ERANGE for sizes beyond 32-bit voxel indexing, SP3D_ENULL for
 * a missing pointer (sample_of may be NULL), SP3D_EUNSUPPORTED for heat-maps narrower or lower than 2 pixels or of more than
 * 2^24 pixels - all before any launch.
 */
int sp3d_unproject_one_bwd(const float *cam, const int32_t *sample_of, const float *centers, const uint8_t *valid,
                           const float *grad_cubes, int64_t grad_cube_stride, const uint16_t *pass_mask, float *grad_hm,
                           int B, int P, int V, int h, int w, int X, int Y, int Z, const float *grid_size, int W_in,
                           int H_in, void *stream);

/*
 * DETERMINISTIC form: round(v * scale) is added to grad_fixed (V,B,h,w) int64 (zero-filled by the caller) with integer
 * atomics, under the contract of sp3d_unproject_bwd_packed_det (`scale`: DEVICE float 2^k, |v * scale| < 2^50).  The integers
 * are those sp3d_unproject_bwd_packed_det adds to channel 0 for the same gradient, mask and scale, whichever scatter it
 * uses: the sums are equal bit for bit.  sp3d_fixed_to_float converts back.
 */
int sp3d_unproject_one_bwd_det(const float *cam, const int32_t *sample_of, const float *centers, const uint8_t *valid,
                               const float *grad_cubes, int64_t grad_cube_stride, const uint16_t *pass_mask,
                               int64_t *grad_fixed, const float *scale, int B, int P, int V, int h, int w, int X, int Y,
                               int Z, const float *grid_size, int W_in, int H_in, void *stream);

#endif /* SP3D_ONE_TRAIN_H */
