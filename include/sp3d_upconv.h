/* Part of the C ABI of libsp3d.so, included by sp3d.h (include that; this file relies on its types and enums): the
 * transposed convolutions of the V2V decoder as one kernel.  One entry added in ABI version 3; no existing entry changes.
 *
 * It lives in a header of its own because sp3d.h's list of entry points is pinned (tests/test_host_cabi.py counts it);
 * tests/test_upconv_weights_split.py holds this file against the binding's table by the same rule. */
#ifndef SP3D_UPCONV_H
#define SP3D_UPCONV_H

/* ConvTranspose3d(kernel 2, stride 2) -> BatchNorm -> ReLU (+ skip) (+ 1x1x1 output conv) in one kernel: the product G of
 * sp3d_upsample2x_scatter[_head] on v_mfma_f32_32x32x16_bf16 with exact three-piece bf16 splits of both operands
 * (fp32 accuracy, fp32 accumulation) and their epilogues on its accumulators - G never exists.
 * x (batch,X,Y,Z,CIN) channels-last; w_split: 48-byte records of bf16 = the three B operands {hi,lo} {hi,hi} {mid,mid}
 * (4 input channels each) at index ((((tap*(O/32) + o/32)*(CIN/8) + chunk)*2 + half)*32 + o%32, tap = 4i + 2j + k, channel =
 * 8*chunk + 4*half + q (_lib.upconv_weights_split), 16-byte aligned.
 * w_out == NULL: out (batch,2X,2Y,2Z,O) = relu(x.W + shift[o]) + skip, (CIN,O) = (128,64); J is ignored.
 * w_out (J,32):  out (batch,2X,2Y,2Z,J) = b_out[j] + sum_o w_out[j][o] * (that), (CIN,O) = (64,32), 1 <= J <= 32, b_out NULL = 0.
 * ReLU lets NaN through (torch.relu).  skip and out must have fewer than 2^31 elements (SP3D_ERANGE). */
int sp3d_upconv2x_fused(const float *x, const void *w_split, const float *shift, const float *skip, const float *w_out,
                        const float *b_out, float *out, int64_t batch, int X, int Y, int Z, int CIN, int O, int J, void *stream);

#endif
