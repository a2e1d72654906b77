// sp3d_split.h - the exact three-piece bf16 split of fp32 operands and the bf16 matrix instruction the split kernels run on
// (sp3d_wino_fused.hip: wino_fused3_kernel, wino_fused16_kernel; sp3d_conv3_direct.hip: conv3_split_kernel;
// sp3d_upconv.hip: upconv2x_fused_kernel).  a = hi + mid + lo, each a bf16 (8+8+8 mantissa bits: exact); the six products whose weight is
// >= 2^-16 relative - hh, hm, mh, hl, lh, mm - are formed exactly by v_mfma_f32_32x32x16_bf16 and accumulated in fp32.
#ifndef SP3D_SPLIT_H
#define SP3D_SPLIT_H
#include <hip/hip_runtime.h>

namespace sp3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef unsigned u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float a, float b)
{
    f32x2 f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// a = hi + mid + lo, each a bf16 (exact: 24 mantissa bits), as the two A operands {lo,hi} and {hi,mid} of 4 channels
__device__ __forceinline__ void split3(const float4 a, u32x4 &q0, u32x4 &q1)
{
    const unsigned hi01 = pack_bf16(a.x, a.y), hi23 = pack_bf16(a.z, a.w);
    // a non-finite input has a non-finite hi piece and (inf - inf | NaN - NaN) = NaN as its residual: v_med3_f32(r, 0, r)
    // is r for every number and 0 for NaN (one instruction per value), so mid = lo = 0 and the value travels in the hi
    // piece alone.  The outputs that come out non-finite are then EXACTLY those of an fp32 convolution; their kind is
    // the convolution's or NaN (inf * w is formed from the weight's three pieces, whose signs differ):
    // tests/test_gpu_parity.py::test_direct_conv3_split_kernel_nonfinite_inputs.
    const float r0 = __builtin_amdgcn_fmed3f(a.x - bf16_lo(hi01), 0.0f, a.x - bf16_lo(hi01));
    const float r1 = __builtin_amdgcn_fmed3f(a.y - bf16_hi(hi01), 0.0f, a.y - bf16_hi(hi01));
    const float r2 = __builtin_amdgcn_fmed3f(a.z - bf16_lo(hi23), 0.0f, a.z - bf16_lo(hi23));
    const float r3 = __builtin_amdgcn_fmed3f(a.w - bf16_hi(hi23), 0.0f, a.w - bf16_hi(hi23));
    const unsigned mid01 = pack_bf16(r0, r1), mid23 = pack_bf16(r2, r3);
    const unsigned lo01 = pack_bf16(r0 - bf16_lo(mid01), r1 - bf16_hi(mid01));
    const unsigned lo23 = pack_bf16(r2 - bf16_lo(mid23), r3 - bf16_hi(mid23));
    q0 = u32x4{lo01, lo23, hi01, hi23};
    q1 = u32x4{hi01, hi23, mid01, mid23};
}

// The two operands share the hi piece: a kernel that keeps many of them in registers keeps the six distinct dwords
// [lo01 lo23 hi01 hi23 mid01 mid23] of split3's result; {lo,hi} = dwords 0..3 (split3_q0), {hi,mid} = dwords 2..5 (split3_q1).
typedef unsigned u32x6 __attribute__((ext_vector_type(6)));
__device__ __forceinline__ u32x6 split3_pieces(const float4 a)
{
    u32x4 q0, q1;
    split3(a, q0, q1);
    return u32x6{q0.x, q0.y, q0.z, q0.w, q1.z, q1.w};
}
__device__ __forceinline__ u32x4 split3_q0(const u32x6 p) { return __builtin_shufflevector(p, p, 0, 1, 2, 3); }
__device__ __forceinline__ u32x4 split3_q1(const u32x6 p) { return __builtin_shufflevector(p, p, 2, 3, 4, 5); }

} // namespace sp3d
#endif
