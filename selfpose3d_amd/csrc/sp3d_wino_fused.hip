// sp3d_wino_fused.hip - Winograd F(2x2x2, 3x3x3) as ONE kernel per layer for the full- and half-resolution 3x3x3
// convolutions of the V2V nets in inference: wino_fused_kernel (fp32 matrix pipe), wino_fused3_kernel (the same on the
// bf16 pipe with exact three-piece splits) at full resolution, wino_fused16_kernel at half resolution, and their C
// entries.  The three-launch form of the quarter resolution is sp3d_wino.hip, the direct convolution sp3d_conv3_direct.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sp3d.h"
#include "sp3d_conv3_host.h"
#include "sp3d_split.h"

// ------------------------------------------------------------------------------------------
// Fused Winograd F(2x2x2, 3x3x3) for the FULL-resolution 3x3x3 layers (C = 16 or 32 -> O = 32), where the
// transformed tensor of the three-launch form (sp3d_wino.hip) would be 524 MB.  One wave = a block of 4x4x2 tiles (8x8x4
// outputs x 32 channels); nothing but x, U and y touches memory:
//   per chunk of 8 input channels: stage the 10x10x6 input region in LDS (20.2 KB, 16-byte aligned rows);
//   per transform point: each lane builds its A operand on the fly - V[p][tile][c] is a signed sum of 8 region
//     voxels (B^T has two non-zeros per row) - B = U[p][c][o] streams from L2, and v_mfma_f32_32x32x2_f32
//     (tiles x outputs, K = 8 channels) accumulates;
//   the inverse transform is linear: along x it is folded into the MFMA accumulation, along y,z it is applied to
//     the accumulators on the VALU; nothing transformed is ever stored.
// ------------------------------------------------------------------------------------------

namespace sp3d {

#ifdef SP3D_WF_TIMELINE
__device__ unsigned long long *g_wf_tl = nullptr;
#define WF_STAMP(slot) do { __builtin_amdgcn_sched_barrier(0); if (tl && lane == 0) tl[slot] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define WF_STAMP(slot) do { } while (0)
#endif

constexpr int WF_RX = 10, WF_RY = 10, WF_RZ = 6;
constexpr int WF_VS = 8;                       // floats per staged voxel (one chunk of 8 input channels)
// Row pitch 84 floats: rows stay 16-byte aligned, so a lane fetches its 4 channels of a voxel with ONE ds_read_b128 (and the
// staging writes are ds_write_b128).  With stride-2 tiles the 16 lanes of a b128 lane group can spread over only 32 of
// the 64 banks whatever the pitch (2*tty*ROW + 2*ttz*PLANE is a multiple of 8 floats): 2-way conflicts, 8 LDS cycles per
// instruction, 16 instructions per (j,k) step = 128 cycles - against 64 ds_read_b32 x >= 4 cycles with the former odd
// pitch (profiles/r01_pmc_wino_fused.json: 74 % of the LDS cycles were conflicts).
constexpr int WF_ROW = WF_RX * WF_VS + 4;
constexpr int WF_LDS = WF_RY * WF_RZ * WF_ROW; // 5 040 floats = 20 160 B -> 8 waves per CU (161 280 of 163 840 B)

// B^T rows as (first tap +, second tap, sign of second): d0-d2, d1+d2, d2-d1, d1-d3
__device__ constexpr int wf_ta(int r) { return r == 0 ? 0 : (r == 1 ? 1 : (r == 2 ? 2 : 1)); }
__device__ constexpr int wf_tb(int r) { return r == 0 ? 2 : (r == 1 ? 2 : (r == 2 ? 1 : 3)); }
__device__ constexpr float wf_sb(int r) { return r == 1 ? 1.0f : -1.0f; }
// A^T = [[1,1,1,0],[0,1,-1,-1]]
__device__ constexpr float wf_at(int a, int r) { return a == 0 ? (r < 3 ? 1.0f : 0.0f) : (r == 0 ? 0.0f : (r == 1 ? 1.0f : -1.0f)); }

template <int C, int MODE>
__global__ __launch_bounds__(64) void wino_fused_kernel(const float *__restrict__ x, const float *__restrict__ U,
                                                       float *__restrict__ y, const float *__restrict__ shift,
                                                       const float *__restrict__ res, int B, int X, int Y, int Z, int NBX,
                                                       int NBY, int NBZ)
{
    constexpr int O = 32;
    __shared__ __attribute__((aligned(16))) float region[WF_LDS];
    const int lane = threadIdx.x, t = lane & 31, h = lane >> 5;
    int bid = blockIdx.x;
    const int bz = bid % NBZ; bid /= NBZ;
    const int by = bid % NBY; bid /= NBY;
    const int bx = bid % NBX;
    const int b = bid / NBX;
    const int ttx = t & 3, tty = (t >> 2) & 3, ttz = t >> 4;
    const int ox0 = bx * 8, oy0 = by * 8, oz0 = bz * 4;                 // first output voxel of the block
    // region address of (vx,vy,vz,c) = (vz*RY + vy)*ROW + vx*VS + c; this tile's patch origin.  MFMA k-slot h of step kk
    // carries channel kk + 4*h of the chunk, so a lane's four channels (kk = 0..3) are 16 contiguous bytes
    const float *rb = region + ((2 * ttz) * WF_RY + 2 * tty) * WF_ROW + (2 * ttx) * WF_VS + 4 * h;

    f32x16 acc[8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[a][v] = 0.0f;
#ifdef SP3D_WF_TIMELINE
    unsigned long long *tl = g_wf_tl ? g_wf_tl + (size_t)blockIdx.x * 80 : nullptr;
#endif
    WF_STAMP(0);

#pragma unroll 1
    for (int cc = 0; cc < C / 8; ++cc) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // stage 600 voxels x 8 channels = 1200 float4, 5 loads in flight per lane
#pragma unroll 1
        for (int i0 = 0; i0 < WF_RX * WF_RY * WF_RZ * 2; i0 += 64 * 5) {
            float4 d[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int idx = i0 + u * 64 + lane;
                const int v = idx >> 1, half = idx & 1;
                const int vx = v % WF_RX, vy = (v / WF_RX) % WF_RY, vz = v / (WF_RX * WF_RY);
                const int gx = ox0 - 1 + vx, gy = oy0 - 1 + vy, gz = oz0 - 1 + vz;
                d[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (idx < WF_RX * WF_RY * WF_RZ * 2 && gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z)
                    d[u] = *reinterpret_cast<const float4 *>(x + ((((int64_t)b * X + gx) * Y + gy) * Z + gz) * C + cc * 8 + half * 4);
            }
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int idx = i0 + u * 64 + lane;
                if (idx < WF_RX * WF_RY * WF_RZ * 2) {
                    const int v = idx >> 1, half = idx & 1;
                    const int vx = v % WF_RX, vy = (v / WF_RX) % WF_RY, vz = v / (WF_RX * WF_RY);
                    *reinterpret_cast<float4 *>(region + (vz * WF_RY + vy) * WF_ROW + vx * WF_VS + half * 4) = d[u];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const float *ub = U + ((int64_t)(cc * 8 + 4 * h)) * O + t;         // + p*C*O + kk*O
        // (y,z) index of the transform point: run-time loop; x index: unrolled.  The inverse transform along x is
        // folded into the MFMA accumulation (two accumulators, A^T = [1,1,1,0] / [0,1,-1,-1] as +-A operands), the one
        // along y,z is applied once per (j,k) on the VALU with wave-uniform coefficients.
        // one (j,k) step; bcur = its 16 B operands (fetched one step ahead: they come from L2, ~700 cycles away),
        // bnxt receives those of step jk_next
        auto step = [&](int jk, int jk_next, const float (&bcur)[16], float (&bnxt)[16]) {
            const int j = jk >> 2, k = jk & 3;
            const int ya = (j == 0) ? 0 : ((j == 2) ? 2 : 1), yb = (j == 3) ? 3 : ((j == 2) ? 1 : 2);
            const int za = (k == 0) ? 0 : ((k == 2) ? 2 : 1), zb = (k == 3) ? 3 : ((k == 2) ? 1 : 2);
            const float sy = (j == 1) ? 1.0f : -1.0f, sz = (k == 1) ? 1.0f : -1.0f;
            const float *r00 = rb + (za * WF_RY + ya) * WF_ROW, *r10 = rb + (za * WF_RY + yb) * WF_ROW;
            const float *r01 = rb + (zb * WF_RY + ya) * WF_ROW, *r11 = rb + (zb * WF_RY + yb) * WF_ROW;
            const float *un = ub + (int64_t)jk_next * C * O;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) bnxt[i * 4 + kk] = un[(int64_t)(i * 16) * C * O + kk * O];
            float g[4][4];                                                 // [x tap][kk]: y,z transform done
#pragma unroll
            for (int xi = 0; xi < 4; ++xi) {
                const float4 v00 = *reinterpret_cast<const float4 *>(r00 + xi * WF_VS), v10 = *reinterpret_cast<const float4 *>(r10 + xi * WF_VS);
                const float4 v01 = *reinterpret_cast<const float4 *>(r01 + xi * WF_VS), v11 = *reinterpret_cast<const float4 *>(r11 + xi * WF_VS);
                g[xi][0] = fmaf(sz, fmaf(sy, v11.x, v01.x), fmaf(sy, v10.x, v00.x));
                g[xi][1] = fmaf(sz, fmaf(sy, v11.y, v01.y), fmaf(sy, v10.y, v00.y));
                g[xi][2] = fmaf(sz, fmaf(sy, v11.z, v01.z), fmaf(sy, v10.z, v00.z));
                g[xi][3] = fmaf(sz, fmaf(sy, v11.w, v01.w), fmaf(sy, v10.w, v00.w));
            }
            if (cc == 0) WF_STAMP(8 + 4 * jk);                             // operands ready
            // wave-uniform y,z coefficients of A^T for the four (b,c) output positions
            float cyz[4];
#pragma unroll
            for (int bc = 0; bc < 4; ++bc) {
                const int bb = bc >> 1, c2 = bc & 1;
                const float cy = bb == 0 ? (j < 3 ? 1.0f : 0.0f) : (j == 0 ? 0.0f : (j == 1 ? 1.0f : -1.0f));
                const float cz = c2 == 0 ? (k < 3 ? 1.0f : 0.0f) : (k == 0 ? 0.0f : (k == 1 ? 1.0f : -1.0f));
                cyz[bc] = cy * cz;
            }
            f32x16 M0, M1;
#pragma unroll
            for (int v = 0; v < 16; ++v) { M0[v] = 0.0f; M1[v] = 0.0f; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const float av = (i == 1) ? g[1][kk] + g[2][kk] : g[wf_ta(i)][kk] - g[wf_tb(i)][kk];
                    const float bv = bcur[i * 4 + kk];
                    if (i < 3) M0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, M0, 0, 0, 0);
                    if (i > 0) M1 = __builtin_amdgcn_mfma_f32_32x32x2f32(i == 1 ? av : -av, bv, M1, 0, 0, 0);
                }
            if (cc == 0) WF_STAMP(9 + 4 * jk);                             // MFMAs issued
#pragma unroll
            for (int bc = 0; bc < 4; ++bc) {
                const float coef = cyz[bc];
                if (coef != 0.0f) {
                    f32x16 cv;
#pragma unroll
                    for (int v = 0; v < 16; ++v) cv[v] = coef;
                    acc[bc] = __builtin_elementwise_fma(M0, cv, acc[bc]);
                    acc[4 + bc] = __builtin_elementwise_fma(M1, cv, acc[4 + bc]);
                }
            }
            if (cc == 0) WF_STAMP(10 + 4 * jk);                            // accumulated
        };
        float b0[16], b1[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) b0[i * 4 + kk] = ub[(int64_t)(i * 16) * C * O + kk * O];
#pragma unroll 1
        for (int jk = 0; jk < 16; jk += 2) {
            step(jk, jk + 1, b0, b1);
            step(jk + 1, (jk + 2) & 15, b1, b0);
        }
    }

    WF_STAMP(5);                                                           // all chunks done
    const float sh = shift[t];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        // residual values of this output position first, 16 loads in flight (clamped addresses, no predicate): inside the
        // bounds branch they came out as load -> s_waitcnt vmcnt(0) -> store chains, one memory round trip per element
        float rv[16];
        if (MODE >= 2) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = 8 * (v >> 2) + (v & 3) + 4 * h;
                const int rx = row & 3, ry = (row >> 2) & 3, rz = row >> 4;
                const int xo = min(ox0 + 2 * rx + (a >> 2), X - 1), yo = min(oy0 + 2 * ry + ((a >> 1) & 1), Y - 1);
                const int zo = min(oz0 + 2 * rz + (a & 1), Z - 1);
                rv[v] = res[((((int64_t)b * X + xo) * Y + yo) * Z + zo) * O + t];
            }
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = 8 * (v >> 2) + (v & 3) + 4 * h;              // tile of this accumulator element
            const int rx = row & 3, ry = (row >> 2) & 3, rz = row >> 4;
            const int xo = ox0 + 2 * rx + (a >> 2), yo = oy0 + 2 * ry + ((a >> 1) & 1), zo = oz0 + 2 * rz + (a & 1);
            if (xo < X && yo < Y && zo < Z) {
                const int64_t idx = ((((int64_t)b * X + xo) * Y + yo) * Z + zo) * O + t;
                float val = acc[a][v] + sh;
                if (MODE == 2) val += rv[v];
                if (MODE >= 1) val = fmaxf(val, 0.0f);
                if (MODE == 3) val += rv[v];
                y[idx] = val;
            }
        }
    }
}


// ------------------------------------------------------------------------------------------
// The same kernel with the products on the bf16 matrix pipe at fp32 accuracy.  v_mfma_f32_32x32x2_f32 runs at 1/16 of
// the bf16 rate and (profiles/r02_pmc_wino_fused.json) keeps the matrix pipe 75 % busy at a throttled clock.
// Every fp32 operand is split into three bf16 pieces a = hi + mid + lo (8+8+8 mantissa bits: exact), the six products
// whose weight is >= 2^-16 relative - hh, hm, mh, hl, lh, mm - are formed exactly by v_mfma_f32_32x32x16_bf16
// (bf16 x bf16 fits fp32) and accumulated in fp32; the dropped terms are < 2^-24 relative, i.e. below one fp32 ulp of
// the product.  K = 16 of one MFMA = 4 channels x 2 (A piece, B piece) pairs per lane half:
//     {hi,hi} x {bm,bh}   +   {mid,mid} x {bm,bh}   +   {lo,hi} x {bh,bl}
// so 8 channels cost 3 MFMAs of 8 passes instead of 4 of 16: 2.7x fewer matrix cycles; the weights are split once on
// the host (U3: per (point, chunk, lane half, output) one 24-byte record [bm(4ch) bh(4ch) bl(4ch)]).
// ------------------------------------------------------------------------------------------
struct WfB { u32x4 mh; u32x2 l; };              // [bm01 bm23 bh01 bh23] [bl01 bl23]

template <int C, int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void wino_fused3_kernel(const float *__restrict__ x, const unsigned *__restrict__ U3,
                                                        float *__restrict__ y, const float *__restrict__ shift,
                                                        const float *__restrict__ res, int B, int X, int Y, int Z, int NBX,
                                                        int NBY, int NBZ)
{
    constexpr int O = 32, NCH = C / 8;
    __shared__ __attribute__((aligned(16))) float region[WF_LDS];
    const int lane = threadIdx.x, t = lane & 31, h = lane >> 5;
    int bid = blockIdx.x;
    const int bz = bid % NBZ; bid /= NBZ;
    const int by = bid % NBY; bid /= NBY;
    const int bx = bid % NBX;
    const int b = bid / NBX;
    const int ttx = t & 3, tty = (t >> 2) & 3, ttz = t >> 4;
    const int ox0 = bx * 8, oy0 = by * 8, oz0 = bz * 4;
    const float *rb = region + ((2 * ttz) * WF_RY + 2 * tty) * WF_ROW + (2 * ttx) * WF_VS + 4 * h;

    f32x16 acc[8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[a][v] = 0.0f;

    // staging constants of this lane: region voxel (x = u >> 1, y = 5 * (u & 1) + sr, z = sz_), channel half sh_
    const int sh_ = lane & 1, sz_ = (lane >> 1) % WF_RZ, sr = (lane >> 1) / WF_RZ;       // lanes 60..63 idle
    const int sgz = oz0 - 1 + sz_, sgy0 = oy0 - 1 + sr, sgy1 = sgy0 + 5;
    const bool sg_inz = sgz >= 0 && sgz < Z, sg_iny0 = sgy0 >= 0 && sgy0 < Y, sg_iny1 = sgy1 >= 0 && sgy1 < Y;
    const int64_t sg_base = ((((int64_t)b * X + (ox0 - 1)) * Y + sgy0) * Z + sgz) * C + sh_ * 4;
    const int sg_lds = (sz_ * WF_RY + sr) * WF_ROW + sh_ * 4;

#pragma unroll 1
    for (int cc = 0; cc < NCH; ++cc) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // stage 600 voxels x 8 channels = 1200 float4, 5 loads in flight per lane (10 or all 19 at once measured no
        // faster: the accumulators start to spill).  Lane = (half, z, column-of-5): the (x,y) column of batch element u
        // is (u >> 1, 5 * (u & 1) + r), so every address is a per-lane constant plus a compile-time offset - the former
        // idx -> (x,y,z) divisions cost 60 VALU instructions per element, a fifth of the kernel's instruction count
        {
            const bool on = lane < 60;
            const int64_t gbase = sg_base + cc * 8;                           // + (x * Y + y5) * Z * C per element
#pragma unroll 1
            for (int u0 = 0; u0 < 20; u0 += 5) {
                float4 d[5];
#pragma unroll
                for (int uu = 0; uu < 5; ++uu) {
                    const int u = u0 + uu;
                    const int gx = ox0 - 1 + (u >> 1);
                    const bool iny = (u & 1) ? sg_iny1 : sg_iny0;
                    d[uu] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (on && sg_inz && iny && gx >= 0 && gx < X)
                        d[uu] = *reinterpret_cast<const float4 *>(x + gbase + ((int64_t)(u >> 1) * Y + 5 * (u & 1)) * Z * C);
                }
#pragma unroll
                for (int uu = 0; uu < 5; ++uu) {
                    const int u = u0 + uu;
                    if (on) *reinterpret_cast<float4 *>(region + sg_lds + 5 * (u & 1) * WF_ROW + (u >> 1) * WF_VS) = d[uu];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // record of (point p = i*16 + jk, chunk cc, lane half h, output t): 6 dwords
        const unsigned *ub = U3 + (((int64_t)cc * 2 + h) * 32 + t) * 6;
        auto load_b = [&](int i, int jk) {
            const unsigned *r = ub + (int64_t)(i * 16 + jk) * NCH * 2 * 32 * 6;
            WfB w;
#if SP3D_W16_ABLATE & 2
            (void)r;
            w.mh = u32x4{0x3f803f80u + (unsigned)jk, 0x3f803f80u, 0x3f803f80u + (unsigned)i, 0x3f803f80u};
            w.l = u32x2{0x3f803f80u, 0x3f803f80u};
#else
            w.mh = *reinterpret_cast<const u32x4_a8 *>(r);
            w.l = *reinterpret_cast<const u32x2_a8 *>(r + 4);
#endif
            return w;
        };
        // B of x points 0,1 arrives one step ahead; B of x points 2,3 is fetched at the top of its own step (it is
        // needed ~600 cycles later): 36 registers of weights in flight instead of 48
        auto step = [&](int jk, int jk_next, const WfB (&bcur)[2], WfB (&bnxt)[2]) {
            const int j = jk >> 2, k = jk & 3;
            const int ya = (j == 0) ? 0 : ((j == 2) ? 2 : 1), yb = (j == 3) ? 3 : ((j == 2) ? 1 : 2);
            const int za = (k == 0) ? 0 : ((k == 2) ? 2 : 1), zb = (k == 3) ? 3 : ((k == 2) ? 1 : 2);
            const float sy = (j == 1) ? 1.0f : -1.0f, sz = (k == 1) ? 1.0f : -1.0f;
            const float *r00 = rb + (za * WF_RY + ya) * WF_ROW, *r10 = rb + (za * WF_RY + yb) * WF_ROW;
            const float *r01 = rb + (zb * WF_RY + ya) * WF_ROW, *r11 = rb + (zb * WF_RY + yb) * WF_ROW;
            WfB blate[2];
            blate[0] = load_b(2, jk);
            blate[1] = load_b(3, jk);
            float g[4][4];
#pragma unroll
            for (int xi = 0; xi < 4; ++xi) {
#if SP3D_W16_ABLATE & 8
                const float f0 = __int_as_float(0x3f800000 + jk + xi), f1 = __int_as_float(0x3f900000 + lane);
                const float4 v00 = make_float4(f0, f1, f0, f1), v10 = make_float4(f1, f0, f1, f0), v01 = v00, v11 = v10;
                (void)r00; (void)r10; (void)r01; (void)r11;
#else
                const float4 v00 = *reinterpret_cast<const float4 *>(r00 + xi * WF_VS), v10 = *reinterpret_cast<const float4 *>(r10 + xi * WF_VS);
                const float4 v01 = *reinterpret_cast<const float4 *>(r01 + xi * WF_VS), v11 = *reinterpret_cast<const float4 *>(r11 + xi * WF_VS);
#endif
                g[xi][0] = fmaf(sz, fmaf(sy, v11.x, v01.x), fmaf(sy, v10.x, v00.x));
                g[xi][1] = fmaf(sz, fmaf(sy, v11.y, v01.y), fmaf(sy, v10.y, v00.y));
                g[xi][2] = fmaf(sz, fmaf(sy, v11.z, v01.z), fmaf(sy, v10.z, v00.z));
                g[xi][3] = fmaf(sz, fmaf(sy, v11.w, v01.w), fmaf(sy, v10.w, v00.w));
            }
            float cyz[4];
#pragma unroll
            for (int bc = 0; bc < 4; ++bc) {
                const int bb = bc >> 1, c2 = bc & 1;
                const float cy = bb == 0 ? (j < 3 ? 1.0f : 0.0f) : (j == 0 ? 0.0f : (j == 1 ? 1.0f : -1.0f));
                const float cz = c2 == 0 ? (k < 3 ? 1.0f : 0.0f) : (k == 0 ? 0.0f : (k == 1 ? 1.0f : -1.0f));
                cyz[bc] = cy * cz;
            }
            f32x16 M0, M1;
#pragma unroll
            for (int v = 0; v < 16; ++v) { M0[v] = 0.0f; M1[v] = 0.0f; }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // x transform: d0-d2, d1+d2, d2-d1, d1-d3; point 3 enters M1 with a minus sign: negate it here
                float av[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    av[kk] = (i == 1) ? g[1][kk] + g[2][kk] : ((i == 3) ? g[3][kk] - g[1][kk] : g[wf_ta(i)][kk] - g[wf_tb(i)][kk]);
                // a = hi + mid + lo, each a bf16 (exact: 24 mantissa bits)
                const unsigned hi01 = pack_bf16(av[0], av[1]), hi23 = pack_bf16(av[2], av[3]);
#if SP3D_W16_ABLATE & 4
                const unsigned mid01 = hi01, mid23 = hi23, lo01 = hi01, lo23 = hi23;
#else
                const float r0 = av[0] - bf16_lo(hi01), r1 = av[1] - bf16_hi(hi01), r2 = av[2] - bf16_lo(hi23), r3 = av[3] - bf16_hi(hi23);
                const unsigned mid01 = pack_bf16(r0, r1), mid23 = pack_bf16(r2, r3);
                const unsigned lo01 = pack_bf16(r0 - bf16_lo(mid01), r1 - bf16_hi(mid01));
                const unsigned lo23 = pack_bf16(r2 - bf16_lo(mid23), r3 - bf16_hi(mid23));
#endif
                const u32x4 Qhh = {hi01, hi23, hi01, hi23}, Qmm = {mid01, mid23, mid01, mid23}, Qlh = {lo01, lo23, hi01, hi23};
                const WfB &w = (i < 2) ? bcur[i] : blate[i - 2];
                const u32x4 Bmh = w.mh;
                const u32x4 Bhl = {w.mh.z, w.mh.w, w.l.x, w.l.y};
#if SP3D_W16_ABLATE & 1
                {   // no matrix instructions: keep every operand alive with one integer op each
                    const unsigned z = (Qhh.x ^ Bmh.x) + (Qmm.y ^ Bmh.z) + (Qlh.x ^ Bhl.w) + (Qlh.z ^ Bhl.y);
                    M0[0] += __uint_as_float(z & 0x3fffffffu);
                    M1[1] += __uint_as_float((z >> 1) & 0x3fffffffu);
                    if (i == 1) {
                        bnxt[0] = load_b(0, jk_next);
                        bnxt[1] = load_b(1, jk_next);
                    }
                    continue;
                }
#endif
                if (i < 3) {
                    M0 = mfma_bf16(Qhh, Bmh, M0);
                    M0 = mfma_bf16(Qmm, Bmh, M0);
                    M0 = mfma_bf16(Qlh, Bhl, M0);
                }
                if (i == 1 || i == 3) {
                    M1 = mfma_bf16(Qhh, Bmh, M1);
                    M1 = mfma_bf16(Qmm, Bmh, M1);
                    M1 = mfma_bf16(Qlh, Bhl, M1);
                }
                if (i == 2) {                                      // M1 -= A.B: flip the sign bits of the weights
                    const u32x4 nmh = Bmh ^ 0x80008000u, nhl = Bhl ^ 0x80008000u;
                    M1 = mfma_bf16(Qhh, nmh, M1);
                    M1 = mfma_bf16(Qmm, nmh, M1);
                    M1 = mfma_bf16(Qlh, nhl, M1);
                }
                if (i == 1) {                                      // next step's early weights, mid-step
                    bnxt[0] = load_b(0, jk_next);
                    bnxt[1] = load_b(1, jk_next);
                }
            }
#pragma unroll
            for (int bc = 0; bc < 4; ++bc) {
                const float coef = cyz[bc];
                if (coef != 0.0f) {
                    f32x16 cv;
#pragma unroll
                    for (int v = 0; v < 16; ++v) cv[v] = coef;
                    acc[bc] = __builtin_elementwise_fma(M0, cv, acc[bc]);
                    acc[4 + bc] = __builtin_elementwise_fma(M1, cv, acc[4 + bc]);
                }
            }
        };
        WfB b0[2], b1[2];
        b0[0] = load_b(0, 0);
        b0[1] = load_b(1, 0);
#pragma unroll 1
        for (int jk = 0; jk < 16; jk += 2) {
            step(jk, jk + 1, b0, b1);
            step(jk + 1, (jk + 2) & 15, b1, b0);
        }
    }

    // accumulator element (a, v) of lane (t, h) is output voxel (ox0 + dx, oy0 + 2h + dy, oz0 + dz), channel t, with
    // dx = 2 (v & 3) + (a >> 2), dy = 4 ((v >> 2) & 1) + ((a >> 1) & 1), dz = 2 (v >> 3) + (a & 1) known at compile time:
    // one per-lane base address, wave-uniform offsets and bounds (only the y bound depends on the lane)
    const float sh = shift[t];
    const int yl = oy0 + 2 * h;
    const int64_t obase = ((((int64_t)b * X + ox0) * Y + yl) * Z + oz0) * O + t;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        float rv[16];                                 // residual values first (see wino_fused_kernel): clamped, unpredicated
        if (MODE >= 2) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int dx = 2 * (v & 3) + (a >> 2), dy = 4 * ((v >> 2) & 1) + ((a >> 1) & 1), dz = 2 * (v >> 3) + (a & 1);
                const int xo = min(ox0 + dx, X - 1), yo = min(yl + dy, Y - 1), zo = min(oz0 + dz, Z - 1);
                rv[v] = res[((((int64_t)b * X + xo) * Y + yo) * Z + zo) * O + t];
            }
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int dx = 2 * (v & 3) + (a >> 2), dy = 4 * ((v >> 2) & 1) + ((a >> 1) & 1), dz = 2 * (v >> 3) + (a & 1);
            if (ox0 + dx < X && oz0 + dz < Z && yl + dy < Y) {
                const int64_t idx = obase + (((int64_t)dx * Y + dy) * Z + dz) * O;
                float val = acc[a][v] + sh;
                if (MODE == 2) val += rv[v];
                if (MODE >= 1) val = fmaxf(val, 0.0f);
                if (MODE == 3) val += rv[v];
                y[idx] = val;
            }
        }
    }
}

// Fused Winograd F(2x2x2,3x3x3) for the HALF-resolution layers (C = 32 | 64 -> O = 64 on 40x40x10): the three-launch form
// (input transform, 64 batched GEMMs, output transform) moves the 131 MB transformed tensor four times (115 us per
// layer, HBM/MALL-bound); here nothing transformed leaves the CU.  Same scheme as wino_fused3_kernel - regions staged in
// LDS, operands built on the fly, exact three-piece bf16 splits, x fold on the matrix pipe, y,z fold on the VALU - on
// v_mfma_f32_16x16x32_bf16: a block is 4x4x1 tiles (8x8x2 outputs) x 64 output channels, chunks of 16 input channels
// (lane = tile x 4-channel group), and the NW waves of a workgroup share the staged region, each owning 64/NW outputs,
// so that the per-lane operand work (transforms + splits) is amortised over 16*NBW outputs.
// ------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int W16_RX = 10, W16_RY = 10, W16_RZ = 4, W16_VS = 16;
constexpr int W16_ROW = W16_RX * W16_VS + 4;
constexpr int W16_LDS = W16_RY * W16_RZ * W16_ROW;               // 6 560 floats = 26 240 B

__device__ __forceinline__ f32x4 mfma16_bf16(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// SKIP: the 1x1x1 projection of a residual block's input on the same accumulators (they are final outputs: acc[a][n], a =
// output position inside the tile, D rows = tiles), y = epilogue(conv3(x) + WS . xs + shift): xs (B,X,Y,Z,32) channels-last,
// WS = [mid hi lo] records of one point [chunk 2][group 4][output 64].  Channel group kg takes skip chunk kg before the LDS
// reduction, when the registers of the main loop are free: lane (tl, q) supplies A row = tile tl, channels 16 kg + 4 q .. + 3
// of voxel (tile, a) - 8 rows, 8 splits and 48 matrix instructions per wave.
// XD: Winograd in y and z only, the x axis as a plain 3-tap convolution.  The x part of F(2,3) buys nothing in this kernel: its
// output side is already folded into the accumulation, where the two outputs of an x pair cost six operand triples for
// four points - exactly what M0 += g0.W0 + g1.W1 + g2.W2, M1 += g1.W0 + g2.W1 + g3.W2 costs on the y,z-transformed values
// g[0..3] themselves.  So the 36 matrix instructions of a step stay, and the x input transform (16 add/sub), the sign
// flips of the weights (8 XOR per output block) and one weight record in four leave it: U3 holds 48 points dx*16 + jk
// (_lib.wino_yz_weights_split: G along y and z, raw along x) instead of 64.
// POOL (with SKIP, MODE 1, grids of whole blocks only - the entry refuses the others): the MaxPool3d(2,2) of the result as
// well, stored right behind y, (B,X/2,Y/2,Z/2,64) channels-last at y + B*X*Y*Z*64.  acc[a][n][v], a = 0..7, are the eight voxels
// (a >> 2, (a >> 1) & 1, a & 1) of the 2x2x2 tile at (ox0 + 2 v, oy0 + 2 q, oz0): one pooling cell, scanned over a in the order
// and with the comparison of maxpool2x_cl_kernel (NaN and -0/+0 come out the same bits); 16 lanes write a 64-byte channel run.
template <int C, int MODE, int NBW, int KS, bool SKIP = false, bool XD = false, bool POOL = false>
__global__ __launch_bounds__(64 * (4 / NBW) * KS) __attribute__((amdgpu_waves_per_eu(NBW <= 2 ? 2 : 1))) void wino_fused16_kernel(const float *__restrict__ x,
                                                                          const unsigned *__restrict__ U3,
                                                                          float *__restrict__ y, const float *__restrict__ shift,
                                                                          const float *__restrict__ res, int B, int X, int Y,
                                                                          int Z, int NBX, int NBY, int NBZ,
                                                                          const float *__restrict__ xs = nullptr,
                                                                          const unsigned *__restrict__ WS = nullptr)
{
    // workgroup = KS channel groups x (4 / NBW) output groups of one wave each: channel group kg owns the 16-channel
    // chunks kg, kg + KS, ... (its own staged region), output group ow owns outputs 16*NBW*ow ...; the KS partial sums
    // meet in LDS at the end.  More waves per block without repeating the operand work: the grid of a half-resolution
    // layer is only 500 blocks.
    constexpr int O = 64, NCH = C / 16, NOW = 4 / NBW, NTG = 64 * NOW;
    static_assert(NCH % KS == 0, "chunks must divide evenly over the channel groups");
    __shared__ __attribute__((aligned(16))) float lds[KS * W16_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kg = wave / NOW, ow = wave % NOW, tg = tid - kg * NTG;          // thread index inside the channel group
    float *region = lds + kg * W16_LDS;
    const int tl = lane & 15, q = lane >> 4;
    int bid = blockIdx.x;
    const int bz = bid % NBZ; bid /= NBZ;
    const int by = bid % NBY; bid /= NBY;
    const int bx = bid % NBX;
    const int b = bid / NBX;
    const int ttx = tl & 3, tty = tl >> 2;
    const int ox0 = bx * 8, oy0 = by * 8, oz0 = bz * 2;
    const float *rb = region + (2 * tty) * W16_ROW + (2 * ttx) * W16_VS + 4 * q;

    f32x4 acc[8][NBW];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int n = 0; n < NBW; ++n) acc[a][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#ifdef SP3D_W16_SETPRIO
    __builtin_amdgcn_s_setprio(SP3D_W16_SETPRIO);       // experiment (round 5): wave priority of the matrix-instruction waves
#endif

    // region of one 16-channel chunk: 400 voxels x 4 float4; every thread of the channel group owns PER of them.  The
    // loads of the group's next chunk are issued before the 16 steps of the current one and parked in registers (a
    // dependent load->store loop costs as much as the steps themselves: ~2 us of memory latency per iteration)
    constexpr int NV4 = W16_RX * W16_RY * W16_RZ * 4, PER = (NV4 + NTG - 1) / NTG;
    int goff[PER], loff[PER];                      // global offset (floats, chunk 0; -1: padding) and LDS offset (-1: none)
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int idx = tg + u * NTG;
        const int v = idx >> 2, part = idx & 3;
        const int vx = v % W16_RX, vy = (v / W16_RX) % W16_RY, vz = v / (W16_RX * W16_RY);
        const int gx = ox0 - 1 + vx, gy = oy0 - 1 + vy, gz = oz0 - 1 + vz;
        const bool in = idx < NV4 && gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z;
        goff[u] = in ? (int)(((((int64_t)gx) * Y + gy) * Z + gz) * C + part * 4) : -1;
        loff[u] = idx < NV4 ? (vz * W16_RY + vy) * W16_ROW + vx * W16_VS + part * 4 : -1;
    }
    const float *xb = x + (int64_t)b * X * Y * Z * C;
    float4 pre[PER];
    auto fetch = [&](int cc) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            pre[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (goff[u] >= 0) pre[u] = *reinterpret_cast<const float4 *>(xb + goff[u] + cc * 16);
        }
    };
    fetch(kg);
#pragma unroll 1
    for (int cc = kg; cc < NCH; cc += KS) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u)
            if (loff[u] >= 0) *reinterpret_cast<float4 *>(region + loff[u]) = pre[u];
        __syncthreads();
        if (cc + KS < NCH) fetch(cc + KS);
        // record of (point p, chunk cc, channel group q, output o): 6 dwords [mid(4ch) hi(4ch) lo(4ch)]
        const unsigned *ub = U3 + ((((int64_t)cc * 4 + q) * O) + ow * NBW * 16 + tl) * 6;
        auto load_b = [&](int i, int jk, int n) {
            const unsigned *r = ub + (int64_t)(i * 16 + jk) * NCH * 4 * O * 6 + n * 16 * 6;
            WfB w;
            w.mh = *reinterpret_cast<const u32x4_a8 *>(r);
            w.l = *reinterpret_cast<const u32x2_a8 *>(r + 4);
            return w;
        };
#pragma unroll 1
        for (int jk = 0; jk < 16; ++jk) {
            const int j = jk >> 2, k = jk & 3;
            // this step's weights: in flight while the operands are built (~1000 cycles)
            constexpr int NXP = XD ? 3 : 4;         // records per step and output block: x taps (XD) or x points
            WfB bw[NBW][NXP];
#pragma unroll
            for (int n = 0; n < NBW; ++n)
#pragma unroll
                for (int i = 0; i < NXP; ++i) {
#if SP3D_W16_ABLATE & 2
                    bw[n][i].mh = u32x4{0x3f803f80u + (unsigned)(jk + n), 0x3f803f80u, 0x3f803f80u + (unsigned)i, 0x3f803f80u};
                    bw[n][i].l = u32x2{0x3f803f80u, 0x3f803f80u};
#else
                    bw[n][i] = load_b(i, jk, n);
#endif
                }
            const int ya = (j == 0) ? 0 : ((j == 2) ? 2 : 1), yb = (j == 3) ? 3 : ((j == 2) ? 1 : 2);
            const int za = (k == 0) ? 0 : ((k == 2) ? 2 : 1), zb = (k == 3) ? 3 : ((k == 2) ? 1 : 2);
            const float sy = (j == 1) ? 1.0f : -1.0f, sz = (k == 1) ? 1.0f : -1.0f;
            const float *r00 = rb + (za * W16_RY + ya) * W16_ROW, *r10 = rb + (za * W16_RY + yb) * W16_ROW;
            const float *r01 = rb + (zb * W16_RY + ya) * W16_ROW, *r11 = rb + (zb * W16_RY + yb) * W16_ROW;
            float g[4][4];
#pragma unroll
            for (int xi = 0; xi < 4; ++xi) {
#if SP3D_W16_ABLATE & 8
                const float f0 = __int_as_float(0x3f800000 + jk + xi), f1 = __int_as_float(0x3f900000 + lane);
                const float4 v00 = make_float4(f0, f1, f0, f1), v10 = make_float4(f1, f0, f1, f0), v01 = v00, v11 = v10;
                (void)r00; (void)r10; (void)r01; (void)r11;
#else
                const float4 v00 = *reinterpret_cast<const float4 *>(r00 + xi * W16_VS), v10 = *reinterpret_cast<const float4 *>(r10 + xi * W16_VS);
                const float4 v01 = *reinterpret_cast<const float4 *>(r01 + xi * W16_VS), v11 = *reinterpret_cast<const float4 *>(r11 + xi * W16_VS);
#endif
                g[xi][0] = fmaf(sz, fmaf(sy, v11.x, v01.x), fmaf(sy, v10.x, v00.x));
                g[xi][1] = fmaf(sz, fmaf(sy, v11.y, v01.y), fmaf(sy, v10.y, v00.y));
                g[xi][2] = fmaf(sz, fmaf(sy, v11.z, v01.z), fmaf(sy, v10.z, v00.z));
                g[xi][3] = fmaf(sz, fmaf(sy, v11.w, v01.w), fmaf(sy, v10.w, v00.w));
            }
            float cyz[4];
#pragma unroll
            for (int bc = 0; bc < 4; ++bc) {
                const int bb = bc >> 1, c2 = bc & 1;
                const float cy = bb == 0 ? (j < 3 ? 1.0f : 0.0f) : (j == 0 ? 0.0f : (j == 1 ? 1.0f : -1.0f));
                const float cz = c2 == 0 ? (k < 3 ? 1.0f : 0.0f) : (k == 0 ? 0.0f : (k == 1 ? 1.0f : -1.0f));
                cyz[bc] = cy * cz;
            }
            f32x4 M0[NBW], M1[NBW];
#pragma unroll
            for (int n = 0; n < NBW; ++n) { M0[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; M1[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float av[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    av[kk] = XD ? g[i][kk]
                                : ((i == 1) ? g[1][kk] + g[2][kk] : ((i == 3) ? g[3][kk] - g[1][kk] : g[wf_ta(i)][kk] - g[wf_tb(i)][kk]));
                const unsigned hi01 = pack_bf16(av[0], av[1]), hi23 = pack_bf16(av[2], av[3]);
#if SP3D_W16_ABLATE & 4
                const unsigned mid01 = hi01, mid23 = hi23, lo01 = hi01, lo23 = hi23;
#else
                const float r0 = av[0] - bf16_lo(hi01), r1 = av[1] - bf16_hi(hi01), r2 = av[2] - bf16_lo(hi23), r3 = av[3] - bf16_hi(hi23);
                const unsigned mid01 = pack_bf16(r0, r1), mid23 = pack_bf16(r2, r3);
                const unsigned lo01 = pack_bf16(r0 - bf16_lo(mid01), r1 - bf16_hi(mid01));
                const unsigned lo23 = pack_bf16(r2 - bf16_lo(mid23), r3 - bf16_hi(mid23));
#endif
                const u32x4 Qhh = {hi01, hi23, hi01, hi23}, Qmm = {mid01, mid23, mid01, mid23}, Qlh = {lo01, lo23, hi01, hi23};
                if (XD) {
                    // g[i] is tap i of output x and tap i - 1 of output x + 1: the same split operand against two records
#pragma unroll
                    for (int n = 0; n < NBW; ++n)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int dx = i - e;
                            if (dx < 0 || dx > 2) continue;
                            const WfB &w = bw[n][dx < NXP ? dx : 0];
                            const u32x4 Bmh = w.mh;
                            const u32x4 Bhl = {w.mh.z, w.mh.w, w.l.x, w.l.y};
                            f32x4 &M = e ? M1[n] : M0[n];
                            M = mfma16_bf16(Qhh, Bmh, M);
                            M = mfma16_bf16(Qmm, Bmh, M);
                            M = mfma16_bf16(Qlh, Bhl, M);
                        }
                    continue;
                }
#pragma unroll
                for (int n = 0; n < NBW; ++n) {
                    const WfB &w = bw[n][i < NXP ? i : 0];
                    const u32x4 Bmh = w.mh;
                    const u32x4 Bhl = {w.mh.z, w.mh.w, w.l.x, w.l.y};
#if SP3D_W16_ABLATE & 1
                    {   // no matrix instructions: keep every operand alive with one integer op each
                        const unsigned z = (Qhh.x ^ Bmh.x) + (Qmm.y ^ Bmh.z) + (Qlh.x ^ Bhl.w) + (Qlh.z ^ Bhl.y);
                        M0[n].x += __uint_as_float(z & 0x3fffffffu);
                        M1[n].y += __uint_as_float((z >> 1) & 0x3fffffffu);
                        continue;
                    }
#endif
                    if (i < 3) {
                        M0[n] = mfma16_bf16(Qhh, Bmh, M0[n]);
                        M0[n] = mfma16_bf16(Qmm, Bmh, M0[n]);
                        M0[n] = mfma16_bf16(Qlh, Bhl, M0[n]);
                    }
                    if (i == 1 || i == 3) {
                        M1[n] = mfma16_bf16(Qhh, Bmh, M1[n]);
                        M1[n] = mfma16_bf16(Qmm, Bmh, M1[n]);
                        M1[n] = mfma16_bf16(Qlh, Bhl, M1[n]);
                    }
                    if (i == 2) {
                        const u32x4 nmh = Bmh ^ 0x80008000u, nhl = Bhl ^ 0x80008000u;
                        M1[n] = mfma16_bf16(Qhh, nmh, M1[n]);
                        M1[n] = mfma16_bf16(Qmm, nmh, M1[n]);
                        M1[n] = mfma16_bf16(Qlh, nhl, M1[n]);
                    }
                }
            }
            // the coefficients are 0 or +-1 and wave-uniform; multiplying by the zeros costs less than branching or
            // selecting around them on accumulators this small
#pragma unroll
            for (int n = 0; n < NBW; ++n)
#pragma unroll
                for (int bc = 0; bc < 4; ++bc) {
#if defined(SP3D_NO_PK) || defined(SP3D_W16_SCALAR_ACC)
                    for (int e = 0; e < 4; ++e) {     // one v_fma_f32 per component instead of v_pk_fma_f32 pairs
                        acc[bc][n][e] = fmaf(M0[n][e], cyz[bc], acc[bc][n][e]);
                        acc[4 + bc][n][e] = fmaf(M1[n][e], cyz[bc], acc[4 + bc][n][e]);
                    }
#else
                    const f32x4 cv = {cyz[bc], cyz[bc], cyz[bc], cyz[bc]};
                    acc[bc][n] = __builtin_elementwise_fma(M0[n], cv, acc[bc][n]);
                    acc[4 + bc][n] = __builtin_elementwise_fma(M1[n], cv, acc[4 + bc][n]);
#endif
                }
        }
    }

    if (SKIP) {
        constexpr int CS = 32;
        static_assert(!SKIP || KS * 16 == CS, "one skip chunk per channel group");
        // the lane's coordinates are derived again here, from a copy the compiler cannot trace: what it would otherwise carry
        // through the main loop for this block costs that loop three spilled registers (252 + these)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int stl = ln & 15, sq = ln >> 4;
        // rows first: voxels outside the volume (edge blocks) read a clamped address, their outputs are never stored
        const float *xsb = xs + (int64_t)b * X * Y * Z * CS + 16 * kg + 4 * sq;
        float4 sx[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int xo = min(ox0 + 2 * (stl & 3) + (a >> 2), X - 1), yo = min(oy0 + 2 * (stl >> 2) + ((a >> 1) & 1), Y - 1);
            const int zo = min(oz0 + (a & 1), Z - 1);
            sx[a] = *reinterpret_cast<const float4 *>(xsb + ((xo * Y + yo) * Z + zo) * CS);
        }
        WfB sw[NBW];
#pragma unroll
        for (int n = 0; n < NBW; ++n) {
            const unsigned *r = WS + ((kg * 4 + sq) * O + (ow * NBW + n) * 16 + stl) * 6;
            sw[n].mh = *reinterpret_cast<const u32x4_a8 *>(r);
            sw[n].l = *reinterpret_cast<const u32x2_a8 *>(r + 4);
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const u32x6 p = split3_pieces(sx[a]);           // [lo01 lo23 hi01 hi23 mid01 mid23]
            const u32x4 Qlh = split3_q0(p), Qhh = {p[2], p[3], p[2], p[3]}, Qmm = {p[4], p[5], p[4], p[5]};
#pragma unroll
            for (int n = 0; n < NBW; ++n) {
                const u32x4 Bmh = sw[n].mh;
                const u32x4 Bhl = {sw[n].mh.z, sw[n].mh.w, sw[n].l.x, sw[n].l.y};
                acc[a][n] = mfma16_bf16(Qhh, Bmh, acc[a][n]);
                acc[a][n] = mfma16_bf16(Qmm, Bmh, acc[a][n]);
                acc[a][n] = mfma16_bf16(Qlh, Bhl, acc[a][n]);
            }
        }
    }

    if (KS > 1) {                                   // partial sums of channel groups 1.. -> group 0, through LDS
        __syncthreads();                            // every region has been read for the last time
        f32x4 *red = reinterpret_cast<f32x4 *>(lds);
        if (kg > 0) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int n = 0; n < NBW; ++n) red[(((kg - 1) * NOW + ow) * 8 * NBW + a * NBW + n) * 64 + lane] = acc[a][n];
        }
        __syncthreads();
        if (kg > 0) return;
#pragma unroll
        for (int g2 = 1; g2 < KS; ++g2)
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int n = 0; n < NBW; ++n) acc[a][n] += red[(((g2 - 1) * NOW + ow) * 8 * NBW + a * NBW + n) * 64 + lane];
    }

    // D of the 16x16 MFMA: lane (col = lane & 15, group = lane >> 4) holds tiles 4*group + v, output 16*nb + col
    if (ox0 + 8 <= X && oy0 + 8 <= Y && oz0 + 2 <= Z) {
        // interior block (every block of a 40x40x10 or 32^3 grid): one per-lane base address, compile-time offsets, no bounds
        // branch per element (64 of them cost ~750 instructions per lane, and kept the residual loads apart)
#pragma unroll
        for (int n = 0; n < NBW; ++n) {
            const int o = (ow * NBW + n) * 16 + tl;
            const float sh = shift[o];
            const int64_t obase = ((((int64_t)b * X + ox0) * Y + oy0) * Z + oz0) * O + o;
            int off[4];                                                    // tile 4 q + v: (rx, ry) = (v, q)
#pragma unroll
            for (int v = 0; v < 4; ++v) off[v] = ((2 * v * Y + 2 * q) * Z) * O;
            float rv[8][4];
            if (MODE >= 2) {
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        rv[a][v] = res[obase + off[v] + (((a >> 2) * Y + ((a >> 1) & 1)) * Z + (a & 1)) * O];
            }
            float pm[4] = {0.0f, 0.0f, 0.0f, 0.0f};                        // POOL: the running maximum of tile 4 q + v
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float val = acc[a][n][v] + sh;
                    if (MODE == 2) val += rv[a][v];
                    if (MODE >= 1) val = SKIP ? relu_keep_nan(val) : fmaxf(val, 0.0f);
                    if (MODE == 3) val += rv[a][v];
                    y[obase + off[v] + (((a >> 2) * Y + ((a >> 1) & 1)) * Z + (a & 1)) * O] = val;
                    if (POOL) pm[v] = (a == 0) ? val : ((val > pm[v] || val != val) ? val : pm[v]);
                }
            if (POOL) {
                static_assert(!POOL || (SKIP && MODE == 1), "the pooled form exists for the folded skip only");
                const int XP = X >> 1, YP = Y >> 1, ZP = Z >> 1;
                float *yp = y + (int64_t)B * X * Y * Z * O;
                const int64_t pbase = ((((int64_t)b * XP + (ox0 >> 1)) * YP + (oy0 >> 1) + q) * ZP + (oz0 >> 1)) * O + o;
#pragma unroll
                for (int v = 0; v < 4; ++v) yp[pbase + (int64_t)v * YP * ZP * O] = pm[v];
            }
        }
        return;
    }
#pragma unroll
    for (int n = 0; n < NBW; ++n) {
        const int o = (ow * NBW + n) * 16 + tl;
        const float sh = shift[o];
        // residual values first, all 32 loads of this output group in flight at once: with the load inside the bounds
        // branch below the compiler emitted branch -> load -> s_waitcnt vmcnt(0) -> store per element, 64 dependent round
        // trips per lane (MODE 2 cost 8.7 us more than MODE 1 at (4,64,40,40,10)).  The address of an element outside the
        // volume is clamped into it (never stored), so the loads need no predicate.
        float rv[8][4];
        if (MODE >= 2) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int tile = 4 * q + v;
                    const int rx = tile & 3, ry = tile >> 2;
                    const int xo = min(ox0 + 2 * rx + (a >> 2), X - 1), yo = min(oy0 + 2 * ry + ((a >> 1) & 1), Y - 1);
                    const int zo = min(oz0 + (a & 1), Z - 1);
                    rv[a][v] = res[((((int64_t)b * X + xo) * Y + yo) * Z + zo) * O + o];
                }
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int tile = 4 * q + v;
                const int rx = tile & 3, ry = tile >> 2;
                const int xo = ox0 + 2 * rx + (a >> 2), yo = oy0 + 2 * ry + ((a >> 1) & 1), zo = oz0 + (a & 1);
                if (xo < X && yo < Y && zo < Z) {
                    const int64_t idx = ((((int64_t)b * X + xo) * Y + yo) * Z + zo) * O + o;
                    float val = acc[a][n][v] + sh;
                    if (MODE == 2) val += rv[a][v];
                    if (MODE >= 1) val = SKIP ? relu_keep_nan(val) : fmaxf(val, 0.0f);
                    if (MODE == 3) val += rv[a][v];
                    y[idx] = val;
                }
            }
        }
    }
}

} // namespace sp3d

using namespace sp3d;

// the checks the four entries share: x, weights, y, shift and (mode >= 2) the residual; `supported` is the entry's own
static int wino_fused_check(const void *x, const void *U, const void *y, const void *shift, const void *residual, int mode, int B,
                            int X, int Y, int Z, bool supported, const Conv3Grid &g)
{
    return conv3_check(B, X, Y, Z, mode, x && U && y && shift && (mode < 2 || residual), supported, g.blocks <= 0x7fffffff);
}

extern "C" int sp3d_wino_fused(const float *x, const float *U, float *y, const float *shift, const float *residual, int mode,
                               int B, int X, int Y, int Z, int C, int O, void *stream)
{
    const Conv3Grid g = conv3_grid(B, X, Y, Z, 8, 8, 4);
    if (const int rc = wino_fused_check(x, U, y, shift, residual, mode, B, X, Y, Z, O == 32 && (C == 16 || C == 32), g)) return rc;
    auto launch = [&](auto c, auto m) {
        hipLaunchKernelGGL((wino_fused_kernel<decltype(c)::value, decltype(m)::value>), dim3((unsigned)g.blocks), dim3(64), 0,
                           (hipStream_t)stream, x, U, y, shift, residual, B, X, Y, Z, g.NBX, g.NBY, g.NBZ);
    };
    with_mode(mode, [&](auto m) { if (C == 16) launch(int_c<16>{}, m); else launch(int_c<32>{}, m); });
    return launch_status();
}

extern "C" int sp3d_debug_wino_fused_timeline(void *dev_buffer)
{
#ifdef SP3D_WF_TIMELINE
    unsigned long long *p = (unsigned long long *)dev_buffer;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(sp3d::g_wf_tl), &p, sizeof(p));
#else
    (void)dev_buffer;
    return SP3D_EUNSUPPORTED;
#endif
}

extern "C" int sp3d_wino_fused_split(const float *x, const void *U3, float *y, const float *shift, const float *residual, int mode,
                                     int B, int X, int Y, int Z, int C, int O, void *stream)
{
    const Conv3Grid g = conv3_grid(B, X, Y, Z, 8, 8, 4);
    const bool supported = O == 32 && (C == 16 || C == 32) && !(reinterpret_cast<uintptr_t>(U3) & 7);
    if (const int rc = wino_fused_check(x, U3, y, shift, residual, mode, B, X, Y, Z, supported, g)) return rc;
    auto launch = [&](auto c, auto m) {
        hipLaunchKernelGGL((wino_fused3_kernel<decltype(c)::value, decltype(m)::value>), dim3((unsigned)g.blocks), dim3(64), 0,
                           (hipStream_t)stream, x, reinterpret_cast<const unsigned *>(U3), y, shift, residual, B, X, Y, Z, g.NBX,
                           g.NBY, g.NBZ);
    };
    with_mode(mode, [&](auto m) { if (C == 16) launch(int_c<16>{}, m); else launch(int_c<32>{}, m); });
    return launch_status();
}

// waves per block of wino_fused16_kernel: two output groups x two input-channel groups of one wave each (2 waves per SIMD
// resident): best of the {1,2,4} x {1,2} configurations measured at (4,64,40,40,10) / (4,32,40,40,10) / (8,64,32,32,32) in
// round 2; the others are no longer instantiated
constexpr int W16_NBW = 2, W16_KS = 2;

extern "C" int sp3d_wino_fused_split64(const float *x, const void *U3, float *y, const float *shift, const float *residual,
                                       int mode, int B, int X, int Y, int Z, int C, int O, void *stream)
{
    const Conv3Grid g = conv3_grid(B, X, Y, Z, 8, 8, 2);
    // SP3D_CONV3_WINO_YZ on the mode: U3 holds the 48-point records, the kernel convolves directly along x.  A negative mode
    // stays negative without the bit, so it is refused as before
    const bool yz = mode >= 0 && (mode & SP3D_CONV3_WINO_YZ);
    if (yz) mode &= ~SP3D_CONV3_WINO_YZ;
    const bool supported = O == 64 && (C == 32 || C == 64) && !(reinterpret_cast<uintptr_t>(U3) & 7);
    if (const int rc = wino_fused_check(x, U3, y, shift, residual, mode, B, X, Y, Z, supported, g)) return rc;
    auto launch = [&](auto c, auto m, auto xd) {
        hipLaunchKernelGGL((wino_fused16_kernel<decltype(c)::value, decltype(m)::value, W16_NBW, W16_KS, false, decltype(xd)::value>),
                           dim3((unsigned)g.blocks), dim3(64 * (4 / W16_NBW) * W16_KS), 0, (hipStream_t)stream, x,
                           reinterpret_cast<const unsigned *>(U3), y, shift, residual, B, X, Y, Z, g.NBX, g.NBY, g.NBZ,
                           (const float *)nullptr, (const unsigned *)nullptr);
    };
    with_mode(mode, [&](auto m) {
        if (yz) { if (C == 32) launch(int_c<32>{}, m, std::true_type{}); else launch(int_c<64>{}, m, std::true_type{}); }
        else { if (C == 32) launch(int_c<32>{}, m, std::false_type{}); else launch(int_c<64>{}, m, std::false_type{}); }
    });
    return launch_status();
}

extern "C" int sp3d_wino_fused_split64_skip(const float *x, const void *U3, float *y, const float *shift, const float *xs,
                                            const void *WS, int B, int X, int Y, int Z, int C, int O, int CS, void *stream)
{
    const Conv3Grid g = conv3_grid(B, X, Y, Z, 8, 8, 2);
    // this entry has no mode: SP3D_CONV3_WINO_YZ rides on the skip width (U3 = the 48-point records; WS is one point either way)
    const bool yz = CS >= 0 && (CS & SP3D_CONV3_WINO_YZ);
    if (yz) CS &= ~SP3D_CONV3_WINO_YZ;
    // ... and so does SP3D_CONV3_POOL2X (the pooled tensor behind y).  The pooled form has no edge-block epilogue: a grid that
    // is not whole 8x8x2 blocks is refused before any launch
    const bool pool = CS >= 0 && (CS & SP3D_CONV3_POOL2X);
    if (pool) CS &= ~SP3D_CONV3_POOL2X;
    const bool whole = X % 8 == 0 && Y % 8 == 0 && Z % 2 == 0;
    const bool supported = O == 64 && C == 64 && CS == 32 && (!pool || whole) &&
                           !((reinterpret_cast<uintptr_t>(U3) | reinterpret_cast<uintptr_t>(WS)) & 7) &&
                           !(reinterpret_cast<uintptr_t>(xs) & 15);
    // (the kernel's 32-bit offsets inside a sample of xs)
    const bool in_range = (int64_t)X * Y * Z * CS <= 0x7fffffff && g.blocks <= 0x7fffffff;
    if (const int rc = conv3_check(B, X, Y, Z, 1, x && U3 && y && shift && xs && WS, supported, in_range)) return rc;
    auto launch = [&](auto xd, auto pl) {
        hipLaunchKernelGGL((wino_fused16_kernel<64, 1, W16_NBW, W16_KS, true, decltype(xd)::value, decltype(pl)::value>),
                           dim3((unsigned)g.blocks), dim3(64 * (4 / W16_NBW) * W16_KS), 0, (hipStream_t)stream, x,
                           reinterpret_cast<const unsigned *>(U3), y, shift, (const float *)nullptr, B, X, Y, Z, g.NBX, g.NBY, g.NBZ, xs,
                           reinterpret_cast<const unsigned *>(WS));
    };
    if (pool) { if (yz) launch(std::true_type{}, std::true_type{}); else launch(std::false_type{}, std::true_type{}); }
    else { if (yz) launch(std::true_type{}, std::false_type{}); else launch(std::false_type{}, std::false_type{}); }
    return launch_status();
}
