// sp3d_unproject_bwd.hip - backward of the unprojection: the scatter kernels and their C entries.
//   unproject_bwd_kernel     planar layout: recomputes the forward value (clamp mask) and scatters
//                            g * w_tap with hardware fp32 atomics.
//   unproject_bwd2_kernel    channels-last gradient, one atomic per tap and 16 channels (needs the forward's pass mask)
//   unproject_bwd3_kernel    the same on dense grids: a block's taps merge in LDS first
//   fixed_to_float_kernel    the deterministic forms accumulate in 64-bit fixed point; this converts back
// The one-channel backward is in sp3d_unproject_one.hip.
#include <type_traits>

#include "sp3d_unproject_pipe.h"

namespace sp3d {

// ------------------------------------------------------------------------------------------
// backward: lane = voxel, planar layout.  Pass 1 recomputes the pre-clamp forward value (the
// clamp mask: grad flows where 0 <= pre <= 1, torch.clamp backward), pass 2 scatters.
// ------------------------------------------------------------------------------------------
template <int JC>
__global__ __launch_bounds__(TILE) void unproject_bwd_kernel(Views hm, const float *__restrict__ cam,
                                                            const float *__restrict__ centers,
                                                            const uint8_t *__restrict__ valid,
                                                            const float *__restrict__ grad_cubes, ViewsMut ghm,
                                                            Geom g)
{
    const int b = blockIdx.y;
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int n = blockIdx.x * TILE + threadIdx.x;
    if (n >= g.N || !valid[b]) return;
    const int vx = n / g.YZ, rem = n - vx * g.YZ, vy = rem / g.Z, vz = rem - vy * g.Z;
    const float x = linspace_at(g.Lx, g.X, vx) + centers[3 * b + 0];
    const float y = linspace_at(g.Ly, g.Y, vy) + centers[3 * b + 1];
    const float z = linspace_at(g.Lz, g.Z, vz) + centers[3 * b + 2];
    const float W_in = (float)g.W_in, H_in = (float)g.H_in;
    const size_t plane = (size_t)g.h * g.w;
    const float *gc = grad_cubes + (size_t)b * g.J * g.N + n;
    for (int j0 = 0; j0 < g.J; j0 += JC) {
        float acc[JC];
#pragma unroll
        for (int k = 0; k < JC; ++k) acc[k] = 0.0f;
        float cnt = 0.0f;
        bool bad = false;
        for (int c = 0; c < g.V; ++c) {
            const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
            float ix, iy;
            const bool bound = sample_pos(cm, x, y, z, g.w, g.h, W_in, H_in, ix, iy);
            cnt += bound ? 1.0f : 0.0f;
            if (ix != ix || iy != iy) { bad = true; continue; }
            if (!bound) continue;
            const Bilin bl = bilin(ix, iy);
            const bool x0ok = bl.x0 >= 0 && bl.x0 <= g.w - 1, x1ok = bl.x0 + 1 >= 0 && bl.x0 + 1 <= g.w - 1;
            const bool y0ok = bl.y0 >= 0 && bl.y0 <= g.h - 1, y1ok = bl.y0 + 1 >= 0 && bl.y0 + 1 <= g.h - 1;
            const float *base = hm.p[c] + ((size_t)bs * g.J + j0) * plane + (ptrdiff_t)bl.y0 * g.w + bl.x0;
#pragma unroll
            for (int k = 0; k < JC; ++k) {
                if (j0 + k < g.J) {
                    const float *pl = base + (size_t)k * plane;
                    const float t00 = (x0ok && y0ok) ? pl[0] : 0.0f;
                    const float t10 = (x1ok && y0ok) ? pl[1] : 0.0f;
                    const float t01 = (x0ok && y1ok) ? pl[g.w] : 0.0f;
                    const float t11 = (x1ok && y1ok) ? pl[g.w + 1] : 0.0f;
                    float v = t00 * bl.wnw;
                    v = fmaf(t10, bl.wne, v);
                    v = fmaf(t01, bl.wsw, v);
                    v = fmaf(t11, bl.wse, v);
                    acc[k] = acc[k] + v;
                }
            }
        }
        if (bad) continue;
        const float den = cnt + 1e-6f;
        float gs[JC];
        bool anyg = false;
#pragma unroll
        for (int k = 0; k < JC; ++k) {
            gs[k] = 0.0f;
            if (j0 + k < g.J) {
                const float pre = acc[k] / den;
                if (pre >= 0.0f && pre <= 1.0f) {
                    gs[k] = gc[(size_t)(j0 + k) * g.N] / den;
                    anyg = anyg || (gs[k] != 0.0f);
                }
            }
        }
        if (!anyg) continue;
        for (int c = 0; c < g.V; ++c) {
            const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
            float ix, iy;
            const bool bound = sample_pos(cm, x, y, z, g.w, g.h, W_in, H_in, ix, iy);
            if (!bound) continue;
            const Bilin bl = bilin(ix, iy);
            const bool x0ok = bl.x0 >= 0 && bl.x0 <= g.w - 1, x1ok = bl.x0 + 1 >= 0 && bl.x0 + 1 <= g.w - 1;
            const bool y0ok = bl.y0 >= 0 && bl.y0 <= g.h - 1, y1ok = bl.y0 + 1 >= 0 && bl.y0 + 1 <= g.h - 1;
            float *base = ghm.p[c] + ((size_t)bs * g.J + j0) * plane + (ptrdiff_t)bl.y0 * g.w + bl.x0;
#pragma unroll
            for (int k = 0; k < JC; ++k) {
                if (j0 + k < g.J && gs[k] != 0.0f) {
                    float *pl = base + (size_t)k * plane;
                    if (x0ok && y0ok) unsafeAtomicAdd(pl, gs[k] * bl.wnw);
                    if (x1ok && y0ok) unsafeAtomicAdd(pl + 1, gs[k] * bl.wne);
                    if (x0ok && y1ok) unsafeAtomicAdd(pl + g.w, gs[k] * bl.wsw);
                    if (x1ok && y1ok) unsafeAtomicAdd(pl + g.w + 1, gs[k] * bl.wse);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// backward, line-coalesced scatter ("bwd2").  Needs the pass mask written by the forward pipe kernel,
// so no heat-map is re-read.  L2 fp32 atomics are one transaction per (instruction, cache line): 64
// scattered lanes run at 21 G atomics/s, 16 lanes on the 16 channels of one 64-B pixel at 325 G/s
// (tools/atomic_bench.hip).  Hence: gradients accumulate into a channels-last (V,B,h,w,16) buffer and
// the scatter maps lane = (voxel-of-4, channel): one atomic instruction = 4 pixels x 16 channels.
//   P1   lane = voxel: sample records of every view -> LDS (same code as the forward kernel)
//   load grad tile (J rows of 64 voxels, coalesced) -> LDS, pass mask / view masks per voxel -> LDS
//   S    lane = (v4, ch): for its 16 voxels, g = pass ? grad / den : 0, then per bound view 4 atomics
// ------------------------------------------------------------------------------------------
// DET: accumulate in 64-bit FIXED POINT (value * *scale, rounded to nearest) with integer atomics.  Integer addition is
// associative, so the result does not depend on the order in which the hardware retires the atomics: bit-identical
// run to run (what SURVEY.md §5 asks for, since the reference's grid_sampler_2d_backward is order-dependent too);
// sp3d_fixed_to_float converts back.  *scale = 2^k chosen by the caller from max|grad| so that 2^40 steps span it.
// PS: pixel stride of the gradient buffer in elements.  PS = JP is the packed form above.  PS = 32 > JP is one channel group of
// SP3D_SCATTER_WIDE (17..32 joints, a pixel is 32 elements): the launch scatters g.J <= JP channels of a (P, J, X, Y, Z)
// gradient whose cube stride is g.sB, into the JP channels that start at the base pointer it is given; everything indexed
// by channel (loops, LDS tile) keeps JP, everything that steps between pixels takes PS.
template <int JP, bool XCD, bool DET = false, int PS = JP>
__global__ __launch_bounds__(64) void unproject_bwd2_kernel(const float *__restrict__ cam,
                                                           const float *__restrict__ centers,
                                                           const uint8_t *__restrict__ valid,
                                                           const float *__restrict__ grad_cubes,
                                                           const uint16_t *__restrict__ pass_mask,
                                                           void *__restrict__ grad_packed_, size_t view_stride,
                                                           Geom g, int tiles_per_sample, const float *__restrict__ scale_p)
{
    using ACC = typename std::conditional<DET, unsigned long long, float>::type;
    ACC *grad_packed = reinterpret_cast<ACC *>(grad_packed_);
    const double scale = DET ? (double)*scale_p : 1.0;
    auto add = [&](ACC *p, float val) {
        if constexpr (DET) atomicAdd(p, (unsigned long long)__double2ll_rn((double)val * scale));
        else unsafeAtomicAdd(p, val);
    };
    extern __shared__ __attribute__((aligned(16))) float bsm[];
    float *rec = bsm;                                  // [V][5][64]
    int *reci = reinterpret_cast<int *>(rec);
    float *gt = bsm + g.V * 320;                       // [JP][64] gradient tile (0 where masked / beyond J)
    uint32_t *vm = reinterpret_cast<uint32_t *>(gt + JP * 64);   // [64] view bits per voxel (bit 31: NaN)
    int b, tile;
    if (XCD) {
        if (!xcd_map(blockIdx.x, g.B, tiles_per_sample, g.xcd_chunk, b, tile)) return;
    } else {
        b = blockIdx.x / tiles_per_sample;
        tile = blockIdx.x - b * tiles_per_sample;
    }
    const int n0 = tile * 64;
    if (n0 >= g.N || !valid[b]) return;
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int lane = threadIdx.x;
    const int nvox = min(64, g.N - n0);
    const bool inb = lane < nvox;
    const int n = n0 + (inb ? lane : 0);
    int vx, rem, vy, vz;
    udiv_magic((uint32_t)n, (uint32_t)g.YZ, g.magicYZ, vx, rem);
    udiv_magic((uint32_t)rem, (uint32_t)g.Z, g.magicZ, vy, vz);
    const float x = linspace_step(g.Lx, g.stepx, g.X, vx) + centers[3 * b + 0];
    const float y = linspace_step(g.Ly, g.stepy, g.Y, vy) + centers[3 * b + 1];
    const float z = linspace_step(g.Lz, g.stepz, g.Z, vz) + centers[3 * b + 2];
    uint32_t mymask = 0;
    for (int c = 0; c < g.V; ++c) {
        const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
        float ix, iy;
        bool isnan;
        const bool bound = sample_pos_fast(cm, x, y, z, g, ix, iy, isnan) && inb;
        if (bound) mymask |= (1u << c);
        if (isnan && inb) mymask |= 0x80000000u;
        const Rec r = make_record<PS>(bound && !isnan, isnan ? 0.0f : ix, isnan ? 0.0f : iy, g.w, g.h);
        const int base = c * 320 + lane;
        reci[base] = r.off;
        rec[base + 64] = r.w00; rec[base + 128] = r.w10; rec[base + 192] = r.w01; rec[base + 256] = r.w11;
    }
    // gradient tile: g = pass ? grad / den : 0     (autograd of project_layer.py:96-99)
    const uint32_t pm = inb ? (uint32_t)pass_mask[(size_t)b * g.N + n] : 0u;
    const float den = (float)__popc(mymask & 0x7fffffffu) + 1e-6f;
    const bool dead = (mymask & 0x80000000u) != 0 || (mymask & 0x7fffffffu) == 0;
    const float *gc = grad_cubes + (PS == JP ? (size_t)b * g.J * g.N : (size_t)b * g.sB) + n;
    bool any = false;
    // the J gradient loads of a voxel in flight together (n is a valid voxel for every lane): inside the per-channel condition
    // they were JP dependent round trips per wave
    float gl[JP];
#pragma unroll
    for (int j = 0; j < JP; ++j) gl[j] = (j < g.J) ? gc[(size_t)j * g.N] : 0.0f;
    const bool live = inb && !dead;
#pragma unroll
    for (int j = 0; j < JP; ++j) {
        float v = 0.0f;
        if (j < g.J && live && ((pm >> j) & 1u)) v = gl[j] / den;
        any = any || (v != 0.0f);
        gt[j * 64 + lane] = v;
    }
    vm[lane] = any ? (mymask & 0x7fffffffu) : 0u;      // voxels without gradient scatter nothing
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // scatter: lane = (v4, ch)
    const int v4 = lane >> 4, ch = lane & 15;
    if (ch >= JP) return;
    const size_t rowf = (size_t)g.w * PS;
    ACC *gbase = grad_packed + (size_t)bs * g.h * rowf + ch;
#pragma unroll 1
    for (int m = 0; m < 16; ++m) {
        const int v = 4 * m + v4;
        uint32_t views = vm[v];
        const float gv = gt[ch * 64 + v];
        while (views) {
            const int c = __ffs((int)views) - 1;
            views &= views - 1;
            const int rb = c * 320 + v;
            ACC *p = gbase + (size_t)c * view_stride + reci[rb];
            const float w00 = rec[rb + 64], w10 = rec[rb + 128], w01 = rec[rb + 192], w11 = rec[rb + 256];
            if (w00 != 0.0f) add(p, gv * w00);
            if (w10 != 0.0f) add(p + PS, gv * w10);
            if (w01 != 0.0f) add(p + rowf, gv * w01);
            if (w11 != 0.0f) add(p + rowf + PS, gv * w11);
        }
    }
}

// ------------------------------------------------------------------------------------------
// backward on DENSE grids (round 4, "bwd3"): a workgroup owns an 8x8x4 block of voxels and, per view, merges the block's tap
// gradients in an LDS patch of the heat-map gradient before they go to memory.
//
// What bounds the scatter (tools/global_atomic_bench.hip, profiles/r04_backward_kernels.md): memory atomics retire at
// ~20.7 G (instruction, 64-byte segment) pairs per second chip-wide - whatever the type (f32, u32, u64, f64, packed bf16),
// the scope, or how the segments of one instruction lie to each other; plain stores of the same segments are 4.6x
// faster.  bwd2 issues one segment per tap (4 per voxel and view).  On the 64^3 person cubes (31.7 mm pitch, ~1.7 heat-map
// pixels) the 1 024 taps of a block fall on ~180 distinct pixels of a ~18x12 rectangle: merged first, 4-5x fewer
// segments leave the CU.
// The merge cannot use fp32 LDS atomics: ds_add_f32 costs ~190 cycles per wave instruction per CU on gfx950, ds_add_u32 /
// ds_add_u64 cost 7 (tools/lds_atomic_bench.hip).  So the patch is 64-bit FIXED POINT: tap value * 2^k, rounded to
// nearest, with k from the block's largest |g| so that 2^50 steps span it (256 taps per pixel at most: no overflow); the
// patch sums are exact, and one rounding to fp32 happens when a pixel leaves (bwd2 rounds after every tap).  With the
// caller's global scale instead (DET) the flush adds the 64-bit sums to the fixed-point buffer with integer atomics:
// bit-identical to bwd2<DET>, run to run and to each other (integer addition is associative).
//   lane = voxel throughout (vz fastest).  gradient of the 16 channels in registers (one round trip: 16 loads in flight)
//   pass 1: project every view -> view mask / den, rectangle of the view's 2x2 tap blocks (LDS atomicMin/Max)
//   per view, per window of <= B3_PX pixels of the rectangle (almost always one): ds_add_u64 into patch[ch][pixel];
//   barrier; flush-and-clear, lanes = (pixel-of-4, channel): 64-byte segments, untouched pixels are skipped.
//   LDS: patch [JP][B3_PXS] int64 | rectangles [MAX_VIEWS][4] | block max           (33.5 KB: 4 workgroups per CU)
// ------------------------------------------------------------------------------------------
constexpr int B3_BX = 8, B3_BY = 8, B3_BZ = 4;
#ifndef SP3D_B3_PX
#define SP3D_B3_PX 256        // A/B on one box, us fp32 / deterministic: 128: 300 / 352, 192: 268 / 350, 256: 274 / 330, 384: 289 / 327, 512: 354 / 346
#endif
constexpr int B3_PX = SP3D_B3_PX;    // pixels of a patch window (a multiple of 32)
constexpr int B3_PXS = B3_PX + 4;    // plane stride (int64 words): == 4 mod 32, so the flush's (pixel-of-4, channel) lanes spread over the banks
#ifndef SP3D_B3_ABL
#define SP3D_B3_ABL 0            // measurement builds only: 1 no flush atomics, 2 no tap adds, 8 no view loop, 16 no gradient loads,
                                 // 32 no pass-1 projection, 64 no patch clear, 128 no divisions
#endif

// PS: pixel stride of the gradient buffer, as in unproject_bwd2_kernel (the patch and its flush lanes keep JP channels)
template <int JP, bool DET, int PS = JP>
__global__ __launch_bounds__(256, 4) void unproject_bwd3_kernel(const float *__restrict__ cam, const float *__restrict__ centers,
                                                            const uint8_t *__restrict__ valid,
                                                            const float *__restrict__ grad_cubes,
                                                            const uint16_t *__restrict__ pass_mask,
                                                            void *__restrict__ grad_acc_, size_t view_stride, Geom g,
                                                            int nbx, int nby, int nbz, const float *__restrict__ scale_p)
{
    using ACC = typename std::conditional<DET, unsigned long long, float>::type;
    ACC *grad_acc = reinterpret_cast<ACC *>(grad_acc_);
    extern __shared__ __attribute__((aligned(16))) unsigned long long psm3[];
    unsigned long long *patch = psm3;                                   // [JP][B3_PXS]
    int *rect = reinterpret_cast<int *>(patch + JP * B3_PXS);           // [MAX_VIEWS][4]: min x0, min y0, max x0 + 1, max y0 + 1
    uint32_t *bmax = reinterpret_cast<uint32_t *>(rect + 4 * SP3D_MAX_VIEWS);
    const int blocks_per_sample = nbx * nby * nbz;
    int b, blk;
    if (!xcd_map(blockIdx.x, g.B, blocks_per_sample, g.xcd_chunk, b, blk)) return;
    if (!valid[b]) return;
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int tid = threadIdx.x;
    const int bz = blk % nbz, by = (blk / nbz) % nby, bx = blk / (nbz * nby);
    const int vx = bx * B3_BX + (tid >> 5), vy = by * B3_BY + ((tid >> 2) & 7), vz = bz * B3_BZ + (tid & 3);
    const bool inb = vx < g.X && vy < g.Y && vz < g.Z;
    const int n = (min(vx, g.X - 1) * g.Y + min(vy, g.Y - 1)) * g.Z + min(vz, g.Z - 1);
    // gradient of this voxel, all channels: issued first, consumed after pass 1
    const float *gc = grad_cubes + (PS == JP ? (size_t)b * g.J * g.N : (size_t)b * g.sB) + n;
    float gq[JP];
#pragma unroll
    for (int j = 0; j < JP; ++j) gq[j] = (SP3D_B3_ABL & 16) ? (float)(j + tid) : gc[(size_t)min(j, g.J - 1) * g.N];
    const uint32_t pm = inb ? (uint32_t)pass_mask[(size_t)b * g.N + n] : 0u;
    if (!(SP3D_B3_ABL & 64))
    for (int e = tid; e < JP * B3_PXS; e += 256) patch[e] = 0ull;
    if (tid < 4 * SP3D_MAX_VIEWS) rect[tid] = (tid & 3) < 2 ? 0x7fffffff : -1;
    if (tid == 0) *bmax = 0u;
    __syncthreads();

    const float x = linspace_step(g.Lx, g.stepx, g.X, min(vx, g.X - 1)) + centers[3 * b + 0];
    const float y = linspace_step(g.Ly, g.stepy, g.Y, min(vy, g.Y - 1)) + centers[3 * b + 1];
    const float z = linspace_step(g.Lz, g.stepz, g.Z, min(vz, g.Z - 1)) + centers[3 * b + 2];
    uint32_t mymask = (SP3D_B3_ABL & 32) ? 31u : 0u;
    for (int c = 0; c < ((SP3D_B3_ABL & 32) ? 0 : g.V); ++c) {
        const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
        float ix, iy;
        bool isnan;
        const bool bound = sample_pos_fast(cm, x, y, z, g, ix, iy, isnan) && inb;
        if (bound) mymask |= (1u << c);
        if (isnan && inb) mymask |= 0x80000000u;
        const bool use = bound && !isnan;
        const RecPk r = make_record_pk(use, v2f{isnan ? 0.0f : ix, isnan ? 0.0f : iy}, g.w, g.h);
        // rectangle: reduce in the wave first (64 lanes on ONE LDS word serialise: 230 us of the kernel when every
        // lane issued its own atomicMin/Max)
        int lo_x = use ? r.x0 : 0x7fffffff, lo_y = use ? r.y0 : 0x7fffffff, hi_x = use ? r.x0 + 1 : -1, hi_y = use ? r.y0 + 1 : -1;
        for (int o = 32; o > 0; o >>= 1) {
            lo_x = min(lo_x, __shfl_xor(lo_x, o)); lo_y = min(lo_y, __shfl_xor(lo_y, o));
            hi_x = max(hi_x, __shfl_xor(hi_x, o)); hi_y = max(hi_y, __shfl_xor(hi_y, o));
        }
        if ((tid & 63) == 0 && hi_x >= 0) {
            atomicMin(&rect[4 * c + 0], lo_x); atomicMin(&rect[4 * c + 1], lo_y);
            atomicMax(&rect[4 * c + 2], hi_x); atomicMax(&rect[4 * c + 3], hi_y);
        }
    }
    // g = pass ? grad / den : 0     (autograd of project_layer.py:96-99)
    const float den = (float)__popc(mymask & 0x7fffffffu) + 1e-6f;
    const bool dead = (mymask & 0x80000000u) != 0 || (mymask & 0x7fffffffu) == 0;
    uint32_t amax = 0u;
#pragma unroll
    for (int j = 0; j < JP; ++j) {
        float v = 0.0f;
        if (j < g.J && inb && !dead && ((pm >> j) & 1u)) v = (SP3D_B3_ABL & 128) ? gq[j] * den : gq[j] / den;
        gq[j] = v;
        amax = max(amax, __float_as_uint(v) & 0x7fffffffu);
    }
    const bool any = amax != 0u;                       // voxels without gradient scatter nothing
    if (!DET) {
        for (int o = 32; o > 0; o >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, o));
        if ((tid & 63) == 0 && amax) atomicMax(bmax, amax);
    }
    __syncthreads();
    double scale, inv_scale = 1.0;
    bool nonfinite = false;     // uniform
    if (DET) {
        scale = (double)*scale_p;
    } else {
        const uint32_t m = *bmax;
        if (m == 0u) return;                           // no gradient anywhere in this block (uniform)
        if ((m >> 23) == 0xffu) {                      // Inf / NaN gradient in this block: no scale exists
            nonfinite = true;
            scale = 1.0;
        } else {
            const int k = min(50 - ((int)(m >> 23) - 126), 200);         // |g| < 2^(E - 126)  ->  |g| * 2^k < 2^50
            scale = __longlong_as_double((long long)(k + 1023) << 52);
            inv_scale = __longlong_as_double((long long)(1023 - k) << 52);
        }
    }
    if (SP3D_B3_ABL & 8) return;

    const size_t rowf = (size_t)g.w * PS;
#pragma unroll 1
    for (int c = 0; c < g.V; ++c) {
        const int rx0 = rect[4 * c + 0], ry0 = rect[4 * c + 1], rx1 = rect[4 * c + 2], ry1 = rect[4 * c + 3];
        if (rx1 < 0) continue;                          // nobody of this block sees view c (uniform)
        const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
        float ix, iy;
        bool isnan;
        const bool bound = sample_pos_fast(cm, x, y, z, g, ix, iy, isnan) && inb;
        const bool use = bound && !isnan;
        const RecPk r = make_record_pk(use, v2f{isnan ? 0.0f : ix, isnan ? 0.0f : iy}, g.w, g.h);
        const bool act = use && any;
        const float wts[4] = {r.wt.x, r.wt.y, r.wb.x, r.wb.y};
        ACC *gview = grad_acc + (size_t)c * view_stride + (size_t)bs * g.h * rowf;
        if (nonfinite) {
            // the block holds an Inf / NaN gradient: per-tap fp32 atomics straight to memory, as bwd2 adds them (the
            // non-finite value reaches exactly the pixels its voxel touches)
            if constexpr (!DET) {
                if (act) {
                    ACC *p0 = gview + ((size_t)r.y0 * g.w + r.x0) * PS;
#pragma unroll
                    for (int j = 0; j < JP; ++j) {
                        if (j >= g.J) break;
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (wts[t] != 0.0f) unsafeAtomicAdd(p0 + (size_t)(t >> 1) * rowf + (t & 1) * PS + j, gq[j] * wts[t]);
                    }
                }
            }
            continue;
        }
        // windows of the rectangle (one, unless the block's footprint in this view is unusually large)
        const int pw = rx1 - rx0 + 1, ph = ry1 - ry0 + 1;
        const int ww = min(pw, B3_PX), wh = min(ph, B3_PX / ww);
        const float rww = 1.0f / (float)ww;
#pragma unroll 1
        for (int wy0 = ry0; wy0 <= ry1; wy0 += wh) {
#pragma unroll 1
            for (int wx0 = rx0; wx0 <= rx1; wx0 += ww) {
                if (act && !(SP3D_B3_ABL & 2)) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int tx = r.x0 + (t & 1) - wx0, ty = r.y0 + (t >> 1) - wy0;
                        if (wts[t] == 0.0f || (unsigned)tx >= (unsigned)ww || (unsigned)ty >= (unsigned)wh) continue;
                        unsigned long long *pp = patch + ty * ww + tx;
                        // round-to-nearest-even of t * 2^k to int64 without a conversion sequence: the sum with 1.5 * 2^52
                        // holds the integer in its low mantissa bits (|t * 2^k| < 2^50); taking the constant's bit
                        // pattern off again touches only the high word.  == __double2ll_rn((double)t * scale) of bwd2<DET>.
#pragma unroll
                        for (int j = 0; j < JP; ++j) {
                            if (j >= g.J) break;                                    // uniform: the pad channels carry nothing (testing only the last three is 5 % slower)
                            const double d = __builtin_fma((double)(gq[j] * wts[t]), scale, 6755399441055744.0);
                            atomicAdd(pp + j * B3_PXS, (unsigned long long)__double_as_longlong(d) - 0x4338000000000000ull);
                        }
                    }
                }
                __syncthreads();
                // flush and clear: element e = (pixel, channel), 64 lanes = 4 pixels x 16 channels = 4 segments of 64 bytes
                const int nwx = min(ww, rx1 - wx0 + 1), nwy = min(wh, ry1 - wy0 + 1);
                const int nel = nwy * ww * 16;
                for (int e = tid; e < nel; e += 256) {
                    const int px = e >> 4, ch = e & 15;
                    if (ch >= JP) continue;
                    const long long val = (long long)patch[ch * B3_PXS + px];
                    if (val == 0) continue;
                    patch[ch * B3_PXS + px] = 0ull;
                    const int ty = (int)(((float)px + 0.5f) * rww), tx = px - ty * ww;
                    if (tx >= nwx || (SP3D_B3_ABL & 1)) continue;
                    ACC *dst = gview + ((size_t)(wy0 + ty) * g.w + (wx0 + tx)) * PS + ch;
                    if constexpr (DET) atomicAdd(dst, (unsigned long long)val);
                    else unsafeAtomicAdd(dst, (float)((double)val * inv_scale));
                }
                __syncthreads();
            }
        }
    }
}

__global__ __launch_bounds__(256) void fixed_to_float_kernel(const long long *__restrict__ acc, float *__restrict__ out,
                                                            const float *__restrict__ scale_p, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)((double)acc[i] / (double)*scale_p);
}

// channel stride 4, 8, 12 or 16 (validated) -> f(std::integral_constant<int, Jp>), whose ::value names a kernel instantiation
template <class F> static void with_jp(int Jp, F &&f)
{
    switch (Jp) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    default: return f(std::integral_constant<int, 16>{});
    }
}

} // namespace sp3d

using namespace sp3d;

extern "C" int sp3d_unproject_bwd_indexed(const float *const *hm_views, const float *cam, const int32_t *sample_of,
                                          const float *centers, const uint8_t *valid, const float *grad_cubes,
                                          float *const *grad_hm_views, int P, int V, int J, int h, int w, int X, int Y,
                                          int Z, const float *grid_size, int W_in, int H_in, void *stream)
{
    Geom g;
    int rc = make_geom(g, P, V, J, h, w, X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    if (!cam || !centers || !valid || !grad_cubes || !grad_hm_views) return SP3D_ENULL;
    g.sample_of = sample_of;
    Views v;
    rc = load_views(v, hm_views, V);
    if (rc) return rc;
    ViewsMut gv;
    for (int c = 0; c < SP3D_MAX_VIEWS; ++c) gv.p[c] = nullptr;
    for (int c = 0; c < V; ++c) {
        if (!grad_hm_views[c]) return SP3D_ENULL;
        gv.p[c] = grad_hm_views[c];
    }
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((g.N + TILE - 1) / TILE, P), block(TILE);
    if (J == 1)
        hipLaunchKernelGGL(unproject_bwd_kernel<1>, grid, block, 0, s, v, cam, centers, valid, grad_cubes, gv, g);
    else if (J <= 4)
        hipLaunchKernelGGL(unproject_bwd_kernel<4>, grid, block, 0, s, v, cam, centers, valid, grad_cubes, gv, g);
    else
        hipLaunchKernelGGL(unproject_bwd_kernel<16>, grid, block, 0, s, v, cam, centers, valid, grad_cubes, gv, g);
    return launch_status();
}

extern "C" int sp3d_unproject_bwd(const float *const *hm_views, const float *cam, const float *centers,
                                  const uint8_t *valid, const float *grad_cubes, float *const *grad_hm_views, int B,
                                  int V, int J, int h, int w, int X, int Y, int Z, const float *grid_size, int W_in,
                                  int H_in, void *stream)
{
    return sp3d_unproject_bwd_indexed(hm_views, cam, nullptr, centers, valid, grad_cubes, grad_hm_views, B, V, J, h, w,
                                      X, Y, Z, grid_size, W_in, H_in, stream);
}

// scatter: which kernel sp3d_unproject_bwd_packed[_det] launches - SP3D_SCATTER_AUTO (by voxel pitch), _PER_TAP (bwd2),
// _MERGE (bwd3).  A per-call argument: the library keeps no selector state (include/sp3d.h "no global state").
// | SP3D_SCATTER_WIDE: 17..32 joints in a 32-element pixel, as two channel groups - one launch each, like the forward
// (sp3d_unproject.hip, WIDE_PS).  Group 0 scatters channels 0-15 under mask plane 0 through the JP = 16 kernel; group 1
// scatters channels 16..J-1 under plane 1 through the kernel of width ceil4(J - 16): its gradient base lies 16 elements
// into the pixel, its grad_cubes 16 channel volumes further, its Geom has J - 16 channels.  Both read cubes at the stride
// of all J channels (Geom::sB) and step pixels by 32.  One scatter choice for both, so AUTO decides once.
static int bwd_packed_impl(const float *cam, const int32_t *sample_of, const float *centers, const uint8_t *valid,
                           const float *grad_cubes, const uint16_t *pass_mask, void *grad_acc, const float *scale, int B,
                           int P, int V, int J, int Jp, int h, int w, int X, int Y, int Z, const float *grid_size,
                           int W_in, int H_in, int scatter, void *stream)
{
    Geom g;
    int rc = make_geom(g, P, V, J, h, w, X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    if (B <= 0) return SP3D_EINVAL;
    const bool wide = (scatter & SP3D_SCATTER_WIDE) != 0;
    const int choice = scatter & 0xff;
    if ((scatter & ~(0xff | SP3D_SCATTER_WIDE)) != 0) return SP3D_EINVAL;
    if (choice != SP3D_SCATTER_AUTO && choice != SP3D_SCATTER_PER_TAP && choice != SP3D_SCATTER_MERGE) return SP3D_EINVAL;
    if (!cam || !centers || !valid || !grad_cubes || !pass_mask || !grad_acc) return SP3D_ENULL;
    if (w < 2 || h < 2) return SP3D_EUNSUPPORTED;
    // wide: the tap offset (y0 * w + x0) * 32 is a 32-bit int; the bound is the forward's (24-bit pixel indices)
    if (wide ? (Jp != WIDE_PS || J > WIDE_PS || (int64_t)h * w > (1 << 24)) : (Jp < J || (Jp & 3) || Jp > 16)) return SP3D_EUNSUPPORTED;
    g.sample_of = sample_of;
    const int tiles = (g.N + 63) / 64;
    const size_t view_stride = (size_t)B * h * w * Jp;
    // dense grids (the 64^3 person cubes at 31.7 mm: voxels ~1.7 heat-map pixels apart): block-wise LDS merge, bwd3.
    // The pixel pitch depends on the cameras (device data); what the host knows is the voxel pitch in mm: <= 50 mm.
    const bool dense = X >= 2 && Y >= 2 && Z >= 2 && (double)grid_size[0] / (X - 1) <= 50.0 &&
                       (double)grid_size[1] / (Y - 1) <= 50.0 && (double)grid_size[2] / (Z - 1) <= 50.0;
    const bool merge = choice == SP3D_SCATTER_MERGE || (choice == SP3D_SCATTER_AUTO && dense);
    const int nbx = (X + B3_BX - 1) / B3_BX, nby = (Y + B3_BY - 1) / B3_BY, nbz = (Z + B3_BZ - 1) / B3_BZ;
    // bwd3: the 16-byte z runs a block reads of the gradient volume share their 256-byte rows with the blocks above and
    // below: keep a whole z column of blocks on one XCD, back to back in dispatch order (chunk = nbz when a power of two)
    if (merge && (nbz & (nbz - 1)) == 0) g.xcd_chunk = nbz;
    const dim3 grid(xcd_grid_blocks(P, merge ? nbx * nby * nbz : tiles, g.xcd_chunk)), block(merge ? 256 : 64);
    hipStream_t s = (hipStream_t)stream;
    // one launch: `jp` channels (the kernel's width) starting at channel ch0 of the pixel and of the cubes, under mask plane pm
    auto launch = [&](auto jp, auto wd, auto det, const Geom &gg, int ch0, const uint16_t *pm) {
        constexpr int JP = decltype(jp)::value, PS = decltype(wd)::value ? WIDE_PS : JP;
        constexpr bool DET = decltype(det)::value;
        const size_t lds = merge ? (size_t)JP * B3_PXS * sizeof(unsigned long long) + (4 * SP3D_MAX_VIEWS + 4) * sizeof(int)
                                 : (size_t)(V * 320 + JP * 64 + 64) * sizeof(float);
        const float *gc = grad_cubes + (size_t)ch0 * g.N;
        void *acc = static_cast<char *>(grad_acc) + (size_t)ch0 * (DET ? sizeof(unsigned long long) : sizeof(float));
        if (merge)
            hipLaunchKernelGGL((unproject_bwd3_kernel<JP, DET, PS>), grid, block, lds, s, cam, centers, valid, gc, pm,
                               acc, view_stride, gg, nbx, nby, nbz, scale);
        else
            hipLaunchKernelGGL((unproject_bwd2_kernel<JP, true, DET, PS>), grid, block, lds, s, cam, centers, valid, gc,
                               pm, acc, view_stride, gg, tiles, scale);
    };
    const int groups = (wide && J > 16) ? 2 : 1;
    for (int k = 0; k < groups && !rc; ++k) {
        Geom gg = g;                                   // gg.sB stays J * N: the cube stride of grad_cubes
        if (wide) gg.J = k ? J - 16 : (J < 16 ? J : 16);
        const int width = wide ? (k ? (gg.J + 3) / 4 * 4 : 16) : Jp;
        const uint16_t *pm = pass_mask + (size_t)k * P * g.N;
        with_jp(width, [&](auto jp) {
            auto go = [&](auto wd) {
                if (scale) launch(jp, wd, std::true_type{}, gg, 16 * k, pm);
                else launch(jp, wd, std::false_type{}, gg, 16 * k, pm);
            };
            if (wide) go(std::true_type{});
            else go(std::false_type{});
        });
        rc = launch_status();
    }
    return rc;
}

extern "C" int sp3d_unproject_bwd_packed(const float *cam, const int32_t *sample_of, const float *centers,
                                         const uint8_t *valid, const float *grad_cubes, const uint16_t *pass_mask,
                                         float *grad_packed, int B, int P, int V, int J, int Jp, int h, int w, int X,
                                         int Y, int Z, const float *grid_size, int W_in, int H_in, int scatter,
                                         void *stream)
{
    return bwd_packed_impl(cam, sample_of, centers, valid, grad_cubes, pass_mask, grad_packed, nullptr, B, P, V, J, Jp, h, w,
                           X, Y, Z, grid_size, W_in, H_in, scatter, stream);
}

extern "C" int sp3d_unproject_bwd_packed_det(const float *cam, const int32_t *sample_of, const float *centers,
                                             const uint8_t *valid, const float *grad_cubes, const uint16_t *pass_mask,
                                             int64_t *grad_fixed, const float *scale, int B, int P, int V, int J, int Jp,
                                             int h, int w, int X, int Y, int Z, const float *grid_size, int W_in, int H_in,
                                             int scatter, void *stream)
{
    if (!scale) return SP3D_ENULL;
    return bwd_packed_impl(cam, sample_of, centers, valid, grad_cubes, pass_mask, grad_fixed, scale, B, P, V, J, Jp, h, w, X,
                           Y, Z, grid_size, W_in, H_in, scatter, stream);
}

extern "C" int sp3d_fixed_to_float(const int64_t *acc, float *out, const float *scale, int64_t n, void *stream)
{
    if (n <= 0) return SP3D_EINVAL;
    if (!acc || !out || !scale) return SP3D_ENULL;
    if ((n + 255) / 256 > 0x7fffffff) return SP3D_ERANGE;
    hipLaunchKernelGGL(fixed_to_float_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long *>(acc), out, scale, (size_t)n);
    return launch_status();
}
