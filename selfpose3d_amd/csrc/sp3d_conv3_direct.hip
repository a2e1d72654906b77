// sp3d_conv3_direct.hip - the direct (implicit-GEMM) 3x3x3 convolution of the full-resolution V2V layers in inference on
// the bf16 matrix pipe at fp32 accuracy: conv3_split_kernel, persistent producer / consumer workgroups, with or without
// the folded 1x1x1 skip projection, and its C entries.  No Winograd: see the comparison below.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sp3d.h"
#include "sp3d_conv3_host.h"
#include "sp3d_split.h"

namespace sp3d {

// ------------------------------------------------------------------------------------------
// Direct 3x3x3 convolution on the bf16 matrix pipe at fp32 accuracy (implicit GEMM, no Winograd).
// With exact three-piece splits a multiply costs 3 bf16 MFMA slots, and the bf16 pipe is 16x the fp32 one: the 2.25x
// multiplication saving of (x-folded) Winograd no longer pays for its operand transforms - the fused Winograd kernels
// (sp3d_wino_fused.hip) are VALU-bound (183 VALU instructions per 18 MFMAs, every step re-transforms and re-splits its
// operands).  Here an input value is split ONCE when its region is staged (pieces stored in LDS: 24 B per voxel and 4-channel group,
// [lo hi mid]), the A operand of tap (dx,dy,dz) is the staged record of the shifted voxel - read with a compile-time LDS
// offset, no VALU at all - and the accumulators ARE the outputs.  Per (tap, 32-voxel block): 3 LDS reads + 3 MFMAs
//     {lo,hi} x {bh,bl}  +  {hi,mid} x {bh,bh}  +  {hi,mid} x {bm,bm}      (A quads are consecutive registers)
// Block = 8x8x2 outputs (4 MFMA row blocks) x NB*32 output channels per wave, 8-channel chunks, region 10x10x4 voxels
// = 19.2 KB of LDS.  Weights: per (tap, chunk, lane half, output) one 24-byte record [mid hi lo] (conv_weights_split).
// ------------------------------------------------------------------------------------------
// Workgroup = 4 consumer waves + 4 producer waves (one of each per SIMD), persistent over output blocks of 16x8x4 voxels.
//   consumers (wave = z layer, 4 row blocks of 16x2 voxels x 32 outputs): per tap 8 ds_read_b128 + 3 global_load_dwordx4
//     + 12 matrix instructions, nothing else; operands one tap ahead, weights three taps ahead (across chunk boundaries);
//   producers: fetch the 18x10x6 region of the NEXT (block, 8-channel chunk) item, split it, write it to the other LDS
//     buffer.  They are separate waves because vmcnt is in-order: a consumer that had the region loads of the next chunk
//     in flight waited for them at its next weight wait (58 us of 207), and between workgroups nobody covered the first
//     chunk's latency.  One barrier per item.
// LDS per buffer: one plane per 4-channel group (lane half); a voxel is the two A operands ready to use, 8 dwords
// [lo hi | hi mid]; rows of 18 voxels (144 dwords), z planes of 10 rows + 4 dwords: with lane = (y = t & 7, z = t >> 3) the
// 16 lanes of a ds_read_b128 group sit on 16 distinct 4-bank slots (searched over row / plane pitches).
// A consumer wave owns 4 consecutive x of the block and ALL its (y,z): the operand of region voxel x' serves the taps
// dx = x' - x of every x it owns, so a (dy,dz) step reads 6 operands for 36 matrix instructions instead of 12 - the LDS
// (85 of its 128 B/clk with one operand read per tap and row block) was what the matrix pipe and the loader waves waited on.
constexpr int CD_BX = 16, CD_BY = 8, CD_BZ = 4;
constexpr int CD_RX = CD_BX + 2, CD_RY = CD_BY + 2, CD_RZ = CD_BZ + 2, CD_VOX = 8, CD_ROW = CD_RX * CD_VOX, CD_ZP = CD_RY * CD_ROW + 4;
constexpr int CD_PLANE = CD_RZ * CD_ZP;                                // 8 664 dwords
constexpr int CD_BUF = 2 * CD_PLANE;                                   // 17 328 dwords = 69 312 B per buffer
constexpr int CD_NV4 = CD_RX * CD_RY * CD_RZ * 2;                      // float4 per item: 2 160
constexpr int CD_PROD = 4;                                             // producer waves: one per SIMD
constexpr int CD_PER = (CD_NV4 + 64 * CD_PROD - 1) / (64 * CD_PROD);   // 9 float4 per producer lane
// buffer stride in dwords (17 408 = 69 632 B: the LDS layout the bank-conflict search was done for; CD_BUF rounded up to 68 x 256)
constexpr int CD_BUFS = ((CD_BUF / 4 + 63) / 64) * 256;
#ifndef SP3D_WG_ABLATE
#define SP3D_WG_ABLATE 0
#endif
struct CdRec { u32x4 hl, hh, mm; };                                    // weight record: B operands {bh,bl} {bh,bh} {bm,bm}


#ifdef SP3D_CD_TIMELINE
__device__ unsigned long long *g_cd_tl = nullptr;      // [wave 6][item 64][4] s_memtime stamps of workgroup 0
#define CD_STAMP(slot) do { __builtin_amdgcn_sched_barrier(0); if (g_cd_tl && blockIdx.x == 0 && lane == 0 && item < 64) { g_cd_tl[(wave * 64 + item) * 4 + (slot)] = __builtin_readcyclecounter(); \
    /* the constant 100 MHz counter next to the first and the latest stamp of wave 0: cycles per microsecond = the clock the kernel ran at */ \
    if (wave == 0 && (slot) == 0 && item == 0) { g_cd_tl[(7 * 64 + 62) * 4 + 0] = wall_clock64(); g_cd_tl[(7 * 64 + 62) * 4 + 1] = __builtin_readcyclecounter(); } \
    if (wave == 0 && (slot) == 3) { g_cd_tl[(7 * 64 + 63) * 4 + 0] = wall_clock64(); g_cd_tl[(7 * 64 + 63) * 4 + 1] = __builtin_readcyclecounter(); } } __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define CD_STAMP(slot) do { (void)item; } while (0)
#endif

// SKIP: the 1x1x1 projection of a residual block's input on the same accumulators, y = epilogue(conv3(x) + WS . xs + shift):
// xs (B,X,Y,Z,16) channels-last, WS = CdRec records of one tap [chunk 2][half 2][output 32].  Consumer waves only: lane
// (t, h) is A row = voxel (4 wave + i, t & 7, t >> 3), channels 8 chunk + 4 h .. + 3 - one float4 per (i, chunk), split
// and multiplied (24 matrix instructions) between the last step of the block's last chunk and the epilogue: once per block a
// workgroup walks.  A voxel of xs is 64 bytes, one cache line for both chunks and both lane halves: the last (dy,dz) step
// requests the first value of each row (4 registers - all eight rows held over that step spill: 256 + 72 B of scratch), the
// rest are cache hits after the step.
// POOL (with SKIP, MODE 1, grids of whole blocks only - the entry refuses the others): the MaxPool3d(2,2) of the result as
// well, stored right behind y, (B,X/2,Y/2,Z/2,32) channels-last at y + B*X*Y*Z*32.  In the interior epilogue lane (t, h) owns
// channel t of voxels x = ox0 + 4 wave + i, y = oy0 + 4 h + (v & 3), z = oz0 + (v >> 2): eight whole 2x2x2 cells, (i >> 1,
// (v & 3) >> 1, v >> 3).  Each is scanned in the order and with the comparison of maxpool2x_cl_kernel (NaN and -0/+0 come out
// the same bits); a pooled store instruction writes two 128-byte voxel rows (h = 0, 1).
template <int C, int MODE, bool SKIP = false, bool POOL = false>
__global__ __launch_bounds__(64 * (4 + CD_PROD)) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3_split_kernel(const float *__restrict__ x, const unsigned *__restrict__ W3, float *__restrict__ y,
                        const float *__restrict__ shift, const float *__restrict__ res, int B, int X, int Y, int Z, int NBX,
                        int NBY, int NBZ, int nblocks, const float *__restrict__ xs = nullptr,
                        const unsigned *__restrict__ WS = nullptr)
{
    constexpr int O = 32, NCH = C / 8, CS = 16;
    // operand roles: a split result wants (voxel, 4 consecutive channels) per lane = weights as the A operand (rows), an
    // fp32-only result wants (channel, 16 voxels) per lane = full 128-byte rows per store instruction (the transposed form's
    // 32-byte pieces cost 8-10 k cycles per block against 3-6 k)
    extern __shared__ __attribute__((aligned(16))) unsigned cd_lds[];      // 2 x CD_BUFS dwords + 4 x 1024 floats of scratch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = lane & 31, h = lane >> 5;
    const int my_blocks = ((int)blockIdx.x < nblocks) ? (nblocks - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int n_items = my_blocks * NCH;
    auto decode = [&](int item, int &b, int &ox0, int &oy0, int &oz0) {
        int bid = (int)blockIdx.x + (item / NCH) * (int)gridDim.x;
        const int bz = bid % NBZ; bid /= NBZ;
        const int by = bid % NBY; bid /= NBY;
        const int bx = bid % NBX;
        b = bid / NBX;
        ox0 = bx * CD_BX; oy0 = by * CD_BY; oz0 = bz * CD_BZ;
    };

    if (wave >= 4) {
        // ---------------- producers: item k -> buffer k & 1 ----------------
        const int pt = tid - 256;                                          // 0 .. 64*CD_PROD-1
        // fp32 input.  VALU issue on a SIMD goes to the older wave first: without priority the (younger) producers got the
        // slots the consumer's matrix stream left over - 28 cycles per instruction, 14 k cycles per item against the
        // consumers' 12 k
        __builtin_amdgcn_s_setprio(2);
        // the producers get one issue slot per consumer matrix instruction (324 per item): everything that does not depend
        // on the item is computed once - LDS offset, offset inside the sample, region coordinates
        float4 d[CD_PER];
        int lo_[CD_PER], rel[CD_PER], vxyz[CD_PER];
#pragma unroll
        for (int u = 0; u < CD_PER; ++u) {
            const int idx = pt + 64 * CD_PROD * u;
            const int v = idx >> 1, half = idx & 1;
            const int vx = v % CD_RX, vy = (v / CD_RX) % CD_RY, vz = v / (CD_RX * CD_RY);
            lo_[u] = idx < CD_NV4 ? half * CD_PLANE + vz * CD_ZP + vy * CD_ROW + vx * CD_VOX : -1;
            rel[u] = ((vx * Y + vy) * Z + vz) * C + half * 4;
            vxyz[u] = idx < CD_NV4 ? (vx | (vy << 8) | (vz << 16)) : 0x00ffffff;      // 255: never in range
        }
        auto issue = [&](int k) {                                          // loads of item k: in flight until iteration k
            int b, ox0, oy0, oz0;
            decode(k, b, ox0, oy0, oz0);
            // element offset of region voxel (0,0,0), chunk k % NCH; may be negative at the volume border (never read there)
            const int64_t vox0 = (((int64_t)b * X + (ox0 - 1)) * Y + (oy0 - 1)) * Z + (oz0 - 1);
            const float *xb = x + vox0 * C + (k % NCH) * 8;
            // voxel (vx,vy,vz) is inside the volume iff vx in [xlo, xhi) ...: wave-uniform bounds
            const int xlo = 1 - ox0, xhi = X + 1 - ox0, ylo = 1 - oy0, yhi = Y + 1 - oy0, zlo = 1 - oz0, zhi = Z + 1 - oz0;
#pragma unroll
            for (int u = 0; u < CD_PER; ++u) {
                const int vx = vxyz[u] & 255, vy = (vxyz[u] >> 8) & 255, vz = vxyz[u] >> 16;
                const bool in = vx >= xlo && vx < xhi && vy >= ylo && vy < yhi && vz >= zlo && vz < zhi;
                d[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (in) d[u] = *reinterpret_cast<const float4 *>(xb + rel[u]);
            }
        };
        if (n_items > 0) issue(0);
        for (int k = 0; k <= n_items; ++k) {
            if (k < n_items) {
                { const int item = k; CD_STAMP(0); }
                unsigned *buf = cd_lds + (k & 1) * CD_BUFS;
#ifdef SP3D_CD_TIMELINE
                __builtin_amdgcn_s_waitcnt(0);            // vmcnt(0) lgkmcnt(0): separates the load wait from the split
                { const int item = k; CD_STAMP(3); }      // (slot 3 is overwritten after the barrier for consumers only)
#endif
#pragma unroll
                for (int u = 0; u < CD_PER; ++u) {
                    u32x4 q0, q1;
                    split3(d[u], q0, q1);
                    if (lo_[u] >= 0) {
                        unsigned *p = buf + lo_[u];
                        *reinterpret_cast<u32x4 *>(p) = q0;
                        *reinterpret_cast<u32x4 *>(p + 4) = q1;
                    }
                }
                { const int item = k; CD_STAMP(1); }
                if (k + 1 < n_items) issue(k + 1);                         // one item ahead: its latency hides behind the barrier
            }
            if (k < n_items) { const int item = k; CD_STAMP(2); }
            __syncthreads();
        }
        return;
    }

    // ---------------- consumers: item k - 1 from buffer (k - 1) & 1 ----------------
    // lane (t, h): output voxels (x = 4 wave + i, y = t & 7, z = t >> 3), i = 0..3 (one accumulator each); operand j = 0..5
    // of step (dy,dz) is region voxel (4 wave + j, y + dy, z + dz), channel group h
    const int a_off = h * CD_PLANE + (t >> 3) * CD_ZP + (t & 7) * CD_ROW + 4 * wave * CD_VOX;
    // weight record of (tap, chunk, lane half h, output t): 12 dwords
    const unsigned *wl = W3 + ((int64_t)h * O + t) * 12;
    struct W3Rec { CdRec d[3]; };                      // the three dx taps of one (dy,dz) step
    auto load_w = [&](int q) {                         // q = flattened (item, step) index; weights depend on (chunk, step)
        const int cc = (q / 9) % NCH, st = q % 9;
        const unsigned *r = wl + ((int64_t)(3 * st) * NCH + cc) * 2 * O * 12;
        W3Rec w;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
#if SP3D_W16_ABLATE & 2
            // measurement build: no weight loads (what would LDS-broadcast weights be worth at most?)
            (void)r; w.d[dx].hl = u32x4{0x3f803f80u + (unsigned)q, 0x3f803f80u, 0x3f803f80u + (unsigned)dx, 0x3f803f80u};
            w.d[dx].hh = w.d[dx].hl ^ 0x00010001u; w.d[dx].mm = w.d[dx].hl ^ 0x00020002u;
#else
            w.d[dx].hl = *reinterpret_cast<const u32x4 *>(r + (int64_t)dx * NCH * 2 * O * 12);
            w.d[dx].hh = *reinterpret_cast<const u32x4 *>(r + (int64_t)dx * NCH * 2 * O * 12 + 4);
            w.d[dx].mm = *reinterpret_cast<const u32x4 *>(r + (int64_t)dx * NCH * 2 * O * 12 + 8);
#endif
        }
        return w;
    };
    struct Opnd { u32x4 lh[6], hm[6]; };
    f32x16 acc[4];
    W3Rec w0, w1;                                      // weights of flattened step q, q+1
    if (n_items > 0) w0 = load_w(0);
    __syncthreads();                                   // item 0 staged
    for (int k = 1; k <= n_items; ++k) {
        const int item = k - 1, cc = item % NCH;
        const unsigned *ab = cd_lds + (item & 1) * CD_BUFS + a_off;
        if (cc == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[m][v] = 0.0f;
        }
        auto load_a = [&](int st, Opnd &a) {
            const int dz = st / 3, dy = st % 3;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const unsigned *p = ab + dz * CD_ZP + dy * CD_ROW + j * CD_VOX;
                a.lh[j] = *reinterpret_cast<const u32x4 *>(p);
                a.hm[j] = *reinterpret_cast<const u32x4 *>(p + 4);
            }
        };
        Opnd a0, a1;
        load_a(0, a0);
        const int q0 = item * 9;
        float s0[4];                                       // SKIP: the first value of each xs row of this lane
        unsigned so[4];                                    // ... and the rows' element offsets in the sample
        CD_STAMP(0);
#pragma unroll
        for (int st = 0; st < 9; ++st) {
            if (SKIP && st == 8 && cc == NCH - 1) {
                // voxels outside the volume (edge blocks) read a clamped address; their rows are never stored
                int b, ox0, oy0, oz0;
                decode(item, b, ox0, oy0, oz0);
                // wave-uniform sample base + a 32-bit lane offset (a sample of xs is below 2^31 bytes: the entry's range check)
                const float *xb = xs + (int64_t)b * X * Y * Z * CS;
                const int ys = min(oy0 + (t & 7), Y - 1), zs = min(oz0 + (t >> 3), Z - 1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xv = min(ox0 + 4 * wave + i, X - 1);
                    so[i] = (unsigned)(((xv * Y + ys) * Z + zs) * CS + 4 * h);
                    s0[i] = xb[so[i]];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            w1 = load_w(min(q0 + st + 1, n_items * 9 - 1));             // unconditional: a branch here costs the register renaming
            if (st + 1 < 9) load_a(st + 1, a1);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(a0.lh[i + dx], w0.d[dx].hl, acc[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(a0.hm[i + dx], w0.d[dx].hh, acc[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(a0.hm[i + dx], w0.d[dx].mm, acc[i]);
            }
            // issue order: one load between matrix instructions (a wave blocked on LDS issue cannot issue its matrix
            // instructions either: tools/conv3_timeline.py)
#pragma unroll
            for (int r = 0; r < 12; ++r) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // 1 DS read
            }
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // 1 VMEM read
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 15, 0);
            __builtin_amdgcn_sched_barrier(0);
            a0 = a1;
            w0 = w1;
        }
        CD_STAMP(1);
        if (SKIP && cc == NCH - 1) {
            float4 sv[2][4];                               // xs rows of this lane, [chunk][i]
            {
                // the rest of a voxel's 64 bytes: the cache line was requested a step ago
                int b, ox0, oy0, oz0;
                decode(item, b, ox0, oy0, oz0);
                const float *xb = xs + (int64_t)b * X * Y * Z * CS;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float *p = xb + so[i];
                    sv[0][i] = make_float4(s0[i], p[1], p[2], p[3]);
                    sv[1][i] = *reinterpret_cast<const float4 *>(p + 8);
                }
            }
            // the weight records (L2 hits: 6 KB shared by every workgroup) arrive while the rows are split
            CdRec ws[2];
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                const unsigned *r = WS + (unsigned)(((c2 * 2 + h) * O + t) * 12);
                ws[c2].hl = *reinterpret_cast<const u32x4 *>(r);
                ws[c2].hh = *reinterpret_cast<const u32x4 *>(r + 4);
                ws[c2].mm = *reinterpret_cast<const u32x4 *>(r + 8);
            }
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                __builtin_amdgcn_sched_barrier(0);         // one chunk's pieces at a time: both would not fit the registers
                u32x4 lh[4], hm[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) split3(sv[c2][i], lh[i], hm[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(lh[i], ws[c2].hl, acc[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(hm[i], ws[c2].hh, acc[i]);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(hm[i], ws[c2].mm, acc[i]);
            }
        }
        if (cc == NCH - 1) {
            // D of the 32x32 MFMA: lane (col = t, h) holds rows m = 8 (v >> 2) + (v & 3) + 4 h, v = 0..15, of every accumulator;
            // row m of accumulator i is voxel (x = 4 wave + i, y = m & 7, z = m >> 3).  Each accumulator goes through the wave's
            // 4 KB of LDS scratch [voxel][channel] and comes back as (voxel, 4 channels) per lane: shift, residual, ReLU,
            // the fp32 result as float4 (128 B per voxel over 8 lanes) and / or the split operands for the next layer
            int b, ox0, oy0, oz0;
            decode(item, b, ox0, oy0, oz0);
            if (ox0 + CD_BX <= X && oy0 + CD_BY <= Y && oz0 + CD_BZ <= Z) {
                // fp32 result only, interior block: straight from the accumulators, lane (t, h) owns channel t of voxels
                // (x = 4 wave + i, y = 4 h + (v & 3), z = v >> 2); 128-byte rows per store, no LDS round trip (3 k cycles
                // against 6-9 k for the transposed form below)
                const float sh = shift[t];
                const int64_t obase = ((((int64_t)b * X + ox0 + 4 * wave) * Y + oy0 + 4 * h) * Z + oz0) * O + t;
                if (POOL) {
                    static_assert(!POOL || (SKIP && MODE == 1), "the pooled form exists for the folded skip only");
                    // final values in place of the sums, then the cells: nothing but the accumulators is live here
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int v = 0; v < 16; ++v) {
                            acc[i][v] = relu_keep_nan(acc[i][v] + sh);
                            y[obase + (((int64_t)i * Y + (v & 3)) * Z + (v >> 2)) * O] = acc[i][v];
                        }
                    const int XP = X >> 1, YP = Y >> 1, ZP = Z >> 1;
                    float *yp = y + (int64_t)B * X * Y * Z * O;
                    const int64_t pbase = ((((int64_t)b * XP + ((ox0 + 4 * wave) >> 1)) * YP + ((oy0 + 4 * h) >> 1)) * ZP + (oz0 >> 1)) * O + t;
#pragma unroll
                    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
                        for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                            for (int cz = 0; cz < 2; ++cz) {
                                float m = acc[2 * ci][8 * cz + 2 * cy];
#pragma unroll
                                for (int s = 1; s < 8; ++s) {                  // s = (dx, dy, dz)
                                    const float val = acc[2 * ci + (s >> 2)][4 * (2 * cz + (s & 1)) + 2 * cy + ((s >> 1) & 1)];
                                    m = (val > m || val != val) ? val : m;
                                }
                                yp[pbase + (((int64_t)ci * YP + cy) * ZP + cz) * O] = m;
                            }
                } else
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int64_t idx = obase + (((int64_t)i * Y + (v & 3)) * Z + (v >> 2)) * O;
                        float val = acc[i][v] + sh;
                        if (MODE == 2) val += res[idx];
                        if (MODE >= 1) val = SKIP ? relu_keep_nan(val) : fmaxf(val, 0.0f);
                        if (MODE == 3) val += res[idx];
#if SP3D_W16_ABLATE & 16
                        if (val == 123.456f)
#endif
                        y[idx] = val;
                    }
            } else {
            float *scr = reinterpret_cast<float *>(cd_lds + 2 * CD_BUFS) + wave * 1024;
            const int g = lane & 7;                                          // channel group of this lane on the way out
            const float4 sh4 = *reinterpret_cast<const float4 *>(shift + 4 * g);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
                for (int v = 0; v < 16; ++v) scr[(8 * (v >> 2) + (v & 3) + 4 * h) * 32 + t] = acc[mb][v];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = (lane >> 3) + 8 * r;
                    float4 a = *reinterpret_cast<const float4 *>(scr + m * 32 + 4 * g);
                    const int xo = ox0 + 4 * wave + mb, yo = oy0 + (m & 7), zo = oz0 + (m >> 3);
                    if (xo < X && yo < Y && zo < Z) {
                        const int64_t vox = (((int64_t)b * X + xo) * Y + yo) * Z + zo;
                        a.x += sh4.x; a.y += sh4.y; a.z += sh4.z; a.w += sh4.w;
                        float4 rr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (MODE >= 2) rr = *reinterpret_cast<const float4 *>(res + vox * O + 4 * g);
                        if (MODE == 2) { a.x += rr.x; a.y += rr.y; a.z += rr.z; a.w += rr.w; }
                        if (MODE >= 1 && SKIP) { a.x = relu_keep_nan(a.x); a.y = relu_keep_nan(a.y); a.z = relu_keep_nan(a.z); a.w = relu_keep_nan(a.w); }
                        if (MODE >= 1 && !SKIP) { a.x = fmaxf(a.x, 0.0f); a.y = fmaxf(a.y, 0.0f); a.z = fmaxf(a.z, 0.0f); a.w = fmaxf(a.w, 0.0f); }
                        if (MODE == 3) { a.x += rr.x; a.y += rr.y; a.z += rr.z; a.w += rr.w; }
#if SP3D_W16_ABLATE & 16
                        if (a.x == 123.456f)
#endif
                        *reinterpret_cast<float4 *>(y + vox * O + 4 * g) = a;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            }
        }
        CD_STAMP(2);
        __syncthreads();
        CD_STAMP(3);
    }
}


} // namespace sp3d


using namespace sp3d;

// CUs of a device, asked once per device (the query is slow); 256 where the device cannot say or has no slot
static int conv3_cu_count(int dev)
{
    static int cu_count[64] = {0};
    if (dev < 0 || dev >= 64) return 256;
    if (cu_count[dev] == 0) {
        int n = 0;
        cu_count[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cu_count[dev];
}

// launch of conv3_split_kernel<C, MODE, SKIP, POOL> behind sp3d_conv3_split and sp3d_conv3_split_skip (the skip term of xs / WS
// on the accumulators; POOL: the pooled tensor behind y); the arguments are validated
template <int C, int MODE, bool SKIP, bool POOL = false>
static int conv3_split_launch(const float *x, const void *W3, float *y, const float *shift, const float *residual, const float *xs,
                              const void *WS, int B, int X, int Y, int Z, const Conv3Grid &g, void *stream)
{
    int dev = 0;
    { const hipError_t ed = hipGetDevice(&dev); if (ed != hipSuccess) return (int)ed; }
    // persistent workgroups, one per CU (158 KB of LDS each), an equal number of blocks each
    const int cus = conv3_cu_count(dev);
    const int rounds = (int)((g.blocks + cus - 1) / cus);
    const int nwg = (int)((g.blocks + rounds - 1) / rounds);
    const size_t lds = (size_t)2 * CD_BUFS * sizeof(unsigned) + 4 * 1024 * sizeof(float);
    // the attribute is per device: remember it per device (a process that drives several GPUs launches on each); devices
    // without a slot share the last one and set it at every launch
    static bool attr_dev[64] = {};
    const int slot = (dev < 0 || dev >= 64) ? 63 : dev;
    if (!attr_dev[slot] || slot == 63) {
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(conv3_split_kernel<C, MODE, SKIP, POOL>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return (int)ea;
        attr_dev[slot] = true;
    }
    hipLaunchKernelGGL((conv3_split_kernel<C, MODE, SKIP, POOL>), dim3((unsigned)nwg), dim3(64 * (4 + CD_PROD)), lds, (hipStream_t)stream, x,
                       reinterpret_cast<const unsigned *>(W3), y, shift, residual, B, X, Y, Z, g.NBX, g.NBY, g.NBZ, (int)g.blocks, xs,
                       reinterpret_cast<const unsigned *>(WS));
    return launch_status();
}

extern "C" int sp3d_conv3_split(const float *x, const void *W3, float *y, const float *shift, const float *residual, int mode,
                                int B, int X, int Y, int Z, int C, int O, void *stream)
{
    // the quarter-resolution layers, (64 | 128) -> 128: another kernel, another weight format, the same checks in the same order
    if (O == 128) return conv3_split128(x, W3, y, shift, residual, mode, B, X, Y, Z, C, O, stream);
    const Conv3Grid g = conv3_grid(B, X, Y, Z, CD_BX, CD_BY, CD_BZ);
    const bool supported = O == 32 && (C == 16 || C == 32) && !((reinterpret_cast<uintptr_t>(W3) | reinterpret_cast<uintptr_t>(y)) & 15);
    const bool in_range = (int64_t)X * Y * Z * C * 2 <= 0x7fffffff && g.blocks <= 0x7fffffff;
    if (const int rc = conv3_check(B, X, Y, Z, mode, x && W3 && y && shift && (mode < 2 || residual), supported, in_range)) return rc;
    return with_mode(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        return C == 16 ? conv3_split_launch<16, M, false>(x, W3, y, shift, residual, nullptr, nullptr, B, X, Y, Z, g, stream)
                       : conv3_split_launch<32, M, false>(x, W3, y, shift, residual, nullptr, nullptr, B, X, Y, Z, g, stream);
    });
}

extern "C" int sp3d_conv3_split_skip(const float *x, const void *W3, float *y, const float *shift, const float *xs,
                                     const void *WS, int B, int X, int Y, int Z, int C, int O, int CS, void *stream)
{
    const Conv3Grid g = conv3_grid(B, X, Y, Z, CD_BX, CD_BY, CD_BZ);
    // this entry has no mode: SP3D_CONV3_POOL2X rides on the skip width.  The pooled form has no edge-block epilogue: a grid
    // that is not whole 16x8x4 blocks is refused before any launch
    const bool pool = CS >= 0 && (CS & SP3D_CONV3_POOL2X);
    if (pool) CS &= ~SP3D_CONV3_POOL2X;
    const bool whole = X % CD_BX == 0 && Y % CD_BY == 0 && Z % CD_BZ == 0;
    const bool supported = O == 32 && C == 32 && CS == 16 && (!pool || whole) &&
                           !((reinterpret_cast<uintptr_t>(W3) | reinterpret_cast<uintptr_t>(WS) | reinterpret_cast<uintptr_t>(xs) |
                              reinterpret_cast<uintptr_t>(y)) & 15);
    const bool in_range = (int64_t)X * Y * Z * C * 2 <= 0x7fffffff && g.blocks <= 0x7fffffff;
    if (const int rc = conv3_check(B, X, Y, Z, 1, x && W3 && y && shift && xs && WS, supported, in_range)) return rc;
    if (pool) return conv3_split_launch<32, 1, true, true>(x, W3, y, shift, nullptr, xs, WS, B, X, Y, Z, g, stream);
    return conv3_split_launch<32, 1, true>(x, W3, y, shift, nullptr, xs, WS, B, X, Y, Z, g, stream);
}


extern "C" int sp3d_debug_conv3_timeline(void *dev_buffer)
{
#ifdef SP3D_CD_TIMELINE
    unsigned long long *p = (unsigned long long *)dev_buffer;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(sp3d::g_cd_tl), &p, sizeof(p));
#else
    (void)dev_buffer;
    return SP3D_EUNSUPPORTED;
#endif
}
