// sp3d_conv3_quarter.hip - the direct (implicit-GEMM) 3x3x3 convolution of the quarter-resolution V2V layers
// (64 | 128 -> 128 channels on 20x20x5 and its like) in inference: conv3_split128_kernel and its C entry.  The arithmetic
// is conv3_split_kernel's (sp3d_conv3_direct.hip): exact three-piece bf16 splits, six partial products in three matrix
// instructions per 8 channels, fp32 accumulation; what differs is the shape of the work.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sp3d.h"
#include "sp3d_conv3_host.h"
#include "sp3d_split.h"

namespace sp3d {

// A quarter-resolution grid has few voxels (8000 at batch 4) and many channels.  The full-resolution kernel's 16x8x4 block
// wastes two thirds of a 20x20x5 grid and gives too few blocks for the chip; here
//   workgroup = one block of 5x5x5 = 125 output voxels (four 32-row matrix blocks, 97.7 % full) x 32 of the 128 outputs:
//     4x4x1 blocks per 20x20x5 sample, 64 at batch 4, x 4 output groups = 256 workgroups;
//   the four consumer waves (one per SIMD) own the SAME rows and outputs and disjoint shares of K: wave w takes the taps
//     w, w + 4, ... of every 8-channel chunk (7/7/7/6; the fourth wave's seventh step only loads), each into its own
//     4 x 16 accumulators.  The partial sums meet once, in LDS, added in the fixed order ((w0 + w1) + w2) + w3: the result
//     does not depend on timing;
//   four producer waves stage the 7x7x7 input region of the next chunks, split once, while the consumers multiply - as in
//     conv3_split_kernel, one barrier per chunk, but through three buffers (see the consumers' loop) - and help with the
//     epilogue.
// Row -> voxel: row m = (y 5 + x) 5 + z of the block; a lane keeps the LDS offset of its four rows' voxels, the operand of
// tap (dx,dy,dz) is that offset + a wave-uniform constant.  Rows past the block (125..127) or outside the volume (edge
// blocks) read a clamped voxel and are never stored.
// LDS image of a chunk: per lane half (4-channel group) two arrays of 16-byte records, {lo,hi} and {hi,mid}, record index
// x Q_PX + y Q_PY + z.  With these pitches and this row order the 16 lanes of every ds_read_b128 lane group sit on 16
// distinct 16-byte slots of the 256-byte bank row (searched over pitches and axis orders: 32-byte [lo hi | hi mid]
// records are 2-way at best).
// Weights: 24 bytes per (output, 4 channels) - the pieces hi, lo, mid once each (_lib.conv_weights_split24) - in blocks of
// 1 536 contiguous bytes per (tap, chunk, 32 outputs): one global_load_dwordx4 and one global_load_dwordx2 per wave and
// tap, each over whole cache lines, and no two waves of a workgroup load the same block.  (With the 48-byte records of
// conv3_split_kernel - three 16-byte loads with a 48-byte lane stride, 24 cache lines each - the weight stream cost 12 of
// the layer's 41 us: profiles/r15_quarter_direct_resources.md.)  Workgroups that share an XCD's L2 share an output group
// (blockIdx % 8 is the XCD): each L2 holds 27 C 32 6 B = 0.66 MB of weights at C = 128.
constexpr int Q_BX = 5, Q_BY = 5, Q_BZ = 5, Q_ROWS = Q_BX * Q_BY * Q_BZ;            // 125 <= 128
constexpr int Q_RX = Q_BX + 2, Q_RY = Q_BY + 2, Q_RZ = Q_BZ + 2;
constexpr int Q_PY = 9, Q_PX = 69;
constexpr int Q_NREC = (Q_RX - 1) * Q_PX + (Q_RY - 1) * Q_PY + Q_RZ;                // 475 records per array
constexpr int Q_ARR = Q_NREC * 4;                                                   // dwords
constexpr int Q_BUF = 4 * Q_ARR;                                                    // [half][{lo,hi} | {hi,mid}]: 30 400 B
constexpr int Q_NV4 = Q_RX * Q_RY * Q_RZ * 2;                                       // float4 per chunk: 686
constexpr int Q_PER = (Q_NV4 + 255) / 256;                                          // 3 per producer lane
constexpr int Q_LDS = 4 * 128 * 32;                                                 // dwords: the four waves' partial sums
#ifndef SP3D_Q_ABLATE
// measurement builds only (profiles/r15_quarter_direct_resources.md): 1 no matrix instructions, 2 no weight loads, 8 no LDS
// operand reads, 32 no staging; of the staging alone: 64 no split arithmetic, 128 no input loads, 256 no LDS stores
#define SP3D_Q_ABLATE 0
#endif
constexpr int Q_NBUF = 3;                                                           // staging buffers: see the barrier placement below
constexpr int Q_LDS_ALL = Q_NBUF * Q_BUF > Q_LDS ? Q_NBUF * Q_BUF : Q_LDS;          // dwords: 91 200 B
static_assert(Q_ROWS <= 128 && Q_RZ < Q_PY, "four row blocks; record Q_RZ of row (0,0) is no voxel's");

template <int C, int MODE>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3_split128_kernel(const float *__restrict__ x, const unsigned *__restrict__ W3, float *__restrict__ y,
                           const float *__restrict__ shift, const float *__restrict__ res, int X, int Y, int Z, int NBX,
                           int NBY, int NBZ, int nblocks)
{
    constexpr int O = 128, NCH = C / 8;
    extern __shared__ __attribute__((aligned(16))) unsigned q_lds[];      // Q_LDS_ALL dwords
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), t = lane & 31, h = lane >> 5;
    // consecutive workgroups go round the 8 XCDs: two XCDs per output group, the blocks dealt to the two in turn
    const int xcd = (int)blockIdx.x & 7, og = xcd >> 1;
    int bid = ((int)blockIdx.x >> 3) * 2 + (xcd & 1);
    if (bid >= nblocks) return;                                        // the whole workgroup, before its first barrier
    const int bz = bid % NBZ; bid /= NBZ;
    const int by = bid % NBY; bid /= NBY;
    const int bx = bid % NBX, b = bid / NBX;
    const int ox0 = bx * Q_BX, oy0 = by * Q_BY, oz0 = bz * Q_BZ;
    const int64_t sample = (int64_t)b * X * Y * Z;                     // voxels before this sample

    if (wave >= 4) {
        // ---------------- producers: chunk k -> buffer k % 3 ----------------
        const int pt = tid - 256;
        // no raised priority (conv3_split_kernel's producers have it): these have issue slots to spare - 84 matrix
        // instructions per chunk and SIMD against ~150 producer instructions - and with it the layer ran 1.8 us longer
        const float *xb = x + sample * C;
        float4 d[Q_PER];
        // LDS dword offset (lanes past the region: a record no voxel uses), element offset in the sample (voxels outside the
        // volume: element 0, loaded and replaced by zero) - no lane-varying branch around a load or a store
        int lo_[Q_PER], rel[Q_PER];
        bool in_[Q_PER];
#pragma unroll
        for (int u = 0; u < Q_PER; ++u) {
            const int idx = pt + 256 * u, v = idx >> 1, half = idx & 1;
            const int vz = v % Q_RZ, vy = (v / Q_RZ) % Q_RY, vx = v / (Q_RZ * Q_RY);
            const int gx = ox0 - 1 + vx, gy = oy0 - 1 + vy, gz = oz0 - 1 + vz;
            const bool have = idx < Q_NV4;
            // the halo stops at the volume's faces: what lies beyond is zero, never the neighbouring sample
            in_[u] = have && gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z;
            lo_[u] = half * 2 * Q_ARR + (have ? vx * Q_PX + vy * Q_PY + vz : Q_RZ) * 4;      // record Q_RZ: z = 7 of row (0,0)
            rel[u] = in_[u] ? ((gx * Y + gy) * Z + gz) * C + half * 4 : 0;
        }
        auto issue = [&](int k) {
#pragma unroll
            for (int u = 0; u < Q_PER; ++u)
#if SP3D_Q_ABLATE & 128
                d[u] = make_float4((float)(rel[u] + k), 1.0f, 2.0f, 3.0f);
#else
                d[u] = *reinterpret_cast<const float4 *>(xb + rel[u] + k * 8);
#endif
        };
#if !(SP3D_Q_ABLATE & 32)
        issue(0);
#endif
        for (int k = 0; k < NCH; ++k) {
            unsigned *buf = q_lds + (k % Q_NBUF) * Q_BUF;
#pragma unroll
            for (int u = 0; u < (SP3D_Q_ABLATE & 32 ? 0 : Q_PER); ++u) {
                u32x4 q0, q1;
#if SP3D_Q_ABLATE & 64
                q0 = u32x4{__float_as_uint(d[u].x), __float_as_uint(d[u].y), __float_as_uint(d[u].z), __float_as_uint(d[u].w)}; q1 = q0;
#else
                split3(in_[u] ? d[u] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), q0, q1);
#endif
#if SP3D_Q_ABLATE & 256
                asm volatile("" :: "v"(q0), "v"(q1));
#else
                *reinterpret_cast<u32x4 *>(buf + lo_[u]) = q0;
                *reinterpret_cast<u32x4 *>(buf + lo_[u] + Q_ARR) = q1;
#endif
            }
            if (k + 1 < NCH && !(SP3D_Q_ABLATE & 32)) issue(k + 1);                             // one chunk ahead: its latency hides behind the barrier
            __syncthreads();
        }
        __syncthreads();                                               // the consumers have read the last chunk
    } else {
        // ---------------- consumers: chunk k from buffer k % 3 ----------------
        // lane (t, h): rows m = t + 32 i, i = 0..3, channel group h of the chunk
        int a_off[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = min(t + 32 * i, Q_ROWS - 1);
            const int vz = min(m % Q_BZ, Z - 1 - oz0), vx = min((m / Q_BZ) % Q_BX, X - 1 - ox0), vy = min(m / (Q_BZ * Q_BX), Y - 1 - oy0);
            a_off[i] = h * 2 * Q_ARR + (vx * Q_PX + vy * Q_PY + vz) * 4;
        }
        // step j of a chunk is tap wave + 4 j; the fourth wave's step 6 loads tap 26 again and multiplies nothing
        auto tap_of = [&](int j) { return min(wave + 4 * j, 26); };
        auto tap_off = [&](int j) { const int tp = tap_of(j); return ((tp % 3) * Q_PX + ((tp / 3) % 3) * Q_PY + tp / 9) * 4; };
        // weights of (tap, chunk, output group): 1 536 contiguous bytes = [half][t] x {bh,bl} (16 B) then [half][t] x {bm} (8 B);
        // {bh,bh} and {bm,bm} are assembled in registers: hb = [bh' bh bl] holds {bh,bh} in dwords 0..3 and {bh,bl} in 2..5
        struct Wrec { u32x4 hl; u32x2 m; };
        struct Opnd { u32x4 lh[4], hm[4]; };
        const unsigned *wl = W3 + og * 384 + (h * 32 + t) * 4;
        auto load_w = [&](int cc, int j) {                             // j is a compile-time constant at every call
            const unsigned *r = wl + (tap_of(j) * NCH + cc) * (4 * 384);
            Wrec w;
#if SP3D_Q_ABLATE & 2
            w.hl = u32x4{0x3f803f80u + (unsigned)(size_t)r, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
            w.m = u32x2{w.hl.x ^ 0x00020002u, 0x3f813f80u};
#else
            w.hl = *reinterpret_cast<const u32x4 *>(r);
            w.m = *reinterpret_cast<const u32x2 *>(r + 256 - (h * 32 + t) * 2);
#endif
            return w;
        };
        auto load_a = [&](const unsigned *buf, int j, Opnd &a) {
            const int off = tap_off(j);
#pragma unroll
            for (int i = 0; i < ((SP3D_Q_ABLATE & 8) && j > 0 ? 0 : 4); ++i) {
                const unsigned *p = buf + a_off[i] + off;
                a.lh[i] = *reinterpret_cast<const u32x4 *>(p);
                a.hm[i] = *reinterpret_cast<const u32x4 *>(p + Q_ARR);
            }
        };
        f32x16 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][v] = 0.0f;
        Wrec w0 = load_w(0, 0), w1 = load_w(0, 1), w2 = load_w(0, 2), w3;
        __syncthreads();                                               // chunk 0 staged
        // Three buffers, so that the barrier "chunk cc + 1 staged" can stand BEFORE the last step of chunk cc: that step
        // fetches the first operands of the next chunk, and the matrix stream runs through the chunk boundary (with two
        // buffers the barrier has to follow the last read of chunk cc, and every chunk began with an exposed LDS latency).
        // The producers pass that barrier to write chunk cc + 2 into the buffer of chunk cc - 1, which all have left.
        Opnd a0, a1;
        load_a(q_lds, 0, a0);
        for (int cc = 0; cc < NCH; ++cc) {
            const unsigned *buf = q_lds + (cc % Q_NBUF) * Q_BUF;
            const unsigned *nbuf = q_lds + (min(cc + 1, NCH - 1) % Q_NBUF) * Q_BUF;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                __builtin_amdgcn_sched_barrier(0);
                // weights three steps ahead, across the chunk boundary (the last three loads of the kernel are not used): an
                // L2 hit under this load takes longer than the 24 matrix instructions of two steps
                w3 = load_w(min(cc + (j + 3) / 7, NCH - 1), (j + 3) % 7);
                if (SP3D_Q_ABLATE & 8) a1 = a0;
                if (j == 6 && cc + 1 < NCH) __syncthreads();           // chunk cc + 1 staged
                load_a(j + 1 < 7 ? buf : nbuf, (j + 1) % 7, a1);       // after the last chunk: read again, not used
#if SP3D_Q_ABLATE & 1
#pragma unroll
                for (int i = 0; i < 4; ++i) asm volatile("" :: "v"(a0.lh[i]), "v"(a0.hm[i]), "v"(w0.hl), "v"(w0.m));
#else
                if (j < 6 || wave < 3) {                               // the fourth wave has six taps: its step 6 only loads
                    const u32x6 hb = {w0.hl.x, w0.hl.y, w0.hl.x, w0.hl.y, w0.hl.z, w0.hl.w};
                    const u32x4 mm = {w0.m.x, w0.m.y, w0.m.x, w0.m.y};
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(a0.lh[i], split3_q1(hb), acc[i]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(a0.hm[i], split3_q0(hb), acc[i]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = mfma_bf16(a0.hm[i], mm, acc[i]);
                }
#endif
                // issue order: one load between matrix instructions (see conv3_split_kernel), the weight loads first
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // 1 VMEM read
                }
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // 1 DS read
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_barrier(0);
                a0 = a1;
                w0 = w1;
                w1 = w2;
                w2 = w3;
            }
        }
        __syncthreads();                                               // all have read the last chunk: its LDS takes the partial sums
        // D of the 32x32 matrix instruction: lane (col = t, h) holds rows 8 (v >> 2) + (v & 3) + 4 h of each accumulator
        float *scr = reinterpret_cast<float *>(q_lds) + wave * (128 * 32);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 16; ++v) scr[(32 * i + 8 * (v >> 2) + (v & 3) + 4 * h) * 32 + t] = acc[i][v];
    }
    __syncthreads();
    // ---------------- epilogue, all eight waves: (row, 4 outputs) per lane, a voxel's 32 outputs = one 128-byte row ----------------
    const float *part = reinterpret_cast<const float *>(q_lds);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int item = tid + 512 * u, m = item >> 3, g = item & 7;
        const int xo = ox0 + (m / Q_BZ) % Q_BX, yo = oy0 + m / (Q_BZ * Q_BX), zo = oz0 + m % Q_BZ;
        if (m < Q_ROWS && xo < X && yo < Y && zo < Z) {
            float4 a = *reinterpret_cast<const float4 *>(part + m * 32 + 4 * g);
#pragma unroll
            for (int w = 1; w < 4; ++w) {                              // ((w0 + w1) + w2) + w3
                const float4 p = *reinterpret_cast<const float4 *>(part + w * (128 * 32) + m * 32 + 4 * g);
                a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
            }
            const float4 sh4 = *reinterpret_cast<const float4 *>(shift + og * 32 + 4 * g);
            const int64_t o = ((sample + ((int64_t)xo * Y + yo) * Z + zo)) * O + og * 32 + 4 * g;
            a.x += sh4.x; a.y += sh4.y; a.z += sh4.z; a.w += sh4.w;
            float4 rr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (MODE >= 2) rr = *reinterpret_cast<const float4 *>(res + o);
            if (MODE == 2) { a.x += rr.x; a.y += rr.y; a.z += rr.z; a.w += rr.w; }
            // fmaxf, as wino_output_kernel: the tier's behaviour on non-finite values does not change
            if (MODE >= 1) { a.x = fmaxf(a.x, 0.0f); a.y = fmaxf(a.y, 0.0f); a.z = fmaxf(a.z, 0.0f); a.w = fmaxf(a.w, 0.0f); }
            if (MODE == 3) { a.x += rr.x; a.y += rr.y; a.z += rr.z; a.w += rr.w; }
            *reinterpret_cast<float4 *>(y + o) = a;
        }
    }
}

} // namespace sp3d


using namespace sp3d;

template <int C, int MODE>
static int conv3_split128_launch(const float *x, const void *W3, float *y, const float *shift, const float *residual, int X,
                                 int Y, int Z, const Conv3Grid &g, void *stream)
{
    // 4 output groups x blocks, in groups of 8 consecutive workgroups = (4 output groups) x (2 blocks)
    const unsigned nwg = (unsigned)(8 * ((g.blocks + 1) / 2));
    const size_t lds = (size_t)Q_LDS_ALL * sizeof(unsigned);
    // more than 64 KB of LDS: the attribute is per device, remembered per device (devices without a slot share the last one
    // and set it at every launch), as conv3_split_launch does
    int dev = 0;
    { const hipError_t ed = hipGetDevice(&dev); if (ed != hipSuccess) return (int)ed; }
    static bool attr_dev[64] = {};
    const int slot = (dev < 0 || dev >= 64) ? 63 : dev;
    if (!attr_dev[slot] || slot == 63) {
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(conv3_split128_kernel<C, MODE>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return (int)ea;
        attr_dev[slot] = true;
    }
    hipLaunchKernelGGL((conv3_split128_kernel<C, MODE>), dim3(nwg), dim3(512), lds, (hipStream_t)stream, x,
                       reinterpret_cast<const unsigned *>(W3), y, shift, residual, X, Y, Z, g.NBX, g.NBY, g.NBZ, (int)g.blocks);
    return launch_status();
}

// sp3d_conv3_split hands its O = 128 calls to this function (sp3d_conv3_direct.hip): the C ABI has one direct-convolution entry
int sp3d::conv3_split128(const float *x, const void *W3, float *y, const float *shift, const float *residual, int mode,
                         int B, int X, int Y, int Z, int C, int O, void *stream)
{
    // output blocks: one entry today; another block shape (bx by bz <= 128) is another instantiation where a measured
    // shape needs it
    const Conv3Grid g = conv3_grid(B, X, Y, Z, Q_BX, Q_BY, Q_BZ);
    const uintptr_t align = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W3) | reinterpret_cast<uintptr_t>(y) |
                            reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(residual);
    const bool supported = O == 128 && (C == 64 || C == 128) && !(align & 15);
    const bool in_range = (int64_t)X * Y * Z * O * 2 <= 0x7fffffff && g.blocks <= 0x0fffffff;
    if (const int rc = conv3_check(B, X, Y, Z, mode, x && W3 && y && shift && (mode < 2 || residual), supported, in_range)) return rc;
    return with_mode(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        return C == 64 ? conv3_split128_launch<64, M>(x, W3, y, shift, residual, X, Y, Z, g, stream)
                       : conv3_split128_launch<128, M>(x, W3, y, shift, residual, X, Y, Z, g, stream);
    });
}
