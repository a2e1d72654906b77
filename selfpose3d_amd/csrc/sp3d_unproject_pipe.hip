// sp3d_unproject_pipe.hip - unproject_pipe_kernel and its kernel table.
#include "sp3d_unproject_pipe.h"

namespace sp3d {

#ifdef SP3D_TIMELINE     // this file's copy of the timeline buffer (sp3d_unproject_host.h)
static __device__ unsigned long long *g_timeline = nullptr;
int set_pipe_timeline(unsigned long long *p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &p, sizeof(p)); }
#endif

// ------------------------------------------------------------------------------------------
// channels-last forward, software-pipelined per wave ("pipe" kernel).
//
// A wave owns 64 consecutive voxels and never synchronises with the other waves of its
// workgroup.  For every view c it alternates two lane mappings:
//   P1(c)   lane l = voxel l : project through camera c, reduce the sample position to one
//           record {offset of the 2x2 tap block, 4 slot weights} staged in the wave's LDS slice
//           (double buffered by view parity).  Taps outside the heat-map (zeros padding) and
//           voxels not seen by camera c become zero WEIGHTS on in-range addresses, so the gather
//           is branch free; the 2x2 block is clamped inside the image and the weights move to
//           the slot whose pixel they belong to (order of the non-zero terms of ATen's
//           bilinear FMA chain is preserved => same bits as the oracle).
//   G(c)    lane (g,q) = voxels {g, 16+g, 32+g, 48+g}, channel quad q : 16 dwordx4 loads (each
//           4-lane group reads 64 contiguous bytes) issued back to back, THEN P1(c+1) runs on the
//           VALU while they are in flight, then the 64 FMAs of view c.
// The result tile goes through the wave's LDS slice once and leaves as dwordx4 rows.
// ------------------------------------------------------------------------------------------
// (the view loop, pipe_views, is shared with the brick kernels: sp3d_unproject_pipe.h)
template <int JP, int NW, bool OUTCL, typename TI, typename TO, int U = 4, int PS = JP>
__device__ __forceinline__ void pipe_tile(const Views &hm, const float *__restrict__ cam, const float *__restrict__ centers,
                                          const uint8_t *__restrict__ valid, float *__restrict__ cubes,
                                          float *__restrict__ grids, const Geom &g, int b, int tile, float *smem,
                                          unsigned wid)
{
    constexpr int NQ = JP / 4;
    // U = voxel slots gathered per batch of loads (4, 2 and 1 measured equal in the one-tile-per-wave kernel)
    constexpr int WLDS = (JP * WOSTR > WREC) ? JP * WOSTR : WREC;   // per-wave LDS floats (sOut aliases the records)
    (void)wid;
    SP3D_DIAG_FLAGS();
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = tile * (64 * NW) + wave * 64;                          // first voxel of this wave
    if (n0 >= g.N) return;
    const int nvox = min(64, g.N - n0);
    TO *cb = reinterpret_cast<TO *>(cubes) + (OUTCL ? (size_t)b * g.J * g.N : (size_t)b * g.sB);
    float *ws = smem + wave * WLDS;
    // offset of voxel n inside one channel plane of a planar result (== n for the dense layout)
    auto plane_off = [&](int n) -> size_t {
        if (g.dense) return (size_t)n;
        int vx, rem, vy, vz;
        udiv_magic((uint32_t)n, (uint32_t)g.YZ, g.magicYZ, vx, rem);
        udiv_magic((uint32_t)rem, (uint32_t)g.Z, g.magicZ, vy, vz);
        return (size_t)vx * g.sX + (size_t)vy * g.sY + vz;
    };

    if (!valid[b]) { // skipped sample: zeros (project_layer.py:48,51,54)
        const size_t zo = OUTCL ? 0 : plane_off(n0 + (lane < nvox ? lane : 0));
        for (int j = 0; j < g.J; ++j)
            if (lane < nvox) Store4<TO>::store1(cb + (OUTCL ? ((size_t)(n0 + lane) * g.J + j) : ((size_t)j * g.sJ + zo)), 0.0f);
        if (grids && lane < nvox) {
            float *gp = grids + ((size_t)b * g.N + n0 + lane) * 3;
            gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
        }
        if (g.pass_mask && lane < nvox) g.pass_mask[(size_t)b * g.N + n0 + lane] = 0;
        return;
    }

    // this lane's voxel (P1 mapping)
    const bool inb = lane < nvox;
    const int n = n0 + (inb ? lane : 0);
    int vx, rem, vy, vz;
    udiv_magic((uint32_t)n, (uint32_t)g.YZ, g.magicYZ, vx, rem);
    udiv_magic((uint32_t)rem, (uint32_t)g.Z, g.magicZ, vy, vz);
    const float x = linspace_step(g.Lx, g.stepx, g.X, vx) + centers[3 * b + 0];
    const float y = linspace_step(g.Ly, g.stepy, g.Y, vy) + centers[3 * b + 1];
    const float z = linspace_step(g.Lz, g.stepz, g.Z, vz) + centers[3 * b + 2];
    if (grids && inb) {
        float *gp = grids + ((size_t)b * g.N + n) * 3;
        gp[0] = x; gp[1] = y; gp[2] = z;
    }
    uint32_t mymask = 0;                        // bound bits of MY voxel (+ bit 31: NaN position)
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
    const int g16 = lane >> 2, q = lane & 3;
    const bool qact = q < NQ;

#ifdef SP3D_TIMELINE
    unsigned long long *tl = g_timeline ? g_timeline + ((size_t)wid * NW + wave) * 32 : nullptr;
#else
    unsigned long long *tl = nullptr;
#endif
    SP3D_STAMP_ALWAYS(0);
#ifdef SP3D_TIMELINE
    if (tl && lane == 0) tl[26] = wall_clock64();       // chip-wide 100 MHz clock (cycle counters are per XCD)
#endif
    pipe_views<JP, TI, U, PS>(hm, cam, g, bs, x, y, z, inb, ws, lane, acc, mymask, tl);

    // view fusion (project_layer.py:96-99) on the gather mapping, result tile -> LDS
    __builtin_amdgcn_wave_barrier();
    SP3D_STAMP_ALWAYS(30);
#ifdef SP3D_TIMELINE
    if (tl && lane == 0) {      // where it ran: HW_ID (wave/simd/cu/se) and XCC_ID
        tl[25] = wall_clock64();                           // view loop done, epilogue starts
        tl[28] = (unsigned long long)__builtin_amdgcn_s_getreg(63492);
        tl[29] = (unsigned long long)__builtin_amdgcn_s_getreg(63508);
    }
    if (tl && lane == 0) tl[31] = (unsigned long long)(mymask & 0x7fffffffu);
#endif
    // per voxel (P1 mapping, once): den = #views seeing it + 1e-6, rden = RN(1/den), 0 for a NaN sample position
    const float den_l = (float)(mymask & 0x7fffffffu) + 1e-6f;
    const float rden_l = (mymask & 0x80000000u) ? 0.0f : 1.0f / den_l;
    const uint32_t jbits = (1u << g.J) - 1u;    // pass-mask bits of the J real channels (the zero pad channels have pre = 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float den = __shfl(den_l, 16 * i + g16);
        const float rden = __shfl(rden_l, 16 * i + g16);      // rden = 0 makes fuse_rcp return exactly 0
        const bool bad = rden == 0.0f;                        // NaN sample position: voxel is zero
        if (g.pass_mask) {
            // gradient pass mask (torch.clamp backward: 0 <= pre <= 1; NaN-zeroed voxels block it)
            uint32_t bits = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float pre = fuse_pre(acc[i][k], den, rden);
                if (!bad && pre >= 0.0f && pre <= 1.0f) bits |= 1u << (4 * q + k);
            }
            if (!qact) bits = 0;
            bits |= (uint32_t)__shfl_xor((int)bits, 1);
            bits |= (uint32_t)__shfl_xor((int)bits, 2);
            const int nn = 16 * i + g16;
            if (q == 0 && nn < nvox) g.pass_mask[(size_t)b * g.N + n0 + nn] = (uint16_t)(bits & jbits);
        }
        if (OUTCL) {
            // channels-last result (B, N, J): this lane's 4 channels are 16 contiguous bytes, the
            // 4 lanes of a voxel 64 B, the wave's 16 voxels of slot i 1 KiB - no LDS transpose.
            const int nn = 16 * i + g16;
            if (qact && 4 * q < g.J && nn < nvox) {
                float4 o;
                o.x = fuse_rcp(acc[i][0], den, rden); o.y = fuse_rcp(acc[i][1], den, rden);
                o.z = fuse_rcp(acc[i][2], den, rden); o.w = fuse_rcp(acc[i][3], den, rden);
                if (!SP3D_DIAG_ON(1) || o.x == 123456.0f) Store4<TO>::store_nt(cb + (size_t)(n0 + nn) * g.J + 4 * q, o);
            }
        } else if (qact) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ws[(4 * q + k) * WOSTR + 16 * i + g16] = fuse_rcp(acc[i][k], den, rden);
        }
    }
#ifdef SP3D_TIMELINE
    if (OUTCL) {
        __builtin_amdgcn_s_waitcnt(0);                          // vmcnt(0): the result stores have left the wave
        if (tl && lane == 0) tl[27] = wall_clock64();
    }
#endif
    if (OUTCL) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // 4 consecutive voxels form one 16-byte piece when they lie in one z-column (dense: any 4; strided: Z % 4 == 0)
    if (g.vec4 && ((g.N & 3) == 0) && nvox == 64 && (g.dense || (g.Z & 3) == 0)) {
        // lane -> (channel j = pass*4 + lane/16, voxel quad u = lane%16): 256 B contiguous per channel
        const int u = lane & 15;
        const size_t po = plane_off(n0 + 4 * u);
        for (int j = lane >> 4; j < g.J; j += 4) {
            const float4 o = *reinterpret_cast<const float4 *>(&ws[j * WOSTR + 4 * u]);
            if (!SP3D_DIAG_ON(1) || o.x == 123456.0f) Store4<TO>::store_nt(cb + (size_t)j * g.sJ + po, o);
        }
    } else {
        const size_t po = plane_off(n0 + (lane < nvox ? lane : 0));
        for (int j = 0; j < g.J; ++j)
            if (lane < nvox) Store4<TO>::store1(cb + (size_t)j * g.sJ + po, ws[j * WOSTR + lane]);
    }
}

// NW = waves per workgroup (waves are independent; NW only sets the dispatch granularity)
// TI / TO: storage type of the packed heat-maps / of the cubes (float or bf16_t); math is fp32.
// PS: elements per packed pixel (the buffer's channel stride); JP channels from the pixel start are gathered.  PS > JP is one
// channel group of a wider pixel (resolve_fwd: `hm` then points at the group's first channel).
template <int JP, bool XCD, int NW, bool OUTCL, typename TI = float, typename TO = float, int PS = JP>
__global__ __launch_bounds__(64 * NW) void unproject_pipe_kernel(Views hm, const float *__restrict__ cam,
                                                             const float *__restrict__ centers,
                                                             const uint8_t *__restrict__ valid,
                                                             float *__restrict__ cubes, float *__restrict__ grids,
                                                             Geom g, int tiles_per_sample, int total_tiles)
{
    constexpr int WLDS = (JP * WOSTR > WREC) ? JP * WOSTR : WREC;
    __shared__ __attribute__((aligned(16))) float smem[NW * WLDS];
    int b, tile;
    if (XCD) {
        if (!xcd_map_fast(blockIdx.x, g, b, tile)) return;
    } else {
        b = blockIdx.x / tiles_per_sample;
        tile = blockIdx.x - b * tiles_per_sample;
    }
    (void)total_tiles;
    pipe_tile<JP, NW, OUTCL, TI, TO, 4, PS>(hm, cam, centers, valid, cubes, grids, g, b, tile, smem, blockIdx.x);
}

#define SP3D_PIPE(JP_, XCD_, NW_, CL_, TI_, TO_, PS_) \
    SP3D_ROW(TileFn, (KernelKey{.jp = JP_, .ps = PS_, .cl = CL_, .taps16 = is16<TI_>(), .cubes16 = is16<TO_>(), .xcd = XCD_, .waves = NW_}), unproject_pipe_kernel, JP_, XCD_, NW_, CL_, TI_, TO_, PS_)
#define SP3D_PIPES(JP_, NW_, TI_, TO_) SP3D_PIPE(JP_, true, NW_, false, TI_, TO_, JP_) SP3D_PIPE(JP_, false, NW_, false, TI_, TO_, JP_) \
    SP3D_PIPE(JP_, true, NW_, true, TI_, TO_, JP_) SP3D_PIPE(JP_, false, NW_, true, TI_, TO_, JP_)
int find_pipe_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_PIPES(4, 1, float, float) SP3D_PIPES(8, 1, float, float) SP3D_PIPES(12, 1, float, float) SP3D_PIPES(16, 1, float, float)
    SP3D_PIPES(4, 4, float, float) SP3D_PIPES(8, 4, float, float) SP3D_PIPES(12, 4, float, float) SP3D_PIPES(16, 4, float, float)
    // bf16 storage: 16 channels, one wave per workgroup only
    SP3D_PIPES(16, 1, bf16_t, float) SP3D_PIPES(16, 1, float, bf16_t) SP3D_PIPES(16, 1, bf16_t, bf16_t)
    // Jp = 32 channel groups: planar result, XCD map
    SP3D_PIPE(4, true, 1, false, float, float, 32) SP3D_PIPE(8, true, 1, false, float, float, 32)
    SP3D_PIPE(12, true, 1, false, float, float, 32) SP3D_PIPE(16, true, 1, false, float, float, 32)
    SP3D_PIPE(16, true, 1, false, bf16_t, float, 32) SP3D_PIPE(16, true, 1, false, float, bf16_t, 32)
    SP3D_PIPE(16, true, 1, false, bf16_t, bf16_t, 32)
    return SP3D_EUNSUPPORTED;
}

} // namespace sp3d
