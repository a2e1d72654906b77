// sp3d_unproject_brick.hip - unproject_brick_kernel (the hot kernel), unproject_brick_h_kernel and their kernel table.
#include "sp3d_unproject_pipe.h"
#include "sp3d_twiddles.h"

namespace sp3d {

#ifdef SP3D_TIMELINE     // this file's copy of the timeline buffer (sp3d_unproject_host.h)
static __device__ unsigned long long *g_timeline = nullptr;
int set_brick_timeline(unsigned long long *p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &p, sizeof(p)); }
#endif

// ------------------------------------------------------------------------------------------
// "brick" kernel: the same per-wave pipeline, but a wave owns a 4x4x4 block of voxels instead of 64
// consecutive ones, and a workgroup is a stack of `zw` such bricks along z.
//
// Why: the gather is bound by L1 misses, not bytes (profiles/r01_pmc_unproject_coarse_b4.json: 9 L2
// requests per 16-quad wave-load, TA busy 76 % of the kernel).  64 consecutive voxels are 3.2 z-columns:
// their projections in one view form 3 well separated vertical runs, and no two voxels of the wave
// share a 128-B line (2.5 distinct lines per voxel-view on the root grid, 2.3 on the 64^3 person
// cubes).  A compact brick always has neighbours along every camera's line of sight; those project
// onto nearly the same pixels: 1.7 lines per voxel-view on the root grid (80 mm voxels, ~4 px apart),
// 0.6-0.8 on the 64^3 cubes and the 160x160x40 grid (tools/sim_l1.py).
//
// Lane -> voxel: lx = lane/16, ly = (lane/4)%4, lz = lane%4 (z fastest, as in memory).  Gather slot i
// of lane group g16 is voxel 16*i + g16, i.e. (lx, ly, lz) = (i, g16/4, g16%4).
// Planar results: every wave leaves its (J x 64) tile in LDS, then the workgroup stores whole z-runs:
// a 16-byte piece = 4 z of one (channel, column), `zw` pieces in a row are contiguous, and so are the
// 4 y-neighbouring columns (when Y pitch == Z): 4*zw*16-byte runs.  Channels-last results leave from
// the gather mapping directly (64 B per voxel).
// ------------------------------------------------------------------------------------------

#ifndef SP3D_BRICK_U
#define SP3D_BRICK_U 4          // voxel slots gathered per batch of tap loads (16 dwordx4 in flight at 4)
#endif
#ifndef SP3D_BRICK_MINW
#define SP3D_BRICK_MINW 4
#endif
// the ZD form's own gather depth / occupancy target (its workgroups are 5 waves: 3 fit a CU at 4 waves per SIMD, 4 at 5)
// U = 2: 88 VGPRs -> 5 waves per SIMD -> FOUR 5-wave workgroups per CU instead of three: 37.5 -> 32.9 us warm, 51.8 -> 48.1
// behind a cache flush (U = 1 / 6 waves: 33.2 / 51.7).  The one-brick workgroups of the other forms keep U = 4 (26.1 vs 24.4 us).
#ifndef SP3D_ZD_U
#define SP3D_ZD_U 2
#endif
#ifndef SP3D_ZD_MINW
#define SP3D_ZD_MINW SP3D_BRICK_MINW
#endif
// ZD (round 6, root grid only: Z == ZDZ voxels = the whole z extent in ONE stack, JP == 16, float in / out): the workgroup
// does not store its cubes at all.  Its 4 x 4 columns x Z x J values stay in LDS and leave as the z-SPECTRUM the opening
// 7^3 conv wants (the direct ZDZ -> ZDSZ/2+1 point DFT of zdft_fwd_cl_kernel, sp3d_fft.hip: same table, same FMA order,
// same bits), in a layout whose unit is this workgroup's 4 x 4 tile: (B, J, K, X/4, Y/4, 16) complex, so every store is
// one whole 128-byte line.  `cubes` then points at that spectrum.  Deletes the cubes' write + re-read (2 x 32.8 MB at
// B = 4) and one launch from the root-net step; cfft2d_88_kernel un-tiles while it loads a plane into LDS.
template <int JP, bool OUTCL, typename TI = float, typename TO = float, bool ZD = false, int PS = JP>
__global__ __launch_bounds__(512, ZD ? SP3D_ZD_MINW : SP3D_BRICK_MINW) void unproject_brick_kernel(Views hm, const float *__restrict__ cam,
                                                                const float *__restrict__ centers,
                                                                const uint8_t *__restrict__ valid,
                                                                float *__restrict__ cubes, float *__restrict__ grids,
                                                                Geom g, int wgs_per_sample, int nby, int nzc, int zw)
{
    constexpr int NQ = JP / 4;
    constexpr int WLDS = (JP * WOSTR > WREC) ? JP * WOSTR : WREC;
    extern __shared__ __attribute__((aligned(16))) float bsmem[];
    int b, wg;
    if (!xcd_map_fast(blockIdx.x, g, b, wg)) return;
    SP3D_DIAG_FLAGS();
    int zc, t;
    if (!(g.xcd_order & 2)) {   // default (round 3): z slowest - consecutive workgroups sweep (y, x) inside one z-layer of bricks
        // and an XCD's chunk is a z-slab: -3 % on all three grids (profiles/r03_ab_zslab.json)
        udiv_magic((uint32_t)wg, (uint32_t)g.bk_nxy, g.bk_magic_nxy, zc, t);
    } else {                    // tuning (z-fastest order): round 2's order, z fastest
        zc = wg % nzc; t = wg / nzc;
    }
    int bx, by;
    udiv_magic((uint32_t)t, (uint32_t)g.bk_nby, g.bk_magic_nby, bx, by);
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = bx * BR, y0 = by * BR, zbase = zc * zw * BR, z0 = zbase + wave * BR;
    TO *cb = reinterpret_cast<TO *>(cubes) + (OUTCL ? (size_t)b * g.J * g.N : (size_t)b * g.sB);
    float *ws = bsmem + wave * WLDS;

    // P1 mapping: this lane's voxel
    const int lx = lane >> 4, ly = (lane >> 2) & 3, lz = lane & 3;
    const int vx = x0 + lx, vy = y0 + ly, vz = z0 + lz;
    const bool inb = vx < g.X && vy < g.Y && vz < g.Z;
    const int n = (min(vx, g.X - 1) * g.Y + min(vy, g.Y - 1)) * g.Z + min(vz, g.Z - 1);
    // gather mapping: slot i of this lane is voxel (x0 + i, y0 + g16/4, z0 + g16%4)
    const int g16 = lane >> 2, q = lane & 3;
    const bool qact = q < NQ;
    const int gy = y0 + (g16 >> 2), gz = z0 + (g16 & 3);
    const bool ginb = gy < g.Y && gz < g.Z;
    const int gn0 = (x0 * g.Y + min(gy, g.Y - 1)) * g.Z + min(gz, g.Z - 1);        // + i * YZ

    const bool dead = ZD && !valid[b];      // ZD: a skipped sample's workgroups still emit their (all-zero) spectrum lines
    if (!ZD && !valid[b]) { // skipped sample: zeros (project_layer.py:48,51,54)
        if (inb) {
            const size_t zo = (size_t)vx * g.sX + (size_t)vy * g.sY + vz;
            for (int j = 0; j < g.J; ++j)
                Store4<TO>::store1(cb + (OUTCL ? ((size_t)n * g.J + j) : ((size_t)j * g.sJ + zo)), 0.0f);
            if (grids) {
                float *gp = grids + ((size_t)b * g.N + n) * 3;
                gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
            }
            if (g.pass_mask) g.pass_mask[(size_t)b * g.N + n] = 0;
        }
        return;
    }

    if (dead) {
        for (int i = lane; i < JP * WOSTR; i += 64) ws[i] = 0.0f;
    } else if (z0 < g.Z) {      // (a stack's last waves may lie above the volume: they only join the barrier)
        const float x = linspace_step(g.Lx, g.stepx, g.X, min(vx, g.X - 1)) + centers[3 * b + 0];
        const float y = linspace_step(g.Ly, g.stepy, g.Y, min(vy, g.Y - 1)) + centers[3 * b + 1];
        const float z = linspace_step(g.Lz, g.stepz, g.Z, min(vz, g.Z - 1)) + centers[3 * b + 2];
        if (grids && inb) {
            float *gp = grids + ((size_t)b * g.N + n) * 3;
            gp[0] = x; gp[1] = y; gp[2] = z;
        }
        uint32_t mymask = 0;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
#ifdef SP3D_TIMELINE
        unsigned long long *tl = g_timeline ? g_timeline + ((size_t)blockIdx.x * zw + wave) * 32 : nullptr;
        SP3D_STAMP_ALWAYS(0);
        if (tl && lane == 0) tl[26] = wall_clock64();
#else
        unsigned long long *tl = nullptr;
#endif
        pipe_views<JP, TI, ZD ? SP3D_ZD_U : SP3D_BRICK_U, PS>(hm, cam, g, bs, x, y, z, inb, ws, lane, acc, mymask, tl, (g.xcd_order & 4) != 0);

        // view fusion (project_layer.py:96-99) on the gather mapping
        __builtin_amdgcn_wave_barrier();
        SP3D_STAMP_ALWAYS(30);
#ifdef SP3D_TIMELINE
        if (tl && lane == 0) {
            tl[25] = wall_clock64();
            tl[28] = (unsigned long long)__builtin_amdgcn_s_getreg(63492);
            tl[29] = (unsigned long long)__builtin_amdgcn_s_getreg(63508);
            tl[31] = (unsigned long long)(mymask & 0x7fffffffu);
        }
#endif
        const float den_l = (float)(mymask & 0x7fffffffu) + 1e-6f;
        const float rden_l = (mymask & 0x80000000u) ? 0.0f : 1.0f / den_l;
        const uint32_t jbits = (1u << g.J) - 1u;    // pass-mask bits of the J real channels
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float den = __shfl(den_l, 16 * i + g16);
            const float rden = __shfl(rden_l, 16 * i + g16);      // rden = 0 makes fuse_rcp return exactly 0
            const bool bad = rden == 0.0f;
            const bool vin = ginb && (x0 + i < g.X);
            const int gn = gn0 + i * g.YZ;
            if (g.pass_mask) {
                uint32_t bits = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float pre = fuse_pre(acc[i][k], den, rden);
                    if (!bad && pre >= 0.0f && pre <= 1.0f) bits |= 1u << (4 * q + k);
                }
                if (!qact) bits = 0;
                bits |= (uint32_t)__shfl_xor((int)bits, 1);
                bits |= (uint32_t)__shfl_xor((int)bits, 2);
                if (q == 0 && vin) g.pass_mask[(size_t)b * g.N + gn] = (uint16_t)(bits & jbits);
            }
            if (OUTCL) {
                if (qact && 4 * q < g.J && vin) {
                    float4 o;
                    o.x = fuse_rcp(acc[i][0], den, rden); o.y = fuse_rcp(acc[i][1], den, rden);
                    o.z = fuse_rcp(acc[i][2], den, rden); o.w = fuse_rcp(acc[i][3], den, rden);
                    if (!SP3D_DIAG_ON(1) || o.x == 123456.0f) Store4<TO>::store_nt(cb + (size_t)gn * g.J + 4 * q, o);
                }
            } else if (qact) {
#pragma unroll
                for (int k = 0; k < 4; ++k) ws[(4 * q + k) * WOSTR + 16 * i + g16] = fuse_rcp(acc[i][k], den, rden);
            }
        }
#ifdef SP3D_TIMELINE
        if (OUTCL) {
            __builtin_amdgcn_s_waitcnt(0);                      // the result stores have left the wave
            if (tl && lane == 0) tl[27] = wall_clock64();
        }
#endif
    }
    if (OUTCL) return;
    __syncthreads();
    if constexpr (ZD) {
        // thread -> (column pos = 4 * lx + ly of the tile, channel c): a wave holds 4 channels x 16 columns, its 16-lane groups
        // store 16 complex values = one 128-byte line per (c, kz)
        constexpr int K = ZDSZ / 2 + 1;
        const int pos = tid & 15, c = tid >> 4;
        if (c >= g.J) return;
        float v[ZDZ];
#pragma unroll
        for (int wz = 0; wz < ZDZ / BR; ++wz) {
            const float4 q4 = *reinterpret_cast<const float4 *>(bsmem + wz * WLDS + c * WOSTR + pos * 4);
            v[4 * wz] = q4.x; v[4 * wz + 1] = q4.y; v[4 * wz + 2] = q4.z; v[4 * wz + 3] = q4.w;
        }
        // g.sB: complex values per sample of the WHOLE spectrum, from the host - a channel group of Jp = 32 has g.J channels
        // of its own but lies inside a spectrum of all J (resolve_fwd); the ZD form reads no other result stride
        float2 *o = reinterpret_cast<float2 *>(cubes) + (size_t)b * (size_t)g.sB + (((size_t)c * K) * (size_t)g.bk_nxy + (size_t)t) * 16 + pos;
        const size_t kstride = (size_t)g.bk_nxy * 16;
        float re[K], im[K];
        zdft_real<ZDZ, ZDSZ>(v, re, im);
#pragma unroll
        for (int k = 0; k < K; ++k) o[(size_t)k * kstride] = make_float2(re[k], im[k]);
        return;
    }
    // workgroup store of the (J, 4, 4, 4*zw) block: thread -> (channel phase jj, column, brick of the stack)
    const float rzw = 1.0f / (float)zw;
    const int per = 16 * zw;                                       // (column, brick) pairs = threads per channel phase
    const int jj = (int)(((float)(tid >> 4) + 0.5f) * rzw);        // tid / per            (0..3)
    const int cw = tid - jj * per;
    const int col = (int)(((float)cw + 0.5f) * rzw), wz = cw - col * zw;
    const int sx = x0 + (col >> 2), sy = y0 + (col & 3), sz = zbase + wz * BR;
    if (sx >= g.X || sy >= g.Y || sz >= g.Z) return;
    const float *tile = bsmem + wz * WLDS + col * 4;
    TO *dst = cb + (size_t)sx * g.sX + (size_t)sy * g.sY + sz;
    if (g.vec4 && (g.Z & 3) == 0) {
        for (int j = jj; j < g.J; j += 4) {
            const float4 o = *reinterpret_cast<const float4 *>(tile + j * WOSTR);
            if (!SP3D_DIAG_ON(1) || o.x == 123456.0f) Store4<TO>::store_nt(dst + (size_t)j * g.sJ, o);
        }
    } else {
        const int nz = min(BR, g.Z - sz);
        for (int j = jj; j < g.J; j += 4)
            for (int k = 0; k < nz; ++k) Store4<TO>::store1(dst + (size_t)j * g.sJ + k, tile[j * WOSTR + k]);
    }
}

// ------------------------------------------------------------------------------------------
// bf16 heat-maps (BASELINE configs[4]) on bricks with TWO lanes per pixel (round 4).
//
// The fp32 kernels give a 64-byte pixel to 4 lanes (16 B each).  With bf16 storage the same mapping loads 8 B per lane:
// half the bytes, the SAME 16 tap wave-loads per view - and the gather is bound by wave-loads through the texture path and
// by L1 line fills, not by bytes (profiles/r04_issue_model.md), so bf16 storage bought nothing and the conversion made it
// slower than fp32 (99.5 vs 90.3 us, ten 64^3 cubes, 4 views).  Here a 32-byte bf16 pixel goes to 2 lanes, 16 B = 8 channels
// each: a wave-load covers 32 voxels instead of 16, a view needs 8 wave-loads instead of 16, and every lane still owns 16
// accumulators (2 voxel slots x 8 channels instead of 4 x 4).  Arithmetic: the bf16 values are widened exactly (<< 16) and
// go through the same fp32 chain in the same order => the same bits as the 4-lane kernel and the oracle on the rounded maps.
// Lane -> voxel for P1 as in the fp32 brick kernel (lane = lx*16 + ly*4 + lz); gather slot i of lane pair g32 = lane/2 is
// voxel 32*i + g32.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void bf16x8_to_f32(const uint4 r, float (&f)[8])
{
    f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
    f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
    f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
}

template <int PS = 16>
__device__ __forceinline__ void pipe_views_h(const Views &hm, const float *__restrict__ cam, const Geom &g, int bs, float x,
                                             float y, float z, bool inb, float *ws, int lane, float (&acc)[2][8],
                                             uint32_t &mymask)
{
    // 16 channels per pixel gathered; PS = bf16 elements per packed pixel (16, or 32 for one group of a 32-channel pixel)
    int *wsi = reinterpret_cast<int *>(ws);
    float4 *ws4 = reinterpret_cast<float4 *>(ws);
    const unsigned long long inbm = __builtin_amdgcn_ballot_w64(inb);
    auto P1 = [&](int c) -> bool {
        const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
        P1State st;
        const bool go = project_pk(cm, g, x, y, z, inbm, st);
        add_mask(mymask, st.bm);
        if (st.nm != 0ull && lane_of(st.nm)) mymask |= 0x80000000u;
        if (!go) return false;
        const unsigned long long um = st.bm & ~st.nm;
        if (um == 0ull) return false;
        const RecPk r = make_record_pk(lane_of(um), st.i, g.w, g.h);
        const int v = (c & 1) * 64 + lane;
        wsi[WOFF + v] = (int)__umul24((unsigned)(PS * 2), __umul24((unsigned)r.y0, (unsigned)g.w) + (unsigned)r.x0);     // bytes
        ws4[v] = make_float4(r.wt.x, r.wt.y, r.wb.x, r.wb.y);
        return true;
    };
    const int g32 = lane >> 1, q = lane & 1;
    const uint32_t qoff = 16u * (uint32_t)q;                    // this lane's 8 channels, bytes
    const size_t row_bytes = (size_t)g.w * PS * 2;
    bool have = P1(0);
#pragma unroll 1
    for (int c = 0; c < g.V; ++c) {
        const bool cur = have;
        const char *vb = reinterpret_cast<const char *>(hm.p[c]) + (size_t)bs * g.h * row_bytes;
        const char *vb2 = vb + row_bytes;
        const int rb = (c & 1) * 64 + g32;
        if (cur) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        uint4 t00[2], t10[2], t01[2], t11[2];
        if (cur) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t off = (uint32_t)wsi[WOFF + rb + 32 * i] + qoff;
                t11[i] = *reinterpret_cast<const uint4 *>(vb2 + off + PS * 2);
                t01[i] = *reinterpret_cast<const uint4 *>(vb2 + off);
                t10[i] = *reinterpret_cast<const uint4 *>(vb + off + PS * 2);
                t00[i] = *reinterpret_cast<const uint4 *>(vb + off);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < g.V) have = P1(c + 1);       // VALU work while the taps are in flight
        __builtin_amdgcn_sched_barrier(0);
        if (cur) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 wq = ws4[rb + 32 * i];                 // (w00, w10, w01, w11)
                float a[8], b[8], cc[8], d[8];
                bf16x8_to_f32(t00[i], a); bf16x8_to_f32(t10[i], b); bf16x8_to_f32(t01[i], cc); bf16x8_to_f32(t11[i], d);
#pragma unroll
                for (int k = 0; k < 8; k += 2) {
                    // ATen's bilinear chain per channel: fma(se, wse, fma(sw, wsw, fma(ne, wne, nw * wnw)))
                    v2f v = v2f{a[k], a[k + 1]} * pk2(wq.x);
                    v = pk_fma(v2f{b[k], b[k + 1]}, pk2(wq.y), v);
                    v = pk_fma(v2f{cc[k], cc[k + 1]}, pk2(wq.z), v);
                    v = pk_fma(v2f{d[k], d[k + 1]}, pk2(wq.w), v);
                    const v2f s2 = v2f{acc[i][k], acc[i][k + 1]} + v;
                    acc[i][k] = s2.x; acc[i][k + 1] = s2.y;
                }
            }
        }
    }
}

// ZD (SP3D_HM_BF16_IN next to SP3D_OUT_ZSPECTRUM): the z-spectrum epilogue of unproject_brick_kernel<..., ZD> behind this
// kernel's gather.  After the view loop a wave's (16 x 64) tile lies in LDS indexed by the brick-local voxel number - the
// layout the fp32 kernel leaves - so the epilogue is that kernel's: thread -> (column, channel), zdft_real<ZDZ, ZDSZ>, the
// store address from g.sB, the `dead` zero fill for a sample that `valid` skips.  It is written out a second time, as
// unproject_one_zd_kernel's gather is: as one function both kernels call it changed the instructions of all five fp32 ZD
// instantiations (compared per kernel in the build's assembly), and those are shipped as they are.  Launch shape and LDS are
// the fp32 ZD launch's.  Every ZD = false instantiation is unchanged.
template <bool OUTCL, typename TO, int PS = 16, bool ZD = false>
__global__ __launch_bounds__(512, ZD ? SP3D_ZD_MINW : SP3D_BRICK_MINW) void unproject_brick_h_kernel(Views hm, const float *__restrict__ cam,
                                                                  const float *__restrict__ centers,
                                                                  const uint8_t *__restrict__ valid,
                                                                  float *__restrict__ cubes, float *__restrict__ grids,
                                                                  Geom g, int wgs_per_sample, int nby, int nzc, int zw)
{
    constexpr int JP = 16;
    constexpr int WLDS = (JP * WOSTR > WREC) ? JP * WOSTR : WREC;
    extern __shared__ __attribute__((aligned(16))) float bsmem[];
    int b, wg;
    if (!xcd_map_fast(blockIdx.x, g, b, wg)) return;
    int zc, t;
    if (!(g.xcd_order & 2)) udiv_magic((uint32_t)wg, (uint32_t)g.bk_nxy, g.bk_magic_nxy, zc, t);
    else { zc = wg % nzc; t = wg / nzc; }
    int bx, by;
    udiv_magic((uint32_t)t, (uint32_t)g.bk_nby, g.bk_magic_nby, bx, by);
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = bx * BR, y0 = by * BR, zbase = zc * zw * BR, z0 = zbase + wave * BR;
    TO *cb = reinterpret_cast<TO *>(cubes) + (OUTCL ? (size_t)b * g.J * g.N : (size_t)b * g.sB);
    float *ws = bsmem + wave * WLDS;

    // P1 mapping: this lane's voxel
    const int lx = lane >> 4, ly = (lane >> 2) & 3, lz = lane & 3;
    const int vx = x0 + lx, vy = y0 + ly, vz = z0 + lz;
    const bool inb = vx < g.X && vy < g.Y && vz < g.Z;
    const int n = (min(vx, g.X - 1) * g.Y + min(vy, g.Y - 1)) * g.Z + min(vz, g.Z - 1);
    const int g32 = lane >> 1, q = lane & 1;

    const bool dead = ZD && !valid[b];      // ZD: a skipped sample's workgroups still emit their (all-zero) spectrum lines
    if (!ZD && !valid[b]) { // skipped sample: zeros (project_layer.py:48,51,54)
        if (inb) {
            const size_t zo = (size_t)vx * g.sX + (size_t)vy * g.sY + vz;
            for (int j = 0; j < g.J; ++j)
                Store4<TO>::store1(cb + (OUTCL ? ((size_t)n * g.J + j) : ((size_t)j * g.sJ + zo)), 0.0f);
            if (grids) {
                float *gp = grids + ((size_t)b * g.N + n) * 3;
                gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
            }
            if (g.pass_mask) g.pass_mask[(size_t)b * g.N + n] = 0;
        }
        return;
    }

    if (dead) {
        for (int i = lane; i < JP * WOSTR; i += 64) ws[i] = 0.0f;
    } else if (z0 < g.Z) {
        const float x = linspace_step(g.Lx, g.stepx, g.X, min(vx, g.X - 1)) + centers[3 * b + 0];
        const float y = linspace_step(g.Ly, g.stepy, g.Y, min(vy, g.Y - 1)) + centers[3 * b + 1];
        const float z = linspace_step(g.Lz, g.stepz, g.Z, min(vz, g.Z - 1)) + centers[3 * b + 2];
        if (grids && inb) {
            float *gp = grids + ((size_t)b * g.N + n) * 3;
            gp[0] = x; gp[1] = y; gp[2] = z;
        }
        uint32_t mymask = 0;
        float acc[2][8];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[i][k] = 0.0f;
        pipe_views_h<PS>(hm, cam, g, bs, x, y, z, inb, ws, lane, acc, mymask);

        __builtin_amdgcn_wave_barrier();
        const float den_l = (float)(mymask & 0x7fffffffu) + 1e-6f;
        const float rden_l = (mymask & 0x80000000u) ? 0.0f : 1.0f / den_l;
        const uint32_t jbits = (1u << g.J) - 1u;    // pass-mask bits of the J real channels
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int v = 32 * i + g32;                             // this slot's voxel inside the brick
            const float den = __shfl(den_l, v);
            const float rden = __shfl(rden_l, v);
            const bool bad = rden == 0.0f;
            const int gx = x0 + (v >> 4), gy = y0 + ((v >> 2) & 3), gz = z0 + (v & 3);
            const bool vin = gx < g.X && gy < g.Y && gz < g.Z;
            const int gn = (min(gx, g.X - 1) * g.Y + min(gy, g.Y - 1)) * g.Z + min(gz, g.Z - 1);
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = fuse_rcp(acc[i][k], den, rden);
            if (g.pass_mask) {
                uint32_t bits = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float pre = fuse_pre(acc[i][k], den, rden);
                    if (!bad && pre >= 0.0f && pre <= 1.0f) bits |= 1u << (8 * q + k);
                }
                bits |= (uint32_t)__shfl_xor((int)bits, 1);
                if (q == 0 && vin) g.pass_mask[(size_t)b * g.N + gn] = (uint16_t)(bits & jbits);
            }
            if (OUTCL) {
                if (vin) {
                    TO *dst = cb + (size_t)gn * g.J + 8 * q;
                    if (sizeof(TO) == 2 && 8 * q + 4 < g.J) {
                        // bf16 cubes: the lane's 8 channels as ONE 16-byte store (round 5: two 8-byte pieces made the L2
                        // write 136 MB for 84 MB of cubes, profiles/r05_pmc_configs4_bf16_v4.json)
                        typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                        const uint2 lo = Store4<bf16_t>::pack4(make_float4(o[0], o[1], o[2], o[3]));
                        const uint2 hi = Store4<bf16_t>::pack4(make_float4(o[4], o[5], o[6], o[7]));
                        v4u t4; t4.x = lo.x; t4.y = lo.y; t4.z = hi.x; t4.w = hi.y;
                        __builtin_nontemporal_store(t4, reinterpret_cast<v4u *>(dst));
                    } else {
                        if (8 * q < g.J) Store4<TO>::store_nt(dst, make_float4(o[0], o[1], o[2], o[3]));
                        if (8 * q + 4 < g.J) Store4<TO>::store_nt(dst + 4, make_float4(o[4], o[5], o[6], o[7]));
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) ws[(8 * q + k) * WOSTR + v] = o[k];
            }
        }
    }
    if (OUTCL) return;
    __syncthreads();
    if constexpr (ZD) {
        // the ZD epilogue of unproject_brick_kernel, statement for statement: thread -> (column pos = 4 * lx + ly of the tile,
        // channel c), one 128-byte line per (c, kz); a channel group of Jp = 32 leaves through `c >= g.J` and g.sB as there
        constexpr int K = ZDSZ / 2 + 1;
        const int pos = tid & 15, c = tid >> 4;
        if (c >= g.J) return;
        float v[ZDZ];
#pragma unroll
        for (int wz = 0; wz < ZDZ / BR; ++wz) {
            const float4 q4 = *reinterpret_cast<const float4 *>(bsmem + wz * WLDS + c * WOSTR + pos * 4);
            v[4 * wz] = q4.x; v[4 * wz + 1] = q4.y; v[4 * wz + 2] = q4.z; v[4 * wz + 3] = q4.w;
        }
        float2 *o = reinterpret_cast<float2 *>(cubes) + (size_t)b * (size_t)g.sB + (((size_t)c * K) * (size_t)g.bk_nxy + (size_t)t) * 16 + pos;
        const size_t kstride = (size_t)g.bk_nxy * 16;
        float re[K], im[K];
        zdft_real<ZDZ, ZDSZ>(v, re, im);
#pragma unroll
        for (int k = 0; k < K; ++k) o[(size_t)k * kstride] = make_float2(re[k], im[k]);
        return;
    }
    // workgroup store of the (J, 4, 4, 4*zw) block: thread -> (channel phase jj, column, brick of the stack); the LDS tile
    // is indexed by the voxel's brick-local number lx*16 + ly*4 + lz, as the fp32 kernel's (slot*16 + g16)
    const float rzw = 1.0f / (float)zw;
    const int per = 16 * zw;
    const int jj = (int)(((float)(tid >> 4) + 0.5f) * rzw);
    const int cw = tid - jj * per;
    const int col = (int)(((float)cw + 0.5f) * rzw), wz = cw - col * zw;
    const int sx = x0 + (col >> 2), sy = y0 + (col & 3), sz = zbase + wz * BR;
    if (sx >= g.X || sy >= g.Y || sz >= g.Z) return;
    const float *tile = bsmem + wz * WLDS + col * 4;
    TO *dst = cb + (size_t)sx * g.sX + (size_t)sy * g.sY + sz;
    if (g.vec4 && (g.Z & 3) == 0) {
        for (int j = jj; j < g.J; j += 4) {
            const float4 o = *reinterpret_cast<const float4 *>(tile + j * WOSTR);
            Store4<TO>::store_nt(dst + (size_t)j * g.sJ, o);
        }
    } else {
        const int nz = min(BR, g.Z - sz);
        for (int j = jj; j < g.J; j += 4)
            for (int k = 0; k < nz; ++k) Store4<TO>::store1(dst + (size_t)j * g.sJ + k, tile[j * WOSTR + k]);
    }
}

#define SP3D_BRICK(JP_, CL_, TI_, TO_, ZD_, PS_) \
    SP3D_ROW(BrickFn, (KernelKey{.jp = JP_, .ps = PS_, .cl = CL_, .taps16 = is16<TI_>(), .cubes16 = is16<TO_>(), .zd = ZD_}), unproject_brick_kernel, JP_, CL_, TI_, TO_, ZD_, PS_)
// bf16 heat-maps: two lanes per pixel, 16 channels
#define SP3D_BRICK_H(CL_, TO_, PS_) \
    SP3D_ROW(BrickFn, (KernelKey{.jp = 16, .ps = PS_, .cl = CL_, .taps16 = 1, .cubes16 = is16<TO_>()}), unproject_brick_h_kernel, CL_, TO_, PS_)
// bf16 maps with the z-spectrum result (SP3D_HM_BF16_IN next to SP3D_OUT_ZSPECTRUM): 13..16 joints at PS = 16, both channel
// groups of a 32-element pixel at PS = 32 (group 1 has width 16 as well, its g.J = J - 16 channels picked by the epilogue).
// A table of its own, for the reason given below; planned by tests/test_bf16_front_host.py, run by tests/test_gpu_bf16_front.py.
#define SP3D_BRICK_H_ZD(PS_) \
    SP3D_ROW(BrickFn, (KernelKey{.jp = 16, .ps = PS_, .taps16 = 1, .zd = true}), unproject_brick_h_kernel, false, float, PS_, true)
static int find_brick_h_zspectrum_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_BRICK_H_ZD(16) SP3D_BRICK_H_ZD(32)
    return SP3D_EUNSUPPORTED;
}

// Jp = 32 channel groups with the z-spectrum result (SP3D_OUT_ZSPECTRUM): group 0 at JP = 16, group 1 at ceil4(J - 16).
// The rows are a table of their own behind find_brick_kernel: the row census of tests/test_fwd_option_sweep_reference.py counts
// the rows of find_brick_kernel that its sweep of cube-writing options reaches; these write no cubes, and each of them is
// planned by tests/test_wide_front_host.py and run by tests/test_gpu_wide_front.py.
static int find_brick_zspectrum32_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_BRICK(16, false, float, float, true, 32) SP3D_BRICK(4, false, float, float, true, 32)
    SP3D_BRICK(8, false, float, float, true, 32) SP3D_BRICK(12, false, float, float, true, 32)
    return find_brick_h_zspectrum_kernel(key, fn, name);
}

int find_brick_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_BRICK(4, false, float, float, false, 4) SP3D_BRICK(4, true, float, float, false, 4)
    SP3D_BRICK(8, false, float, float, false, 8) SP3D_BRICK(8, true, float, float, false, 8)
    SP3D_BRICK(12, false, float, float, false, 12) SP3D_BRICK(12, true, float, float, false, 12)
    SP3D_BRICK(16, false, float, float, false, 16) SP3D_BRICK(16, true, float, float, false, 16)
    SP3D_BRICK(16, false, float, float, true, 16)       // the stack's cubes leave as their z-spectrum (sp3d_unproject_fwd_zdft)
    SP3D_BRICK(16, false, float, bf16_t, false, 16) SP3D_BRICK(16, true, float, bf16_t, false, 16)
    SP3D_BRICK_H(false, float, 16) SP3D_BRICK_H(true, float, 16) SP3D_BRICK_H(false, bf16_t, 16) SP3D_BRICK_H(true, bf16_t, 16)
    // Jp = 32 channel groups: planar result
    SP3D_BRICK(4, false, float, float, false, 32) SP3D_BRICK(8, false, float, float, false, 32)
    SP3D_BRICK(12, false, float, float, false, 32) SP3D_BRICK(16, false, float, float, false, 32)
    SP3D_BRICK(16, false, float, bf16_t, false, 32) SP3D_BRICK_H(false, float, 32) SP3D_BRICK_H(false, bf16_t, 32)
    return find_brick_zspectrum32_kernel(key, fn, name);
}

} // namespace sp3d
