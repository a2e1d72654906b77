// sp3d_unproject_tile.hip - the unprojection kernels that need no clamped 2x2 tap block, and the heat-map re-tiling pass.
//   unproject_planar_kernel  lane = voxel, heat-maps in the reference's planar (B,J,h,w)
//                            layout; simple, exact, gather of 4*J scattered dwords / view.
//   pack_nhwc_kernel         (B,J,h,w) x V  ->  (V,B,h,w,Jp): LDS-tiled transpose so that a
//                            bilinear tap becomes ONE contiguous Jp*4-byte read.
//   unproject_nhwc_kernel    the first channels-last kernel ("tile"): phase 1 (lane = voxel) projects the tile's
//                            voxels through every camera and stages the sample positions in
//                            LDS; phase 2 (4 lanes = one voxel, each lane one 16-byte channel
//                            quad) gathers the taps with dwordx4 loads whose 4-lane groups
//                            read 64 contiguous bytes; phase 3 stores the (J, tile) result
//                            through LDS as coalesced dwordx4 rows.
// Their kernel tables and sp3d_pack_heatmaps[_ex]; the forward entries are in sp3d_unproject.hip.
#include "sp3d_unproject_host.h"

namespace sp3d {

// ------------------------------------------------------------------------------------------
// planar-layout forward: lane = voxel.  JC = channels accumulated per pass.
// ------------------------------------------------------------------------------------------
template <int JC>
__global__ __launch_bounds__(TILE) void unproject_planar_kernel(Views hm, const float *__restrict__ cam,
                                                               const float *__restrict__ centers,
                                                               const uint8_t *__restrict__ valid,
                                                               float *__restrict__ cubes, float *__restrict__ grids,
                                                               Geom g)
{
    const int b = blockIdx.y;
    const int bs = g.sample_of ? g.sample_of[b] : b;   // row of the heat-map batch / camera table this cube reads
    const int n = blockIdx.x * TILE + threadIdx.x;
    if (n >= g.N) return;
    float *cb = cubes + (size_t)b * g.J * g.N;
    if (!valid[b]) { // project_layer.py:48,51,54 - skipped sample stays zero
        for (int j = 0; j < g.J; ++j) cb[(size_t)j * g.N + n] = 0.0f;
        if (grids) {
            float *gp = grids + ((size_t)b * g.N + n) * 3;
            gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
        }
        return;
    }
    const int vx = n / g.YZ, rem = n - vx * g.YZ, vy = rem / g.Z, vz = rem - vy * g.Z;
    const float x = linspace_at(g.Lx, g.X, vx) + centers[3 * b + 0];
    const float y = linspace_at(g.Ly, g.Y, vy) + centers[3 * b + 1];
    const float z = linspace_at(g.Lz, g.Z, vz) + centers[3 * b + 2];
    if (grids) {
        float *gp = grids + ((size_t)b * g.N + n) * 3;
        gp[0] = x; gp[1] = y; gp[2] = z;
    }
    const float W_in = (float)g.W_in, H_in = (float)g.H_in;
    const size_t plane = (size_t)g.h * g.w;
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
            if (ix != ix || iy != iy) { bad = true; continue; } // NaN sample -> NaN -> 0 (project_layer.py:98)
            if (!bound) continue;                                // val * 0
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
        const float den = cnt + 1e-6f;
#pragma unroll
        for (int k = 0; k < JC; ++k)
            if (j0 + k < g.J) cb[(size_t)(j0 + k) * g.N + n] = bad ? 0.0f : fuse(acc[k], den);
    }
}

// ------------------------------------------------------------------------------------------
// (B,J,h,w) x V  ->  (V,B,h,w,JP) re-tiling.  One workgroup = 256 pixels of one (view,sample).
// ------------------------------------------------------------------------------------------
constexpr int PSTR = 260; // LDS row stride (floats): rows 16-B aligned, <=2-way write conflicts

template <int JP, typename TI = float, typename TO = float>
__global__ __launch_bounds__(256) void pack_nhwc_kernel(Views hm, float *__restrict__ packed_, int B, int J, int HW)
{
    __shared__ float tile[JP][PSTR];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * 256;
    const int b = blockIdx.y, v = blockIdx.z;
    const TI *src = reinterpret_cast<const TI *>(hm.p[v]) + (size_t)b * J * HW;
    TO *packed = reinterpret_cast<TO *>(packed_);
    const int p = p0 + tid;
    // all J plane loads in flight before the first LDS write: with the load inside `if (p < HW)` the compiler emitted
    // branch -> load -> s_waitcnt vmcnt(0) -> ds_write per channel, JP dependent round trips per workgroup.  The pixel index is
    // clamped instead (a lane past the end re-reads the last pixel and writes zero).
    const int pc = p < HW ? p : HW - 1;
    float vals[JP];
    // channel index clamped too (planes j >= J re-read plane J - 1 and are zeroed below): straight-line code, no branch between
    // the loads - behind a wave-uniform `j < J` branch the bf16 form still waited for every load before widening it
    if constexpr (sizeof(TI) == 2) {
        uint32_t raw[JP];
#pragma unroll
        for (int j = 0; j < JP; ++j) raw[j] = (uint32_t)reinterpret_cast<const uint16_t *>(src)[(size_t)min(j, J - 1) * HW + pc];
#pragma unroll
        for (int j = 0; j < JP; ++j) vals[j] = j < J ? __uint_as_float(raw[j] << 16) : 0.0f;
    } else {
#pragma unroll
        for (int j = 0; j < JP; ++j) vals[j] = reinterpret_cast<const float *>(src)[(size_t)min(j, J - 1) * HW + pc];
#pragma unroll
        for (int j = 0; j < JP; ++j) vals[j] = j < J ? vals[j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < JP; ++j) tile[j][tid] = p < HW ? vals[j] : 0.0f;
    __syncthreads();
    constexpr int NQ = JP / 4;
    TO *dst = packed + (((size_t)v * B + b) * HW + p0) * JP;
    for (int e = tid; e < 256 * NQ; e += 256) {
        const int px = e / NQ, q = e - px * NQ;
        if (p0 + px < HW) {
            float4 o;
            o.x = tile[4 * q + 0][px]; o.y = tile[4 * q + 1][px];
            o.z = tile[4 * q + 2][px]; o.w = tile[4 * q + 3][px];
            Store4<TO>::store_any(dst + (size_t)px * JP + 4 * q, o);           // heat-maps are caller data: NaN stays NaN
        }
    }
}

// ------------------------------------------------------------------------------------------
// channels-last forward (the hot kernel).
//   JP   = floats per pixel (channel stride), multiple of 4, <= 16 per pass
//   LDS  = sIx,sIy [V][TILE] sample positions, sMask[TILE] bound bits (+bit31 NaN flag),
//          sOut [JP][OSTR] result tile
// ------------------------------------------------------------------------------------------

template <int JP, bool XCD, int U>
__global__ __launch_bounds__(TILE) void unproject_nhwc_kernel(Views hm, const float *__restrict__ cam,
                                                             const float *__restrict__ centers,
                                                             const uint8_t *__restrict__ valid,
                                                             float *__restrict__ cubes, float *__restrict__ grids,
                                                             Geom g, int tiles_per_sample, int total_tiles)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sOut = smem;                                   // [JP][OSTR]
    float *sIx = sOut + JP * OSTR;                        // [V][TILE]
    float *sIy = sIx + g.V * TILE;                        // [V][TILE]
    uint32_t *sMask = reinterpret_cast<uint32_t *>(sIy + g.V * TILE); // [TILE]

    int b, tile;
    if (XCD) {
        if (!xcd_map(blockIdx.x, g.B, tiles_per_sample, g.xcd_chunk, b, tile)) return;
    } else {
        b = blockIdx.x / tiles_per_sample;
        tile = blockIdx.x - b * tiles_per_sample;
    }
    (void)total_tiles;
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int n0 = tile * TILE;
    const int tid = threadIdx.x;
    const int nvox = min(TILE, g.N - n0);
    float *cb = cubes + (size_t)b * g.J * g.N;
    constexpr int NQ = JP / 4;

    if (!valid[b]) { // skipped sample: zeros (project_layer.py:48,51,54)
        for (int j = 0; j < g.J; ++j)
            if (tid < nvox) cb[(size_t)j * g.N + n0 + tid] = 0.0f;
        if (grids && tid < nvox) {
            float *gp = grids + ((size_t)b * g.N + n0 + tid) * 3;
            gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
        }
        return;
    }

    // ---- phase 1: lane = voxel; project through every camera, stage sample positions
    {
        const int n = n0 + tid;
        uint32_t mask = 0;
        if (tid < nvox) {
            const int vx = n / g.YZ, rem = n - vx * g.YZ, vy = rem / g.Z, vz = rem - vy * g.Z;
            const float x = linspace_at(g.Lx, g.X, vx) + centers[3 * b + 0];
            const float y = linspace_at(g.Ly, g.Y, vy) + centers[3 * b + 1];
            const float z = linspace_at(g.Lz, g.Z, vz) + centers[3 * b + 2];
            if (grids) {
                float *gp = grids + ((size_t)b * g.N + n) * 3;
                gp[0] = x; gp[1] = y; gp[2] = z;
            }
            const float W_in = (float)g.W_in, H_in = (float)g.H_in;
            for (int c = 0; c < g.V; ++c) {
                const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
                float ix, iy;
                const bool bound = sample_pos(cm, x, y, z, g.w, g.h, W_in, H_in, ix, iy);
                if (bound) mask |= (1u << c);
                if (ix != ix || iy != iy) mask |= 0x80000000u;
                sIx[c * TILE + tid] = ix;
                sIy[c * TILE + tid] = iy;
            }
        }
        sMask[tid] = mask;
    }
    __syncthreads();

    // ---- phase 2: 4 lanes = one voxel; lane q owns channels [4q, 4q+4).  U voxels are in
    //      flight per lane (4*U dwordx4 loads issued back to back before the first use).
    {
        constexpr int LPV = 4;                 // lanes per voxel
        constexpr int GROUPS = TILE / LPV;     // 64 voxel groups per workgroup
        constexpr int VPG = TILE / GROUPS;     // 4 voxels per group
        const int grp = tid / LPV, q = tid % LPV;
        const bool qact = q < NQ;              // JP < 16: upper lanes idle
        const size_t rowf = (size_t)g.w * JP;  // floats per heat-map row
#pragma unroll 1
        for (int i0 = 0; i0 < VPG; i0 += U) {
            float acc[U][4];
            uint32_t msk[U];
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < U; ++i) {
                msk[i] = sMask[(i0 + i) * GROUPS + grp];
                if (msk[i] & 0x80000000u) msk[i] = 0x80000000u;   // NaN position: voxel is zero, skip gathers
                any |= msk[i];
                acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0f;
            }
            uint32_t cnt[U];
#pragma unroll
            for (int i = 0; i < U; ++i) cnt[i] = sMask[(i0 + i) * GROUPS + grp];
#pragma unroll 1
            for (int c = 0; c < g.V; ++c) {
                if (!__any((any >> c) & 1u)) continue;         // wave-uniform skip
                const float *vb = hm.p[c] + (size_t)bs * g.h * rowf + 4 * q;
                float4 t00[U], t10[U], t01[U], t11[U];
                float wnw[U], wne[U], wsw[U], wse[U];
                // Branch-free gather: every lane always loads.  A tap outside the heat-map (zeros
                // padding) or a lane whose voxel is not in view c gets weight 0 and a clamped /
                // parked address (pixel (0,0): all parked lanes hit one cache line).
#pragma unroll
                for (int i = 0; i < U; ++i) {
                    const bool on = qact && ((msk[i] >> c) & 1u);
                    const int t = (i0 + i) * GROUPS + grp;
                    const Bilin bl = bilin(sIx[c * TILE + t], sIy[c * TILE + t]);
                    const bool x0ok = on && bl.x0 >= 0 && bl.x0 <= g.w - 1;
                    const bool x1ok = on && bl.x0 + 1 >= 0 && bl.x0 + 1 <= g.w - 1;
                    const bool y0ok = bl.y0 >= 0 && bl.y0 <= g.h - 1;
                    const bool y1ok = bl.y0 + 1 >= 0 && bl.y0 + 1 <= g.h - 1;
                    wnw[i] = (x0ok && y0ok) ? bl.wnw : 0.0f;
                    wne[i] = (x1ok && y0ok) ? bl.wne : 0.0f;
                    wsw[i] = (x0ok && y1ok) ? bl.wsw : 0.0f;
                    wse[i] = (x1ok && y1ok) ? bl.wse : 0.0f;
                    const int xa = on ? min(max(bl.x0, 0), g.w - 1) : 0, xb = on ? min(max(bl.x0 + 1, 0), g.w - 1) : 0;
                    const int ya = on ? min(max(bl.y0, 0), g.h - 1) : 0, yb = on ? min(max(bl.y0 + 1, 0), g.h - 1) : 0;
                    const float *ra = vb + (size_t)ya * rowf, *rb = vb + (size_t)yb * rowf;
                    t00[i] = *reinterpret_cast<const float4 *>(ra + xa * JP);
                    t10[i] = *reinterpret_cast<const float4 *>(ra + xb * JP);
                    t01[i] = *reinterpret_cast<const float4 *>(rb + xa * JP);
                    t11[i] = *reinterpret_cast<const float4 *>(rb + xb * JP);
                }
#pragma unroll
                for (int i = 0; i < U; ++i) {
                    float v;
                    v = t00[i].x * wnw[i]; v = fmaf(t10[i].x, wne[i], v); v = fmaf(t01[i].x, wsw[i], v); v = fmaf(t11[i].x, wse[i], v); acc[i][0] = acc[i][0] + v;
                    v = t00[i].y * wnw[i]; v = fmaf(t10[i].y, wne[i], v); v = fmaf(t01[i].y, wsw[i], v); v = fmaf(t11[i].y, wse[i], v); acc[i][1] = acc[i][1] + v;
                    v = t00[i].z * wnw[i]; v = fmaf(t10[i].z, wne[i], v); v = fmaf(t01[i].z, wsw[i], v); v = fmaf(t11[i].z, wse[i], v); acc[i][2] = acc[i][2] + v;
                    v = t00[i].w * wnw[i]; v = fmaf(t10[i].w, wne[i], v); v = fmaf(t01[i].w, wsw[i], v); v = fmaf(t11[i].w, wse[i], v); acc[i][3] = acc[i][3] + v;
                }
            }
            if (qact) {
#pragma unroll
                for (int i = 0; i < U; ++i) {
                    const int t = (i0 + i) * GROUPS + grp;
                    const bool bad = (cnt[i] & 0x80000000u) != 0;
                    const float den = (float)__popc(cnt[i] & 0x7fffffffu) + 1e-6f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) sOut[(4 * q + k) * OSTR + t] = bad ? 0.0f : fuse(acc[i][k], den);
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 3: coalesced store of the (J, tile) block, 16 B per lane where aligned
    if (((g.N & 3) == 0) && nvox == TILE) {
        for (int e = tid; e < g.J * (TILE / 4); e += TILE) {
            const int j = e / (TILE / 4), u = e - j * (TILE / 4);
            const float4 o = *reinterpret_cast<const float4 *>(&sOut[j * OSTR + 4 * u]);
            *reinterpret_cast<float4 *>(cb + (size_t)j * g.N + n0 + 4 * u) = o;
        }
    } else {
        for (int j = 0; j < g.J; ++j)
            if (tid < nvox) cb[(size_t)j * g.N + n0 + tid] = sOut[j * OSTR + tid];
    }
}

#define SP3D_TILE(JP_, XCD_, U_) SP3D_ROW(TileFn, (KernelKey{.jp = JP_, .ps = JP_, .xcd = XCD_, .unroll = U_}), unproject_nhwc_kernel, JP_, XCD_, U_)
#define SP3D_TILES(JP_) SP3D_TILE(JP_, true, 1) SP3D_TILE(JP_, false, 1) SP3D_TILE(JP_, true, 2) SP3D_TILE(JP_, false, 2) \
    SP3D_TILE(JP_, true, 4) SP3D_TILE(JP_, false, 4)
int find_tile_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_TILES(4) SP3D_TILES(8) SP3D_TILES(12) SP3D_TILES(16)
    return SP3D_EUNSUPPORTED;
}

#define SP3D_PLANAR(JC_) SP3D_ROW(PlanarFn, (KernelKey{.jp = JC_, .ps = JC_}), unproject_planar_kernel, JC_)
int find_planar_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_PLANAR(1) SP3D_PLANAR(4) SP3D_PLANAR(16)
    return SP3D_EUNSUPPORTED;
}

#define SP3D_PACK(JP_, TI_, TO_) SP3D_ROW(PackFn, (KernelKey{.jp = JP_, .ps = JP_, .taps16 = is16<TI_>(), .cubes16 = is16<TO_>()}), pack_nhwc_kernel, JP_, TI_, TO_)
int find_pack_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_PACK(4, float, float) SP3D_PACK(8, float, float) SP3D_PACK(12, float, float) SP3D_PACK(16, float, float)
    SP3D_PACK(32, float, float) SP3D_PACK(16, bf16_t, bf16_t) SP3D_PACK(16, bf16_t, float) SP3D_PACK(16, float, bf16_t)
    SP3D_PACK(32, bf16_t, bf16_t) SP3D_PACK(32, bf16_t, float) SP3D_PACK(32, float, bf16_t)
    return SP3D_EUNSUPPORTED;
}

} // namespace sp3d

using namespace sp3d;

extern "C" int sp3d_pack_heatmaps_ex(const void *const *hm_views, void *packed, int in_bf16, int out_bf16, int B, int V,
                                     int J, int Jp, int h, int w, void *stream)
{
    if (B <= 0 || V <= 0 || J <= 0 || h <= 0 || w <= 0 || V > SP3D_MAX_VIEWS) return SP3D_EINVAL;
    if (!packed) return SP3D_ENULL;
    if (Jp < J || (Jp & 3)) return SP3D_EUNSUPPORTED;
    Views v;
    int rc = load_views(v, reinterpret_cast<const float *const *>(hm_views), V);
    if (rc) return rc;
    int HW = h * w;
    dim3 grid((HW + 255) / 256, B, V), block(256);
    hipStream_t s = (hipStream_t)stream;
    float *pk = reinterpret_cast<float *>(packed);
    const void *fn;
    const char *name;
    if (find_pack_kernel(KernelKey{.jp = Jp, .ps = Jp, .taps16 = in_bf16 ? 1 : 0, .cubes16 = out_bf16 ? 1 : 0}, fn, name)) return SP3D_EUNSUPPORTED;
    void *args[] = {&v, &pk, &B, &J, &HW};
    (void)hipLaunchKernel(fn, grid, block, args, 0, s);
    return launch_status();
}

extern "C" int sp3d_pack_heatmaps(const float *const *hm_views, float *packed, int B, int V, int J, int Jp, int h,
                                  int w, void *stream)
{
    return sp3d_pack_heatmaps_ex(reinterpret_cast<const void *const *>(hm_views), packed, 0, 0, B, V, J, Jp, h, w, stream);
}
