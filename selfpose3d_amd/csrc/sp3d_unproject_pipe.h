// sp3d_unproject_pipe.h - device code the unprojection kernel files share: the measurement switches and the view loop of the
// pipelined kernels (unproject_pipe_kernel, unproject_brick_kernel), and the scalar tap record of the two scatter kernels
// that take a record per lane (unproject_bwd2_kernel, unproject_one_bwd_kernel).
#ifndef SP3D_UNPROJECT_PIPE_H
#define SP3D_UNPROJECT_PIPE_H
#include "sp3d_proj_pk.h"
#include "sp3d_unproject_host.h"

namespace sp3d {

// measurement only (tools/wave_timeline.py): when non-null the pipelined kernel stores s_memtime stamps
// per wave: [start, after P1(0), after view 0..V-1, end] (18 slots per wave)
// (the buffer itself, g_timeline, is a __device__ variable of each file whose kernels stamp: sp3d_unproject_host.h)
#ifdef SP3D_TIMELINE        // 1: wave start / end only (light), 2: + per-view stamps
#define SP3D_STAMP_ALWAYS(slot) do { if (tl && lane == 0) tl[slot] = __builtin_readcyclecounter(); } while (0)
#if SP3D_TIMELINE >= 2
#define SP3D_STAMP(slot) SP3D_STAMP_ALWAYS(slot)
#else
#define SP3D_STAMP(slot) do { } while (0)
#endif
#else
#define SP3D_STAMP(slot) do { } while (0)
#define SP3D_STAMP_ALWAYS(slot) do { } while (0)
#endif

// SP3D_ABLATE (sp3d_unproject_host.h), one bit at a time
#define SP3D_DIAG_ON(bit) ((SP3D_ABLATE) & (bit))
#define SP3D_DIAG_FLAGS() do { } while (0)
#if SP3D_ABLATE
#define SP3D_DIAG
#endif

struct Rec {
    int off;
    float w00, w10, w01, w11;
};

// scalar form of make_record_pk (sp3d_proj_pk.h), used by the backward scatter kernel
// ESZ: the record's offset is in units of 1/ESZ elements (ESZ = sizeof(element) gives byte offsets)
template <int JP, int ESZ = 1>
__device__ __forceinline__ Rec make_record(bool use, float ix, float iy, int w, int h)
{
    const RecPk p = make_record_pk(use, v2f{ix, iy}, w, h);
    Rec r;
    r.off = (p.y0 * w + p.x0) * (JP * ESZ);
    r.w00 = p.wt.x; r.w10 = p.wt.y; r.w01 = p.wb.x; r.w11 = p.wb.y;
    return r;
}

// The view loop shared by the pipelined kernels: P1 (lane = voxel) and G (lane = (voxel-of-4, channel quad)) for the 64
// voxels of this wave; `x,y,z` is this lane's voxel centre, `inb` whether the lane has a voxel at all.  On return
// acc[i][k] holds sum over views of the bilinear samples of voxel slot 16*i + lane/4, channel 4*(lane%4) + k, and
// mymask = number of views that see the lane's own voxel (+ bit 31: NaN sample position).
// Round 3: the projection runs on packed fp32 pairs (sp3d_proj_pk.h), a tap record is one 16-byte weight quad + one
// offset word (2 LDS instructions per slot instead of 5), the interpolation is written on channel pairs.
template <int JP, typename TI, int U = 4, int PS = JP>
__device__ __forceinline__ void pipe_views(const Views &hm, const float *__restrict__ cam, const Geom &g, int bs, float x,
                                           float y, float z, bool inb, float *ws, int lane, float (&acc)[4][4],
                                           uint32_t &mymask, unsigned long long *tl, bool vsync = false)
{
    // vsync (tuning bit 10, brick kernel only; round-5 L1-residency experiment): a workgroup barrier per view, so that all
    // waves of a workgroup gather from the SAME view at any time (every wave of the workgroup runs all V iterations)
    constexpr int NQ = JP / 4;
    int *wsi = reinterpret_cast<int *>(ws);
    float4 *ws4 = reinterpret_cast<float4 *>(ws);
    (void)tl;
    SP3D_DIAG_FLAGS();
#ifdef SP3D_DIAG
    if (SP3D_DIAG_ON(8)) {      // stagger: waves of one SIMD start up to ~1.5k cycles apart
        const unsigned hw = __builtin_amdgcn_s_getreg(63492);   // HW_ID: wave_id[3:0]
        for (unsigned k = 0; k < (hw & 3u); ++k) __builtin_amdgcn_s_sleep(8);
    }
#endif
    const unsigned long long inbm = __builtin_amdgcn_ballot_w64(inb);
    auto P1 = [&](int c) -> bool {
        const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
#ifdef SP3D_DIAG
        if (SP3D_DIAG_ON(4)) {      // no projection: a fixed record per lane (distinct pixels, in range)
            if (inb) mymask += 1u;
            const int v = (c & 1) * 64 + lane;
            wsi[WOFF + v] = (int)((unsigned)(lane * 37 + c * 4001 + 1000 + (int)(x * 0.01f)) % (unsigned)(g.w * (g.h - 2))) * (PS * (int)sizeof(TI));
            ws4[v] = make_float4(0.25f, 0.25f, 0.25f, 0.25f);
            return true;
        }
#endif
        P1State st;
        const bool go = project_pk(cm, g, x, y, z, inbm, st);
        add_mask(mymask, st.bm);
        if (st.nm != 0ull && lane_of(st.nm)) mymask |= 0x80000000u;
        if (!go) return false;
        const unsigned long long um = st.bm & ~st.nm;
        if (um == 0ull) return false;           // no voxel of this wave sees camera c
        const RecPk r = make_record_pk(lane_of(um), st.i, g.w, g.h);
        const int v = (c & 1) * 64 + lane;
        wsi[WOFF + v] = (int)__umul24((unsigned)(PS * (int)sizeof(TI)), __umul24((unsigned)r.y0, (unsigned)g.w) + (unsigned)r.x0);
        ws4[v] = make_float4(r.wt.x, r.wt.y, r.wb.x, r.wb.y);
        return true;
    };

    // gather mapping
    const int g16 = lane >> 2, q = lane & 3;
    const bool qact = q < NQ;
    const uint32_t qoff = qact ? 4u * (uint32_t)sizeof(TI) * (uint32_t)q : 0u;      // this lane's channel quad, bytes
    const size_t rowf = (size_t)g.w * PS;
    bool have = P1(0);
    SP3D_STAMP(1);
#pragma unroll 1
    for (int c = 0; c < g.V; ++c) {
        SP3D_STAMP(2 + 4 * (c < 7 ? c : 6));
        if (vsync) __builtin_amdgcn_s_barrier();
        const bool cur = have;
        // wave-uniform row bases (SGPR pairs) + one 32-bit element offset per lane: the four taps of a slot are
        // {vb, vb2} + off (+ PS as an immediate), no 64-bit VALU address arithmetic
        const char *vb = reinterpret_cast<const char *>(reinterpret_cast<const TI *>(hm.p[c]) + (size_t)bs * g.h * rowf);
        const char *vb2 = vb + rowf * sizeof(TI);
        const int rb = (c & 1) * 64 + g16;
        if (cur) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        // the 4 voxel slots of this lane group are gathered U at a time (4*U dwordx4 loads in flight);
        // P1(c+1) is scheduled between the first group's loads and its FMAs
#pragma unroll
        for (int gi = 0; gi < 4 / U; ++gi) {
            float4 t00[U], t10[U], t01[U], t11[U];
#ifdef SP3D_DIAG
            if (SP3D_DIAG_ON(2)) {
#pragma unroll
                for (int k = 0; k < U; ++k) t00[k] = t10[k] = t01[k] = t11[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else
#endif
            if (cur) {
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const uint32_t off = (uint32_t)wsi[WOFF + rb + 16 * (gi * U + k)] + qoff;      // bytes
                    // (issued in the reverse of the order the interpolation consumes them: loads return in order, so
                    // the wait for t00 covers the slot's other three and the chain needs one s_waitcnt per slot, not four)
                    t11[k] = Store4<TI>::load(reinterpret_cast<const TI *>(vb2 + off) + PS);
                    t01[k] = Store4<TI>::load(reinterpret_cast<const TI *>(vb2 + off));
                    t10[k] = Store4<TI>::load(reinterpret_cast<const TI *>(vb + off) + PS);
                    t00[k] = Store4<TI>::load(reinterpret_cast<const TI *>(vb + off));
                }
            }
            if (gi == 0) {
                __builtin_amdgcn_sched_barrier(0);
                SP3D_STAMP(3 + 4 * (c < 7 ? c : 6));     // all tap loads issued
                if (c + 1 < g.V) have = P1(c + 1);       // VALU work while the taps are in flight
                __builtin_amdgcn_sched_barrier(0);
                SP3D_STAMP(4 + 4 * (c < 7 ? c : 6));     // next view projected
            }
            if (cur && !SP3D_DIAG_ON(16)) {
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const int i = gi * U + k;
                    const float4 wq = ws4[rb + 16 * i];                 // (w00, w10, w01, w11)
                    // ATen's bilinear chain per channel: fma(se, wse, fma(sw, wsw, fma(ne, wne, nw * wnw)))
                    v2f lo = v2f{t00[k].x, t00[k].y} * pk2(wq.x), hi = v2f{t00[k].z, t00[k].w} * pk2(wq.x);
                    lo = pk_fma(v2f{t10[k].x, t10[k].y}, pk2(wq.y), lo); hi = pk_fma(v2f{t10[k].z, t10[k].w}, pk2(wq.y), hi);
                    lo = pk_fma(v2f{t01[k].x, t01[k].y}, pk2(wq.z), lo); hi = pk_fma(v2f{t01[k].z, t01[k].w}, pk2(wq.z), hi);
                    lo = pk_fma(v2f{t11[k].x, t11[k].y}, pk2(wq.w), lo); hi = pk_fma(v2f{t11[k].z, t11[k].w}, pk2(wq.w), hi);
                    const v2f a0 = v2f{acc[i][0], acc[i][1]} + lo, a1 = v2f{acc[i][2], acc[i][3]} + hi;
                    acc[i][0] = a0.x; acc[i][1] = a0.y; acc[i][2] = a1.x; acc[i][3] = a1.y;
                }
            }
        }
    }
}

} // namespace sp3d
#endif
