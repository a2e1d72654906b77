// sp3d_unproject_one.hip - the one-channel path (SP3D_HM_ONE_CHANNEL): unproject_one_kernel with its kernel table, its
// z-spectrum form unproject_one_zd_kernel (SP3D_HM_ONE_ZSPECTRUM, resolve_one_zd) with a table of its own, and the
// backward of that channel, unproject_one_bwd_kernel behind sp3d_unproject_one_bwd[_det].  The forward entries are in
// sp3d_unproject.hip (resolve_one).
#include <type_traits>

#include "sp3d_unproject_pipe.h"
#include "sp3d_twiddles.h"

namespace sp3d {

// ------------------------------------------------------------------------------------------
// one-channel forward (SP3D_HM_ONE_CHANNEL): ONE channel of a wider heat-map tensor, read where it lies - the root
// joint's map of the ROOTNET_ROOTHM root nets (cuboid_proposal_net.py:103-108 of the reference, V2VNet(1, 1)).
//
// Lane = voxel in every phase (projection, gather, view fusion, store): no LDS, no barrier.  A wave owns 64 consecutive
// voxels.  hm.p[c] points at the wanted channel's element (sample 0, row 0, pixel 0) of view c; a tap is one
// global_load_dword at  sample * s_sample + y * s_row + x * s_px  elements from it, so the same kernel reads a channel
// plane of a planar (B,Jt,h,w) tensor (Jt*h*w, w, 1) and a channel of a channels-last (B,h,w,PS) buffer
// (h*w*PS, w*PS, PS).  Projection and tap records are project_pk / make_record_pk (zero weights on clamped in-range
// addresses: a branch-free gather); interpolation and view fusion are pipe_views' / pipe_tile's, operation for
// operation, so the result has the bits of the packed path's channel.
//
// Latency (at B = 1 the root grid is 2 000 waves on 1 024 SIMDs): the views are taken in chunks of CS; a chunk's
// records stay in registers, all of its tap loads are issued back to back, and the next chunk is projected while
// they are in flight.  The FMAs run last, in view order.  VT >= V is the number of view slots the kernel is unrolled
// for (resolve_one: V itself up to 6, then 8, 10, 12, 16), CS = 4 up to 8 views and 8 above.
//
// Result: planar with g.J = 1 or 4 channels (dense or strided; channels 1-3 zeros), or channels-last (B,X,Y,Z,4) as
// one 16-byte store {v, 0, 0, 0} per lane.
//
// MASK (sp3d_unproject_one_fwd_train): the lane also writes its voxel's word of g.pass_mask - bit 0 by the predicate of
// pipe_tile / unproject_brick_kernel on the same fuse_pre value, so the words are the packed training forward's at J = 1
// (an unseen voxel passes, a NaN-zeroed one does not, a cube that `valid` skips gets zeros).  One 2-byte store per lane,
// 128 contiguous bytes per wave.  The MASK = false instantiations are the kernels of the inference path, unchanged.
// ------------------------------------------------------------------------------------------
// TI (SP3D_HM_BF16_IN: TI = bf16_t): the element type of the heat-maps.  A bf16 tap is one 2-byte load (s_sample, s_row and
// s_px stay element counts, the byte offset is (y0 * s_row + x0 * s_px) << 1), kept as loaded while the chunk's taps are in
// flight and widened exactly (<< 16) where the interpolation consumes it: the same fp32 chain in the same order, so the
// result has the bits of the TI = float kernel on the widened maps.  An odd channel of a bf16 (B,15,h,w) tensor or of a 16- or
// 32-channel bf16 pixel is 2-byte aligned only and is read in place like any other.  TI = float is what it was.
// MASK with TI = bf16_t (SP3D_HM_BF16_TRAIN on sp3d_unproject_one_fwd_train): both of the above in one instantiation - the
// mask word comes from the same fuse_pre value, so the words are the fp32 MASK kernel's on the widened maps.
template <typename TI> struct OneTap;
template <> struct OneTap<float> {
    using raw = float;
    static constexpr int SHIFT = 2;
    __device__ __forceinline__ static raw load(const char *p) { return *reinterpret_cast<const float *>(p); }
    __device__ __forceinline__ static float value(raw r) { return r; }
};
template <> struct OneTap<bf16_t> {
    using raw = uint32_t;
    static constexpr int SHIFT = 1;
    __device__ __forceinline__ static raw load(const char *p) { return (uint32_t)*reinterpret_cast<const uint16_t *>(p); }
    __device__ __forceinline__ static float value(raw r) { return __uint_as_float(r << 16); }
};

template <int VT, int CS, bool OUTCL, bool MASK = false, typename TI = float>
__global__ __launch_bounds__(64) void unproject_one_kernel(Views hm, const float *__restrict__ cam,
                                                           const float *__restrict__ centers,
                                                           const uint8_t *__restrict__ valid, float *__restrict__ cubes,
                                                           float *__restrict__ grids, Geom g, long long s_sample,
                                                           int s_row, int s_px)
{
    constexpr int NCH = (VT + CS - 1) / CS;
    int b, tile;
    if (!xcd_map_fast(blockIdx.x, g, b, tile)) return;
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int lane = threadIdx.x;
    const int n0 = tile * 64;
    if (n0 >= g.N) return;
    const int nvox = min(64, g.N - n0);
    const bool inb = lane < nvox;
    const int n = n0 + (inb ? lane : 0);
    int vx, rem, vy, vz;
    udiv_magic((uint32_t)n, (uint32_t)g.YZ, g.magicYZ, vx, rem);
    udiv_magic((uint32_t)rem, (uint32_t)g.Z, g.magicZ, vy, vz);
    // where this lane's voxel goes: channel plane j of a planar result starts j * sJ further
    float *dst = OUTCL ? cubes + ((size_t)b * g.N + n) * 4
                       : cubes + (size_t)b * g.sB + (g.dense ? (size_t)n : (size_t)vx * g.sX + (size_t)vy * g.sY + vz);
    float out = 0.0f;
    uint16_t word = 0;                              // MASK: this voxel's pass-mask word
    if (valid[b]) {
        const float x = linspace_step(g.Lx, g.stepx, g.X, vx) + centers[3 * b + 0];
        const float y = linspace_step(g.Ly, g.stepy, g.Y, vy) + centers[3 * b + 1];
        const float z = linspace_step(g.Lz, g.stepz, g.Z, vz) + centers[3 * b + 2];
        if (grids && inb) {
            float *gp = grids + ((size_t)b * g.N + n) * 3;
            gp[0] = x; gp[1] = y; gp[2] = z;
        }
        const unsigned long long inbm = __builtin_amdgcn_ballot_w64(inb);
        uint32_t mymask = 0;                        // views that see MY voxel (+ bit 31: NaN position)
        uint32_t have = 0;                          // wave-uniform: views with a record (some voxel of the wave sees them)
        uint32_t off[VT];                           // byte offset of the 2x2 block inside the sample's image
        float w00[VT], w10[VT], w01[VT], w11[VT];
        typename OneTap<TI>::raw t00[VT], t10[VT], t01[VT], t11[VT];
        const size_t pxb = (size_t)s_px * sizeof(TI), rowb = (size_t)s_row * sizeof(TI);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int c = ch * CS; c < (ch + 1) * CS && c < VT; ++c) {
                off[c] = 0u;
                w00[c] = w10[c] = w01[c] = w11[c] = 0.0f;
                if (c < g.V) {
                    const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
                    P1State st;
                    const bool go = project_pk(cm, g, x, y, z, inbm, st);
                    add_mask(mymask, st.bm);
                    if (st.nm != 0ull && lane_of(st.nm)) mymask |= 0x80000000u;
                    const unsigned long long um = st.bm & ~st.nm;
                    if (go && um != 0ull) {         // else: no voxel of this wave sees camera c
                        const RecPk r = make_record_pk(lane_of(um), st.i, g.w, g.h);
                        off[c] = (__umul24((unsigned)r.y0, (unsigned)s_row) + __umul24((unsigned)r.x0, (unsigned)s_px)) << OneTap<TI>::SHIFT;
                        w00[c] = r.wt.x; w10[c] = r.wt.y; w01[c] = r.wb.x; w11[c] = r.wb.y;
                        have |= 1u << c;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // The chunk's taps: four wave-uniform bases (scalar register pairs) + one 32-bit byte offset per lane, no
            // branch between the loads.  A view without a record (and a slot past V, which reads view 0) loads its
            // first 2x2 block with zero weights and is left out of the sum below.  Issued in the reverse of the order
            // the interpolation consumes them (loads return in order).
#pragma unroll
            for (int c = min((ch + 1) * CS, VT) - 1; c >= ch * CS; --c) {
                const char *vb = reinterpret_cast<const char *>(reinterpret_cast<const TI *>(c < g.V ? hm.p[c] : hm.p[0]) + (ptrdiff_t)bs * s_sample);
                const char *vb2 = vb + rowb;
                t11[c] = OneTap<TI>::load(vb2 + pxb + off[c]);
                t01[c] = OneTap<TI>::load(vb2 + off[c]);
                t10[c] = OneTap<TI>::load(vb + pxb + off[c]);
                t00[c] = OneTap<TI>::load(vb + off[c]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < VT; ++c) {
            // ATen's bilinear chain: fma(se, wse, fma(sw, wsw, fma(ne, wne, nw * wnw)))
            float v = OneTap<TI>::value(t00[c]) * w00[c];
            v = fmaf(OneTap<TI>::value(t10[c]), w10[c], v);
            v = fmaf(OneTap<TI>::value(t01[c]), w01[c], v);
            v = fmaf(OneTap<TI>::value(t11[c]), w11[c], v);
            const float a = acc + v;
            acc = ((have >> c) & 1u) ? a : acc;     // wave-uniform, as the pipelined kernels skip such a view
        }
        // view fusion (project_layer.py:96-99): den = #views seeing the voxel + 1e-6; NaN sample position -> 0
        const float den = (float)(mymask & 0x7fffffffu) + 1e-6f;
        const float rden = (mymask & 0x80000000u) ? 0.0f : 1.0f / den;
        out = fuse_rcp(acc, den, rden);
        if constexpr (MASK) {
            // gradient pass mask (torch.clamp backward: 0 <= pre <= 1; a NaN-zeroed voxel, rden == 0, blocks it)
            const float pre = fuse_pre(acc, den, rden);
            word = (rden != 0.0f && pre >= 0.0f && pre <= 1.0f) ? 1 : 0;
        }
    } else if (grids && inb) {                      // skipped sample: zeros (project_layer.py:48,51,54)
        float *gp = grids + ((size_t)b * g.N + n) * 3;
        gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
    }
    if (!inb) return;
    if constexpr (MASK) g.pass_mask[(size_t)b * g.N + n] = word;
    if (OUTCL) {
        Store4<float>::store_nt(dst, make_float4(out, 0.0f, 0.0f, 0.0f));
    } else {
        dst[0] = out;
        for (int j = 1; j < g.J; ++j) dst[(size_t)j * g.sJ] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------------
// one channel in, z-spectrum out (SP3D_HM_ONE_ZSPECTRUM): unproject_one_kernel's read and arithmetic with the result of
// unproject_brick_kernel<..., ZD> at J = 1 - the cubes are never written.  `cubes` is the (P, 1, K, X/4, Y/4, 16) complex
// spectrum, K = ZDSZ/2+1; grids are not written (the entries refuse them), there is no pass mask.
//
// A workgroup owns one 4 x 4 tile of z columns over the whole z extent (Z == ZDZ == 20): 320 threads = 5 waves, wave = brick
// of 4 z layers, lane = voxel with the brick kernel's mapping (lx = lane/16, ly = (lane/4)%4, lz = lane%4), so a wave's 64
// voxels project onto neighbouring pixels.  X % 4 == Y % 4 == 0 and Z == 20 (resolve_one_zd): every lane has a voxel.
// Per lane the chunked gather of unproject_one_kernel, operation for operation: project_pk / make_record_pk, CS views' taps in
// flight while the next chunk is projected, the FMAs in view order, the wave-uniform view skip, fuse_rcp - the fused value has
// the bits unproject_one_kernel gives (a view no voxel of the wave sees adds an exact zero there, so the different voxels a
// wave holds change nothing for finite maps, as between the pipe and the brick kernels).  The gather is written out here a
// second time on purpose: as a function both kernels call it changed the instructions of every unproject_one_kernel
// instantiation (compared per kernel in the build's assembly), and those kernels are shipped as they are.
// The 320 fused values go to a 16 x 20 float slab in LDS (pos * 20 + z: 64 distinct banks per wave on the way in, 16 distinct
// 16-byte columns on the way out), one barrier, then 16 lanes run zdft_real<ZDZ, ZDSZ> on a column each - the table and FMA
// order of zdft_fwd_cl_kernel and the brick kernel's ZD epilogue, hence their bits - and store K float2 apiece: 16 lanes x
// 8 bytes = one whole 128-byte line per plane, at tile t = bx * (Y/4) + by whatever workgroup order the XCD map chose.
// A sample that `valid` skips writes its K all-zero lines.
//
// blockIdx -> (sample, tile): the grid is exactly P * tiles workgroups; block bid runs on XCD bid % 8, and XCD x takes the
// x-th eighth of the (sample, tile) sequence (tiles are x-major: a slab of the volume of one or two samples per XCD).
// ------------------------------------------------------------------------------------------
template <int VT, int CS, typename TI = float>
__global__ __launch_bounds__(64 * (ZDZ / BR)) void unproject_one_zd_kernel(Views hm, const float *__restrict__ cam,
                                                                          const float *__restrict__ centers,
                                                                          const uint8_t *__restrict__ valid,
                                                                          float *__restrict__ cubes, float *__restrict__ grids,
                                                                          Geom g, long long s_sample, int s_row, int s_px)
{
    constexpr int NCH = (VT + CS - 1) / CS;
    constexpr int K = ZDSZ / 2 + 1;
    extern __shared__ __attribute__((aligned(16))) float slab[];       // 16 columns x ZDZ floats (resolve_one_zd)
    (void)grids;
    // the x-th eighth of the g.B * g.xm_tiles (sample, tile) pairs, the first `total % 8` eighths one pair longer
    const int total = g.B * g.xm_tiles, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int lin = xcd * (total >> 3) + min(xcd, total & 7) + slot;
    int b, t;
    udiv_magic((uint32_t)lin, (uint32_t)g.xm_tiles, g.xm_magic_tiles, b, t);
    int bx, by;
    udiv_magic((uint32_t)t, (uint32_t)g.bk_nby, g.bk_magic_nby, bx, by);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2 *o = reinterpret_cast<float2 *>(cubes) + ((size_t)b * K * (size_t)g.xm_tiles + (size_t)t) * 16 + tid;
    const size_t kstride = (size_t)g.xm_tiles * 16;
    if (!valid[b]) {                                // skipped sample: its all-zero spectrum lines
        if (tid < 16) {
#pragma unroll
            for (int k = 0; k < K; ++k) o[(size_t)k * kstride] = make_float2(0.0f, 0.0f);
        }
        return;
    }
    const int bs = g.sample_of ? g.sample_of[b] : b;
    const int lx = lane >> 4, ly = (lane >> 2) & 3, lz = lane & 3;
    const int vx = bx * BR + lx, vy = by * BR + ly, vz = wave * BR + lz;
    {
        const float x = linspace_step(g.Lx, g.stepx, g.X, vx) + centers[3 * b + 0];
        const float y = linspace_step(g.Ly, g.stepy, g.Y, vy) + centers[3 * b + 1];
        const float z = linspace_step(g.Lz, g.stepz, g.Z, vz) + centers[3 * b + 2];
        const unsigned long long inbm = ~0ull;      // every lane has a voxel
        uint32_t mymask = 0;                        // views that see MY voxel (+ bit 31: NaN position)
        uint32_t have = 0;                          // wave-uniform: views with a record (some voxel of the wave sees them)
        uint32_t off[VT];                           // byte offset of the 2x2 block inside the sample's image
        float w00[VT], w10[VT], w01[VT], w11[VT];
        typename OneTap<TI>::raw t00[VT], t10[VT], t01[VT], t11[VT];
        const size_t pxb = (size_t)s_px * sizeof(TI), rowb = (size_t)s_row * sizeof(TI);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
            for (int c = ch * CS; c < (ch + 1) * CS && c < VT; ++c) {
                off[c] = 0u;
                w00[c] = w10[c] = w01[c] = w11[c] = 0.0f;
                if (c < g.V) {
                    const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
                    P1State st;
                    const bool go = project_pk(cm, g, x, y, z, inbm, st);
                    add_mask(mymask, st.bm);
                    if (st.nm != 0ull && lane_of(st.nm)) mymask |= 0x80000000u;
                    const unsigned long long um = st.bm & ~st.nm;
                    if (go && um != 0ull) {         // else: no voxel of this wave sees camera c
                        const RecPk r = make_record_pk(lane_of(um), st.i, g.w, g.h);
                        off[c] = (__umul24((unsigned)r.y0, (unsigned)s_row) + __umul24((unsigned)r.x0, (unsigned)s_px)) << OneTap<TI>::SHIFT;
                        w00[c] = r.wt.x; w10[c] = r.wt.y; w01[c] = r.wb.x; w11[c] = r.wb.y;
                        have |= 1u << c;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            // the chunk's taps as unproject_one_kernel issues them: wave-uniform bases, one 32-bit byte offset per lane, no
            // branch between the loads, in the reverse of the order the interpolation consumes them
#pragma unroll
            for (int c = min((ch + 1) * CS, VT) - 1; c >= ch * CS; --c) {
                const char *vb = reinterpret_cast<const char *>(reinterpret_cast<const TI *>(c < g.V ? hm.p[c] : hm.p[0]) + (ptrdiff_t)bs * s_sample);
                const char *vb2 = vb + rowb;
                t11[c] = OneTap<TI>::load(vb2 + pxb + off[c]);
                t01[c] = OneTap<TI>::load(vb2 + off[c]);
                t10[c] = OneTap<TI>::load(vb + pxb + off[c]);
                t00[c] = OneTap<TI>::load(vb + off[c]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < VT; ++c) {
            // ATen's bilinear chain: fma(se, wse, fma(sw, wsw, fma(ne, wne, nw * wnw)))
            float v = OneTap<TI>::value(t00[c]) * w00[c];
            v = fmaf(OneTap<TI>::value(t10[c]), w10[c], v);
            v = fmaf(OneTap<TI>::value(t01[c]), w01[c], v);
            v = fmaf(OneTap<TI>::value(t11[c]), w11[c], v);
            const float a = acc + v;
            acc = ((have >> c) & 1u) ? a : acc;     // wave-uniform, as the pipelined kernels skip such a view
        }
        // view fusion (project_layer.py:96-99): den = #views seeing the voxel + 1e-6; NaN sample position -> 0
        const float den = (float)(mymask & 0x7fffffffu) + 1e-6f;
        const float rden = (mymask & 0x80000000u) ? 0.0f : 1.0f / den;
        slab[(lane >> 2) * ZDZ + wave * BR + lz] = fuse_rcp(acc, den, rden);
    }
    __syncthreads();
    if (tid >= 16) return;
    float v[ZDZ];
#pragma unroll
    for (int wz = 0; wz < ZDZ / BR; ++wz) {
        const float4 q4 = *reinterpret_cast<const float4 *>(slab + tid * ZDZ + wz * BR);
        v[4 * wz] = q4.x; v[4 * wz + 1] = q4.y; v[4 * wz + 2] = q4.z; v[4 * wz + 3] = q4.w;
    }
    float re[K], im[K];
    zdft_real<ZDZ, ZDSZ>(v, re, im);
#pragma unroll
    for (int k = 0; k < K; ++k) o[(size_t)k * kstride] = make_float2(re[k], im[k]);
}

// ------------------------------------------------------------------------------------------
// one-channel backward (sp3d_unproject_one_bwd[_det]): the scatter of bwd2 for ONE gradient channel, into dense (V,B,h,w)
// planes instead of channel 0 of 16-byte pixels.  bwd2<4> runs this case on 16 of its 64 lanes and three of every four
// atomics it issues add the zero gradient of a pad channel; here lane = voxel throughout and every atomic carries a value.
//   pass 1   lane = voxel: sample_pos_fast per view -> view bits (+ bit 31: NaN position), den = popc + 1e-6
//            g = (bit 0 of the pass-mask word && !dead) ? grad / den : 0; a wave without any g != 0 ends here
//   pass 2   per view (wave-uniform loop, camera record in scalar registers): sample_pos_fast + make_record again - the
//            calls of bwd2's phase P1, so offset and weights are bwd2's - then up to four atomics g * w on the lanes that see
//            the view, each predicated on its weight.  Same fp32 products (grad / den) * w as bwd2: with DET the integers
//            added are the same, so the result equals channel 0 of sp3d_unproject_bwd_packed_det bit for bit.
// No LDS, no barrier: the record of a view lives in registers while its taps are issued.  grad_cubes: channel 0 of cube p is
// N contiguous floats at p * grad_stride (N for a (P,1,..) gradient, 4N for a planar (P,4,..) one).
// ------------------------------------------------------------------------------------------
template <bool DET>
__global__ __launch_bounds__(64) void unproject_one_bwd_kernel(const float *__restrict__ cam,
                                                              const float *__restrict__ centers,
                                                              const uint8_t *__restrict__ valid,
                                                              const float *__restrict__ grad_cubes, long long grad_stride,
                                                              const uint16_t *__restrict__ pass_mask,
                                                              void *__restrict__ grad_hm_, size_t view_stride, Geom g,
                                                              int tiles_per_sample, const float *__restrict__ scale_p)
{
    using ACC = typename std::conditional<DET, unsigned long long, float>::type;
    ACC *grad_hm = reinterpret_cast<ACC *>(grad_hm_);
    const double scale = DET ? (double)*scale_p : 1.0;
    auto add = [&](ACC *p, float val) {
        if constexpr (DET) atomicAdd(p, (unsigned long long)__double2ll_rn((double)val * scale));
        else unsafeAtomicAdd(p, val);
    };
    int b, tile;
    if (!xcd_map(blockIdx.x, g.B, tiles_per_sample, g.xcd_chunk, b, tile)) return;
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
    // the two loads of a voxel in flight while the views are projected (n is a valid voxel for every lane)
    const uint32_t pm = (uint32_t)pass_mask[(size_t)b * g.N + n];
    const float gl = grad_cubes[(size_t)b * (size_t)grad_stride + n];
    uint32_t mymask = 0;
    for (int c = 0; c < g.V; ++c) {
        const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
        float ix, iy;
        bool isnan;
        const bool bound = sample_pos_fast(cm, x, y, z, g, ix, iy, isnan) && inb;
        if (bound) mymask |= (1u << c);
        if (isnan && inb) mymask |= 0x80000000u;
    }
    // g = pass ? grad / den : 0     (autograd of project_layer.py:96-99)
    const float den = (float)__popc(mymask & 0x7fffffffu) + 1e-6f;
    const bool dead = (mymask & 0x80000000u) != 0 || (mymask & 0x7fffffffu) == 0;
    float gv = 0.0f;
    if (inb && !dead && (pm & 1u)) gv = gl / den;
    const uint32_t views = gv != 0.0f ? (mymask & 0x7fffffffu) : 0u;      // voxels without gradient scatter nothing
    if (__builtin_amdgcn_ballot_w64(views != 0u) == 0ull) return;
    ACC *gbase = grad_hm + (size_t)bs * g.h * g.w;
#pragma unroll 1
    for (int c = 0; c < g.V; ++c) {
        const float *cm = cam + ((size_t)bs * g.V + c) * SP3D_CAM_STRIDE;
        float ix, iy;
        bool isnan;
        const bool bound = sample_pos_fast(cm, x, y, z, g, ix, iy, isnan) && inb;
        const Rec r = make_record<1>(bound && !isnan, isnan ? 0.0f : ix, isnan ? 0.0f : iy, g.w, g.h);
        if ((views >> c) & 1u) {
            ACC *p = gbase + (size_t)c * view_stride + r.off;
            if (r.w00 != 0.0f) add(p, gv * r.w00);
            if (r.w10 != 0.0f) add(p + 1, gv * r.w10);
            if (r.w01 != 0.0f) add(p + g.w, gv * r.w01);
            if (r.w11 != 0.0f) add(p + g.w + 1, gv * r.w11);
        }
    }
}

// one-channel kernel: VT view slots gathered in chunks of CS
#define SP3D_ONE(VT_, CS_) SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .views = VT_, .chunk = CS_}), unproject_one_kernel, VT_, CS_, false) \
    SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .cl = true, .views = VT_, .chunk = CS_}), unproject_one_kernel, VT_, CS_, true) \
    SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .views = VT_, .chunk = CS_, .mask = true}), unproject_one_kernel, VT_, CS_, false, true) \
    SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .cl = true, .views = VT_, .chunk = CS_, .mask = true}), unproject_one_kernel, VT_, CS_, true, true)
// bf16 maps (SP3D_HM_BF16_IN): the same ladder, planar and channels-last results, no pass mask.  Tables of their
// own behind the fp32 ones, as find_brick_zspectrum32_kernel is behind find_brick_kernel
#define SP3D_ONE_H(VT_, CS_) SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .taps16 = 1, .views = VT_, .chunk = CS_}), unproject_one_kernel, VT_, CS_, false, false, bf16_t) \
    SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .cl = true, .taps16 = 1, .views = VT_, .chunk = CS_}), unproject_one_kernel, VT_, CS_, true, false, bf16_t)
static int find_one_h_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_ONE_H(1, 4) SP3D_ONE_H(2, 4) SP3D_ONE_H(3, 4) SP3D_ONE_H(4, 4) SP3D_ONE_H(5, 4) SP3D_ONE_H(6, 4) SP3D_ONE_H(8, 4)
    SP3D_ONE_H(10, 8) SP3D_ONE_H(12, 8) SP3D_ONE_H(16, 8)
    return SP3D_EUNSUPPORTED;
}

// bf16 maps into the training forward (SP3D_HM_BF16_TRAIN on sp3d_unproject_one_fwd_train): the MASK = true kernels with 2-byte
// taps, planar and channels-last results.  Behind the inference rows, as they are
// behind the fp32 ones; planned by tests/test_bf16_train_host.py, run by tests/test_gpu_bf16_train.py.
#define SP3D_ONE_H_TRAIN(VT_, CS_) SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .taps16 = 1, .views = VT_, .chunk = CS_, .mask = true}), unproject_one_kernel, VT_, CS_, false, true, bf16_t) \
    SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .cl = true, .taps16 = 1, .views = VT_, .chunk = CS_, .mask = true}), unproject_one_kernel, VT_, CS_, true, true, bf16_t)
static int find_one_h_train_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_ONE_H_TRAIN(1, 4) SP3D_ONE_H_TRAIN(2, 4) SP3D_ONE_H_TRAIN(3, 4) SP3D_ONE_H_TRAIN(4, 4) SP3D_ONE_H_TRAIN(5, 4)
    SP3D_ONE_H_TRAIN(6, 4) SP3D_ONE_H_TRAIN(8, 4) SP3D_ONE_H_TRAIN(10, 8) SP3D_ONE_H_TRAIN(12, 8) SP3D_ONE_H_TRAIN(16, 8)
    return SP3D_EUNSUPPORTED;
}

int find_one_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_ONE(1, 4) SP3D_ONE(2, 4) SP3D_ONE(3, 4) SP3D_ONE(4, 4) SP3D_ONE(5, 4) SP3D_ONE(6, 4) SP3D_ONE(8, 4) SP3D_ONE(10, 8)
    SP3D_ONE(12, 8) SP3D_ONE(16, 8)
    if (key.mask) return find_one_h_train_kernel(key, fn, name);
    return find_one_h_kernel(key, fn, name);
}

// the z-spectrum form (SP3D_HM_ONE_ZSPECTRUM): the same view slots and chunks
#define SP3D_ONE_ZD(VT_, CS_) SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .zd = true, .views = VT_, .chunk = CS_}), unproject_one_zd_kernel, VT_, CS_)
// ... and with bf16 maps (SP3D_HM_BF16_IN next to it)
#define SP3D_ONE_ZD_H(VT_, CS_) SP3D_ROW(OneFn, (KernelKey{.jp = 1, .ps = 1, .taps16 = 1, .zd = true, .views = VT_, .chunk = CS_}), unproject_one_zd_kernel, VT_, CS_, bf16_t)
static int find_one_zd_h_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_ONE_ZD_H(1, 4) SP3D_ONE_ZD_H(2, 4) SP3D_ONE_ZD_H(3, 4) SP3D_ONE_ZD_H(4, 4) SP3D_ONE_ZD_H(5, 4) SP3D_ONE_ZD_H(6, 4)
    SP3D_ONE_ZD_H(8, 4) SP3D_ONE_ZD_H(10, 8) SP3D_ONE_ZD_H(12, 8) SP3D_ONE_ZD_H(16, 8)
    return SP3D_EUNSUPPORTED;
}

int find_one_zd_kernel(const KernelKey &key, const void *&fn, const char *&name)
{
    SP3D_ONE_ZD(1, 4) SP3D_ONE_ZD(2, 4) SP3D_ONE_ZD(3, 4) SP3D_ONE_ZD(4, 4) SP3D_ONE_ZD(5, 4) SP3D_ONE_ZD(6, 4) SP3D_ONE_ZD(8, 4)
    SP3D_ONE_ZD(10, 8) SP3D_ONE_ZD(12, 8) SP3D_ONE_ZD(16, 8)
    return find_one_zd_h_kernel(key, fn, name);
}

} // namespace sp3d

using namespace sp3d;

// scale == nullptr: fp32 atomics into (V,B,h,w) float; else 64-bit fixed point into (V,B,h,w) int64
static int one_bwd_impl(const float *cam, const int32_t *sample_of, const float *centers, const uint8_t *valid,
                        const float *grad_cubes, int64_t grad_cube_stride, const uint16_t *pass_mask, void *grad_acc,
                        const float *scale, int B, int P, int V, int h, int w, int X, int Y, int Z, const float *grid_size,
                        int W_in, int H_in, void *stream)
{
    Geom g;
    const int rc = make_geom(g, P, V, 1, h, w, X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    if (B <= 0 || grad_cube_stride < (int64_t)g.N) return SP3D_EINVAL;
    if (!cam || !centers || !valid || !grad_cubes || !pass_mask || !grad_acc) return SP3D_ENULL;
    // a clamped 2x2 tap block needs a 2x2 image; its offset inside a plane is a 32-bit int of at most 2^24 pixels
    if (w < 2 || h < 2 || (int64_t)h * w > (1 << 24)) return SP3D_EUNSUPPORTED;
    g.sample_of = sample_of;
    const int tiles = (g.N + 63) / 64;
    const size_t view_stride = (size_t)B * h * w;
    const long long gstride = (long long)grad_cube_stride;
    dim3 grid(xcd_grid_blocks(P, tiles, g.xcd_chunk)), block(64);
    hipStream_t s = (hipStream_t)stream;
    if (scale)
        hipLaunchKernelGGL(unproject_one_bwd_kernel<true>, grid, block, 0, s, cam, centers, valid, grad_cubes, gstride, pass_mask,
                           grad_acc, view_stride, g, tiles, scale);
    else
        hipLaunchKernelGGL(unproject_one_bwd_kernel<false>, grid, block, 0, s, cam, centers, valid, grad_cubes, gstride, pass_mask,
                           grad_acc, view_stride, g, tiles, scale);
    return launch_status();
}

extern "C" int sp3d_unproject_one_bwd(const float *cam, const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                      const float *grad_cubes, int64_t grad_cube_stride, const uint16_t *pass_mask,
                                      float *grad_hm, int B, int P, int V, int h, int w, int X, int Y, int Z,
                                      const float *grid_size, int W_in, int H_in, void *stream)
{
    return one_bwd_impl(cam, sample_of, centers, valid, grad_cubes, grad_cube_stride, pass_mask, grad_hm, nullptr, B, P, V, h,
                        w, X, Y, Z, grid_size, W_in, H_in, stream);
}

extern "C" int sp3d_unproject_one_bwd_det(const float *cam, const int32_t *sample_of, const float *centers,
                                          const uint8_t *valid, const float *grad_cubes, int64_t grad_cube_stride,
                                          const uint16_t *pass_mask, int64_t *grad_fixed, const float *scale, int B, int P,
                                          int V, int h, int w, int X, int Y, int Z, const float *grid_size, int W_in, int H_in,
                                          void *stream)
{
    if (!scale) return SP3D_ENULL;
    return one_bwd_impl(cam, sample_of, centers, valid, grad_cubes, grad_cube_stride, pass_mask, grad_fixed, scale, B, P, V, h,
                        w, X, Y, Z, grid_size, W_in, H_in, stream);
}
