// sp3d_upconv.hip - ConvTranspose3d(kernel 2, stride 2) + BatchNorm + ReLU + skip (+ the 1x1x1 output conv) of the V2V
// decoder (lib/models/v2v_net.py:57-69, 100-108, 128-133) in ONE kernel.
//
// The layer has no overlapping taps: output voxel (2x+i, 2y+j, 2z+k) depends on input voxel (x,y,z) only, so it is the
// product G[n, (tap, o)] = X[n, :] . W[:, (tap, o)] followed by a scatter.  sp3d_upsample2x_scatter(_head) takes G from a
// library GEMM, i.e. G (8*O floats per input voxel: 65.5 MB at 40x40x10 -> 80x80x20, batch 4) is written to memory and read
// back.  Here the product is formed on the bf16 matrix pipe with the exact three-piece splits of sp3d_split.h (the six
// piece products of conv3_split_kernel, fp32 accumulation) and the epilogue runs on the accumulators: what moves is x,
// the skip tensor and the result.
//
// Workgroup = 4 waves = 128 consecutive input voxels (32 per wave) x a range of taps.  Lane (t,h) of a wave loads voxel t,
// channels 8 kc + 4 h .. + 3 of the 8-channel chunks kc of one 64-channel K stage, splits them once and keeps the A
// operands in registers (6 dwords per chunk: 48).  CIN = 64 is one K stage: loaded once, used for every tap.  CIN = 128
// re-loads its two K stages per tap (the 8 tap workgroups of a tile run side by side: x comes from the L2) - with all 128
// channels resident the kernel needed more than 256 registers.
// Per tap the wave holds one f32x16 accumulator per 32 output channels (32 voxels x 32 channels, lane (t,h) = channel t,
// rows m = 8 (v >> 2) + (v & 3) + 4 h), so one store instruction writes two full 128-byte voxel rows.
// Weights: pre-split on the host (_lib.upconv_weights_split), 48-byte records {bh,bl} {bh,bh} {bm,bm} of 4 channels at
// index ((((tap*(O/32) + ob)*(CIN/8) + kc)*2 + half)*32 + o.  The four waves share them through LDS in stages of
// (tap, ob, 64 channels of K) = 24 576 B, two buffers: the next stage is fetched to registers before the matrix
// instructions of the current one and written to the other buffer after them; one barrier per stage.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sp3d.h"
#include "sp3d_device.h"
#include "sp3d_split.h"

namespace sp3d {

constexpr int UC_STAGE = 8 * 2 * 32 * 3;               // u32x4 per stage: 8 chunks x 2 lane halves x 32 outputs x 48 B
constexpr int UC_PER = UC_STAGE / 256;                 // u32x4 per thread and stage: 6
constexpr int UC_SCR = 33;                             // row pitch of the head's per-wave scratch: lane = voxel reads hit 32 banks

// grid: blockIdx.x = tile * ny + tap group (the tap groups of a tile are neighbours in launch order)
// MULTI: a workgroup walks more than one tap (taps_per_block > 1) and fetches the next tap's skip rows ahead
template <int CIN, int O, bool HEAD, bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void upconv2x_fused_kernel(
    const float *__restrict__ x, const u32x4 *__restrict__ W, const float *__restrict__ shift, const float *__restrict__ skip,
    const float *__restrict__ wout, const float *__restrict__ bout, float *__restrict__ out, int n_in, int X, int Y, int Z, int J,
    int ny, int taps_per_block)
{
    constexpr int KS = CIN / 64, OB = O / 32, SPT = KS * OB;          // weight stages per tap, in the order (ks, ob)
    extern __shared__ __attribute__((aligned(16))) u32x4 uc_lds[];     // 2 x UC_STAGE, then (HEAD) 4 x 32 x UC_SCR + 32 x 32 + 32 floats
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = lane & 31, h = lane >> 5;
    const int tile = (int)blockIdx.x / ny;
    const int tap0 = ((int)blockIdx.x % ny) * taps_per_block;
    const int n0 = tile * 128 + wave * 32;
    const int nvalid = n_in - n0;                                      // voxels of this wave inside the tensor (<= 0: none)
    const int nstages = taps_per_block * SPT;

    float *scr = reinterpret_cast<float *>(uc_lds + 2 * UC_STAGE) + wave * 32 * UC_SCR;
    float *wo = reinterpret_cast<float *>(uc_lds + 2 * UC_STAGE) + 4 * 32 * UC_SCR;      // [J][32], then the bias [32]
    if (HEAD) {
        for (int i = tid; i < J * 32; i += 256) wo[i] = wout[i];
        if (tid < 32) wo[32 * 32 + tid] = (bout && tid < J) ? bout[tid] : 0.0f;
    }

    // stage q of this workgroup = (tap0 + q / SPT, ks = (q % SPT) / OB, ob = q % OB): UC_STAGE consecutive u32x4, 6 per thread
    u32x4 wreg[UC_PER];
    auto fetch = [&](int q) {
        const int tap = tap0 + q / SPT, ks = (q % SPT) / OB, ob = q % OB;
        const u32x4 *p = W + (int64_t)((tap * OB + ob) * KS + ks) * UC_STAGE + tid;
#pragma unroll
        for (int r = 0; r < UC_PER; ++r) wreg[r] = p[256 * r];
    };
    auto stash = [&](int buf) {
        u32x4 *p = uc_lds + buf * UC_STAGE + tid;
#pragma unroll
        for (int r = 0; r < UC_PER; ++r) p[256 * r] = wreg[r];
    };
    fetch(0);

    // A operands of K stage ks: voxel n0 + t (clamped: rows past the end compute on a copy of the last voxel, never stored)
    const int na = min(n0 + t, n_in - 1);
    const float *xp = x + (int64_t)na * CIN + 4 * h;
    u32x6 ap[8];                                                       // [lo hi mid]: {lo,hi} = dwords 0..3, {hi,mid} = 2..5
    auto load_a = [&](int ks) {
        float4 d[8];
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) d[kc] = *reinterpret_cast<const float4 *>(xp + 64 * ks + 8 * kc);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) ap[kc] = split3_pieces(d[kc]);
    };
    if (KS == 1) load_a(0);
    // output voxel of tap (0,0,0) of input voxel n0 + t (clamped); tap (i,j,k) adds ((i 2Y) + j) 2Z + k
    int base;
    {
        int n = na;
        const int z = n % Z; n /= Z;
        const int y = n % Y; n /= Y;
        const int xx = n % X;
        const int b = n / X;
        base = ((b * 2 * X + 2 * xx) * 2 * Y + 2 * y) * 2 * Z + 2 * z;
    }
    // accumulator rows of this lane: voxels m(v) = 8 (v >> 2) + (v & 3) + 4 h, as 32-bit element offsets of their O channels
    // (sp3d_upconv2x_fused refuses tensors of 2^31 elements and more: one address register per row instead of two)
    unsigned vb[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) vb[v] = (unsigned)__shfl(base, 8 * (v >> 2) + (v & 3) + 4 * h) * O + t;

    auto tap_off = [&](int tap) { return (((tap >> 2) * 2 * Y) + ((tap >> 1) & 1)) * 2 * Z + (tap & 1); };
    float sk[OB][16];
    auto fetch_skip = [&](int tap, int ob) {               // skip rows of (tap, ob), in the accumulator's layout
        const int toff = tap_off(tap);
#pragma unroll
        for (int v = 0; v < 16; ++v) sk[ob][v] = skip[vb[v] + (unsigned)(toff * O + ob * 32)];
    };
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) fetch_skip(tap0, ob);
    stash(0);
    __syncthreads();

    int buf = 0, q = 0;
    for (int tap = tap0; tap < tap0 + taps_per_block; ++tap) {
        const int toff = tap_off(tap);
        f32x16 acc[OB];
#pragma unroll
        for (int ob = 0; ob < OB; ++ob)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[ob][v] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (KS > 1) load_a(ks);
#pragma unroll
            for (int ob = 0; ob < OB; ++ob, ++q) {
                // unconditional (the last stage fetches itself again, into the buffer nobody reads): no branch around the loads
                fetch(min(q + 1, nstages - 1));
                const u32x4 *wl = uc_lds + buf * UC_STAGE + (h * 32 + t) * 3;
#pragma unroll
                for (int kc = 0; kc < 8; ++kc) {
                    const u32x4 hl = wl[kc * 192], hh = wl[kc * 192 + 1], mm = wl[kc * 192 + 2];
                    acc[ob] = mfma_bf16(split3_q0(ap[kc]), hl, acc[ob]);
                    acc[ob] = mfma_bf16(split3_q1(ap[kc]), hh, acc[ob]);
                    acc[ob] = mfma_bf16(split3_q1(ap[kc]), mm, acc[ob]);
                }
                if (ks == KS - 1) {
                    // ---- epilogue of (tap, ob), straight from the accumulators: relu(acc + shift) + skip ----
                    const float sh = shift[ob * 32 + t];
                    const unsigned ob_off = (unsigned)(toff * O + ob * 32);
                    float val[16];
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const float a = acc[ob][v] + sh;
                        val[v] = (a < 0.0f ? 0.0f : a) + sk[ob][v];    // NaN propagates like torch.relu
                    }
                    // the next tap's skip rows are requested before this tap's stores (loads queued behind stores wait for them)
                    // (a workgroup's last tap asks for its own rows again - no branch around the loads: one cost the CIN = 128
                    // kernel 18 spilled registers; MULTI = false, one tap per workgroup, has no next tap and asks for nothing)
                    if (MULTI) fetch_skip(min(tap + 1, tap0 + taps_per_block - 1), ob);
                    if (!HEAD) {
                        if (nvalid >= 32) {
#pragma unroll
                            for (int v = 0; v < 16; ++v) out[vb[v] + ob_off] = val[v];
                        } else {
#pragma unroll
                            for (int v = 0; v < 16; ++v)
                                if (8 * (v >> 2) + (v & 3) + 4 * h < nvalid) out[vb[v] + ob_off] = val[v];
                        }
                    } else {
                        // head[voxel][j] = bout[j] + sum_o wout[j][o] val[voxel][o]: the tile goes through the wave's scratch and
                        // comes back as lane = (voxel t, channel half h), 16 channels each; the two halves meet in one exchange
#pragma unroll
                        for (int v = 0; v < 16; ++v) scr[(8 * (v >> 2) + (v & 3) + 4 * h) * UC_SCR + t] = val[v];
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        float c[16];
#pragma unroll
                        for (int i = 0; i < 16; ++i) c[i] = scr[t * UC_SCR + 16 * h + i];
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        float *hp = out + (unsigned)(base + toff) * (unsigned)J;
                        const bool mine = h == 0 && t < nvalid;
                        for (int j = 0; j < J; ++j) {
                            const float *wj = wo + j * 32 + 16 * h;
                            float p = 0.0f;
#pragma unroll
                            for (int i4 = 0; i4 < 4; ++i4) {
                                const float4 w4 = *reinterpret_cast<const float4 *>(wj + 4 * i4);
                                p = fmaf(c[4 * i4 + 3], w4.w, fmaf(c[4 * i4 + 2], w4.z, fmaf(c[4 * i4 + 1], w4.y, fmaf(c[4 * i4], w4.x, p))));
                            }
                            p += __shfl_xor(p, 32);
                            if (mine) hp[j] = p + wo[32 * 32 + j];
                        }
                    }
                }
                stash(buf ^ 1);
                __syncthreads();
                buf ^= 1;
            }
        }
    }
}

} // namespace sp3d

extern "C" int sp3d_upconv2x_fused(const float *x, const void *w_split, const float *shift, const float *skip,
                                   const float *w_out, const float *b_out, float *out, int64_t batch, int X, int Y, int Z,
                                   int CIN, int O, int J, void *stream)
{
    using namespace sp3d;
    const bool head = w_out != nullptr;
    if (batch <= 0 || X <= 0 || Y <= 0 || Z <= 0 || CIN <= 0 || O <= 0 || (head && (J <= 0 || J > 32))) return SP3D_EINVAL;
    if (!x || !w_split || !shift || !skip || !out) return SP3D_ENULL;
    if (!((CIN == 64 && O == 32 && head) || (CIN == 128 && O == 64 && !head))) return SP3D_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_split)) & 15) return SP3D_EUNSUPPORTED;
    const int64_t n_in = batch * X * Y * Z;
    if (n_in * 8 * (head && J > O ? J : O) > 0x7fffffff) return SP3D_ERANGE;      // element offsets are 32-bit in the kernel
    const int tiles = (int)((n_in + 127) / 128);
    // 256 CUs with two workgroups resident on each (LDS: 70 KB with the head; registers: two waves per SIMD).  The 8 taps
    // are split over workgroups until there are about two per CU; a split re-reads and re-splits x, so no further.
    //   64 -> 32 + head at 40x40x10, batch 4: 500 tiles x 1 workgroup of 8 taps;
    //   128 -> 64 at 20x20x5, batch 4: 63 tiles x 8 workgroups of one tap (x per tap comes from the L2 either way).
    int ny = 1;
    while (ny < 8 && (int64_t)tiles * ny < 480) ny *= 2;
    const dim3 grid((unsigned)(tiles * ny)), block(256);
    const size_t lds = (size_t)2 * UC_STAGE * 16 + (head ? (size_t)(4 * 32 * UC_SCR + 32 * 32 + 32) * sizeof(float) : 0);
    hipStream_t s = (hipStream_t)stream;
    const u32x4 *w = reinterpret_cast<const u32x4 *>(w_split);
    if (head) {
        // more than 64 KB of dynamic LDS: the attribute is per device and remembered per device, as sp3d_conv3_split does
        // (devices past the table share its last slot and set the attribute on every call; two threads that both find the
        // flag clear both set the same value)
        int dev = 0;
        { const hipError_t ed = hipGetDevice(&dev); if (ed != hipSuccess) return (int)ed; }
        if (dev < 0 || dev >= 64) dev = 63;
        const bool multi = ny < 8;
        const auto kern = multi ? upconv2x_fused_kernel<64, 32, true, true> : upconv2x_fused_kernel<64, 32, true, false>;
        static bool attr_dev[2][64] = {};
        if (!attr_dev[multi][dev] || dev == 63) {
            const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (ea != hipSuccess) return (int)ea;
            attr_dev[multi][dev] = true;
        }
        hipLaunchKernelGGL(kern, grid, block, lds, s, x, w, shift, skip, w_out, b_out, out, (int)n_in, X, Y, Z, J, ny, 8 / ny);
    } else {
        const auto kern = ny < 8 ? upconv2x_fused_kernel<128, 64, false, true> : upconv2x_fused_kernel<128, 64, false, false>;
        hipLaunchKernelGGL(kern, grid, block, lds, s, x, w, shift, skip, w_out, b_out, out, (int)n_in, X, Y, Z, 0, ny, 8 / ny);
    }
    return sp3d::launch_status();
}
