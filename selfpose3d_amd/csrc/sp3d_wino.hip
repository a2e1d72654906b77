// sp3d_wino.hip - input / output transforms of Winograd F(2x2x2, 3x3x3) for the low-resolution 3x3x3 convolutions
// of the V2V nets in inference (reference: the `Res3DBlock`s of lib/models/v2v_net.py:23-45 at 1/4 resolution).
// The FALLBACK FORM of that tier since sp3d_conv3_quarter.hip: grids of up to 64 whole 5x5x5 blocks (the headline 20x20x5 at
// batch 4) run as one direct kernel per layer (route "conv3_split128_" of v2v_net.conv3_route); the route "wino_conv3d_", these
// three launches behind _lib.wino_conv3d_, is what every other grid, widths other than (64 | 128) -> 128 and SP3D_QUARTER_DIRECT=0 get.
//
// At 1/4 resolution (20x20x5 voxels, 128 channels, batch 4) a 3x3x3 convolution is a GEMM with only 8 000 rows;
// MIOpen's implicit-GEMM kernels reach 60 TFLOP/s there (112 us per layer).  Winograd needs 64 multiplies per 8 outputs
// instead of 216, as 64 independent (tiles x C) x (C x O) products - one batched fp32 GEMM (rocBLAS through torch.bmm,
// 36 us) - between two memory-bound transforms, which are these kernels:
//   wino_input : channels-last activations (B,X,Y,Z,C) -> V[64][tiles][C],  V = B^T d B  along each axis
//   wino_output: M[64][tiles][O] -> channels-last (B,X,Y,Z,O), y = A^T m A, fused with the layer's epilogue
//                (shift [+ residual] [+ ReLU], the modes of sp3d_channel_shift_act)
// lane = channel (coalesced 4-byte accesses across the channel-contiguous layouts), one thread = one (tile, channel).
// The weight transform U = G g G^T is done once per plan on the host side of the binding (torch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sp3d.h"
#include "sp3d_conv3_host.h"

namespace sp3d {

__device__ __forceinline__ void bt4(float &d0, float &d1, float &d2, float &d3)
{
    const float t0 = d0 - d2, t1 = d1 + d2, t2 = d2 - d1, t3 = d1 - d3;
    d0 = t0; d1 = t1; d2 = t2; d3 = t3;
}

__global__ __launch_bounds__(256) void wino_input_kernel(const float *__restrict__ x, float *__restrict__ V, int B, int X,
                                                        int Y, int Z, int C, int TX, int TY, int TZ)
{
    const int64_t T = (int64_t)B * TX * TY * TZ;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= T * C) return;
    const int c = (int)(gid % C);
    int64_t t = gid / C;
    const int tz = (int)(t % TZ); int64_t r = t / TZ;
    const int ty = (int)(r % TY); r /= TY;
    const int tx = (int)(r % TX);
    const int b = (int)(r / TX);
    float d[4][4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int xi = 2 * tx - 1 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yj = 2 * ty - 1 + j;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int zk = 2 * tz - 1 + k;
                const bool in = xi >= 0 && xi < X && yj >= 0 && yj < Y && zk >= 0 && zk < Z;
                d[i][j][k] = in ? x[((((int64_t)b * X + xi) * Y + yj) * Z + zk) * C + c] : 0.0f;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) bt4(d[i][j][0], d[i][j][1], d[i][j][2], d[i][j][3]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) bt4(d[i][0][k], d[i][1][k], d[i][2][k], d[i][3][k]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) bt4(d[0][j][k], d[1][j][k], d[2][j][k], d[3][j][k]);
    const int64_t plane = T * C;
    float *v = V + t * C + c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[(int64_t)((i * 4 + j) * 4 + k) * plane] = d[i][j][k];
}

template <int MODE>
__global__ __launch_bounds__(256) void wino_output_kernel(const float *__restrict__ M, float *__restrict__ y,
                                                         const float *__restrict__ shift, const float *__restrict__ res,
                                                         int B, int X, int Y, int Z, int O, int TX, int TY, int TZ)
{
    const int64_t T = (int64_t)B * TX * TY * TZ;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= T * O) return;
    const int o = (int)(gid % O);
    int64_t t = gid / O;
    const int tz = (int)(t % TZ); int64_t r = t / TZ;
    const int ty = (int)(r % TY); r /= TY;
    const int tx = (int)(r % TX);
    const int b = (int)(r / TX);
    const int64_t plane = T * O;
    const float *m = M + t * O + o;
    // A^T along x while loading: two rows of (4 x 4)
    float a[2][4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float m0 = m[(int64_t)((0 * 4 + j) * 4 + k) * plane], m1 = m[(int64_t)((1 * 4 + j) * 4 + k) * plane];
            const float m2 = m[(int64_t)((2 * 4 + j) * 4 + k) * plane], m3 = m[(int64_t)((3 * 4 + j) * 4 + k) * plane];
            a[0][j][k] = (m0 + m1) + m2;
            a[1][j][k] = (m1 - m2) - m3;
        }
    const float sh = shift[o];
    // residual values first (clamped addresses, no predicate): inside the bounds branches below each was a load -> wait ->
    // store round trip of its own
    float rv[2][2][2];
    if (MODE >= 2) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int xo = min(2 * tx + i, X - 1), yo = min(2 * ty + j, Y - 1), zo = min(2 * tz + k, Z - 1);
                    rv[i][j][k] = res[((((int64_t)b * X + xo) * Y + yo) * Z + zo) * O + o];
                }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float bq[2][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bq[0][k] = (a[i][0][k] + a[i][1][k]) + a[i][2][k];
            bq[1][k] = (a[i][1][k] - a[i][2][k]) - a[i][3][k];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float c0 = (bq[j][0] + bq[j][1]) + bq[j][2], c1 = (bq[j][1] - bq[j][2]) - bq[j][3];
            const int xo = 2 * tx + i, yo = 2 * ty + j;
            if (xo >= X || yo >= Y) continue;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int zo = 2 * tz + k;
                if (zo >= Z) continue;
                const int64_t idx = ((((int64_t)b * X + xo) * Y + yo) * Z + zo) * O + o;
                float v = (k == 0 ? c0 : c1) + sh;
                if (MODE == 2) v += rv[i][j][k];
                if (MODE >= 1) v = fmaxf(v, 0.0f);
                if (MODE == 3) v += rv[i][j][k];
                y[idx] = v;
            }
        }
    }
}

} // namespace sp3d

using namespace sp3d;

extern "C" int sp3d_wino_input(const float *x, float *V, int B, int X, int Y, int Z, int C, void *stream)
{
    if (C <= 0) return SP3D_EINVAL;
    const Conv3Grid t = conv3_grid(B, X, Y, Z, 2, 2, 2);
    const int64_t n = t.blocks * C;
    if (const int rc = conv3_check(B, X, Y, Z, 0, x && V, true, (n + 255) / 256 <= 0x7fffffff)) return rc;
    hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, V, B, X, Y, Z,
                       C, t.NBX, t.NBY, t.NBZ);
    return launch_status();
}

extern "C" int sp3d_wino_output(const float *M, float *y, const float *shift, const float *residual, int mode, int B, int X,
                                int Y, int Z, int O, void *stream)
{
    if (O <= 0) return SP3D_EINVAL;
    const Conv3Grid t = conv3_grid(B, X, Y, Z, 2, 2, 2);
    const int64_t n = t.blocks * O;
    if (const int rc = conv3_check(B, X, Y, Z, mode, M && y && shift && (mode < 2 || residual), true, (n + 255) / 256 <= 0x7fffffff))
        return rc;
    with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL((wino_output_kernel<decltype(m)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, M, y, shift, residual, B, X, Y, Z, O, t.NBX, t.NBY, t.NBZ);
    });
    return launch_status();
}
