// sp3d_conv3_host.h - what the sources of the 3x3x3 convolutions share (sp3d_wino.hip, sp3d_wino_fused.hip,
// sp3d_conv3_direct.hip).  Device side: the measurement switch and the ReLU of the kernels that fold a skip projection.
// Host side: the pieces every C entry of the three files is made of - the argument check in the ABI's return-code order,
// the grid of output blocks and the run-time mode as a compile-time constant (the launch epilogue is sp3d_device.h's).
#ifndef SP3D_CONV3_HOST_H
#define SP3D_CONV3_HOST_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/sp3d.h"
#include "sp3d_device.h"

#ifndef SP3D_W16_ABLATE
#define SP3D_W16_ABLATE 0      // measurement builds only (tools/diag_w16.py): 1 no MFMA, 2 no weight loads, 4 no split, 8 no LDS reads
#endif

namespace sp3d {

// ReLU of the kernels that fold a skip projection: a NaN of the projection's input stays a NaN (torch.relu); fmaxf, which
// the other instantiations keep, returns 0 for it
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.0f ? 0.0f : v; }

// The check every entry makes before its first HIP call, in the order the ABI documents: sizes and mode (SP3D_EINVAL), the
// pointers the mode needs (SP3D_ENULL), widths and alignments the kernels are built for (SP3D_EUNSUPPORTED), index range
// (SP3D_ERANGE).  The three conditions are the entry's own; an entry without a mode passes the one it launches.
inline int conv3_check(int B, int X, int Y, int Z, int mode, bool pointers, bool supported, bool in_range)
{
    if (B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || mode < 0 || mode > 3) return SP3D_EINVAL;
    if (!pointers) return SP3D_ENULL;
    if (!supported) return SP3D_EUNSUPPORTED;
    return in_range ? SP3D_OK : SP3D_ERANGE;
}

// output blocks of bx x by x bz voxels over B volumes of X x Y x Z; a launch needs blocks <= 0x7fffffff
struct Conv3Grid { int NBX, NBY, NBZ; int64_t blocks; };
inline Conv3Grid conv3_grid(int B, int X, int Y, int Z, int bx, int by, int bz)
{
    const int NBX = (X + bx - 1) / bx, NBY = (Y + by - 1) / by, NBZ = (Z + bz - 1) / bz;
    return {NBX, NBY, NBZ, (int64_t)B * NBX * NBY * NBZ};
}

// epilogue mode 0..3 (validated) -> f(std::integral_constant<int, mode>), whose ::value names a kernel instantiation
template <int V> using int_c = std::integral_constant<int, V>;
template <class F> inline auto with_mode(int mode, F &&f)
{
    switch (mode) {
    case 0: return f(int_c<0>{});
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    default: return f(int_c<3>{});
    }
}

// the quarter-resolution widths of sp3d_conv3_split, (C, O) = (64 | 128, 128): validation and launch of conv3_split128_kernel
// (sp3d_conv3_quarter.hip), same arguments and return codes
int conv3_split128(const float *x, const void *W3, float *y, const float *shift, const float *residual, int mode, int B, int X,
                   int Y, int Z, int C, int O, void *stream);

} // namespace sp3d
#endif
