// sp3d_unproject_host.h - what the sources of the unprojection share on the host side: sp3d_unproject.hip (the launch plan
// and the forward entries) and the kernel files sp3d_unproject_tile.hip, _pipe.hip, _brick.hip, _one.hip, _bwd.hip.  The sizes
// both the kernels and the plan's grid / LDS arithmetic are written in, the Geom every entry starts from, and the kernel
// tables: a table takes the address of a kernel template, so each lives in the file that instantiates its kernels.
#ifndef SP3D_UNPROJECT_HOST_H
#define SP3D_UNPROJECT_HOST_H
#include <string.h>

#include "sp3d_device.h"

// measurement only (tools/diag_ablate.py builds one library per -DSP3D_ABLATE=<mask>, never shipped): compile-time
// switches that REMOVE one part of the pipelined kernels (results are then wrong on purpose) to see how the parts
// compose in time.  1: no result stores  2: no tap loads (FMAs run on zeros)  4: no projection (synthetic tap
// records)  8: staggered start (s_sleep by wave slot)  16: no FMAs
#ifndef SP3D_ABLATE
#define SP3D_ABLATE 0
#endif

namespace sp3d {

constexpr int TILE = 256; // voxels per workgroup (= threads per workgroup)
constexpr int OSTR = 260; // tile kernel: row stride (floats) of its result tile in LDS
// pipe and brick kernels, per wave (the layout is described at pipe_views, sp3d_unproject_pipe.h)
constexpr int WREC = 2 * 5 * 64;           // floats: weights [buf][voxel][4] (16-byte records), then offsets [buf][voxel]
constexpr int WOFF = 2 * 4 * 64;           // first offset word
constexpr int WOSTR = 68;                  // sOut row stride (floats), rows 16-B aligned
constexpr int BR = 4;                      // brick kernels: a wave owns BR x BR x BR voxels
constexpr int ZDZ = 20, ZDSZ = 28;         // brick kernel, z-spectrum result: z extent of the grid, length of the z transform
constexpr int WIDE_PS = 32;                // 17..32 joints: elements of a packed pixel, gathered and scattered as two channel groups

inline int make_geom(Geom &g, int B, int V, int J, int h, int w, int X, int Y, int Z, const float *grid_size,
                     int W_in, int H_in)
{
    if (B <= 0 || V <= 0 || J <= 0 || h <= 0 || w <= 0 || X <= 0 || Y <= 0 || Z <= 0 || W_in <= 0 || H_in <= 0)
        return SP3D_EINVAL;
    if (V > SP3D_MAX_VIEWS) return SP3D_EINVAL;
    if (!grid_size) return SP3D_ENULL;
    const int64_t N = (int64_t)X * Y * Z;
    if (N > (int64_t)0x7fffffff - TILE) return SP3D_ERANGE;
    if ((int64_t)B * ((N + TILE - 1) / TILE) > (int64_t)0x7fffffff - 8) return SP3D_ERANGE;
    if ((int64_t)h * w * 16 > (int64_t)0x7fffffff) return SP3D_ERANGE;
    g.B = B; g.V = V; g.J = J; g.h = h; g.w = w; g.X = X; g.Y = Y; g.Z = Z;
    g.sample_of = nullptr;
    g.pass_mask = nullptr;
    g.xcd_chunk = 1;
    g.xcd_order = 0;
    g.xm_mode = 2; g.xm_log2xps = g.xm_log2K = g.xm_rows = 0; g.xm_tiles = 1; g.xm_magic_tiles = 0;
    g.bk_nxy = g.bk_nby = 1; g.bk_magic_nxy = g.bk_magic_nby = 0;
    g.blk_log2py = 0; g.blk_w = g.blk_h = g.blk_nbx = g.blk_nzc = 1; g.blk_magic_wh = g.blk_magic_h = 0;
    g.N = (int)N; g.YZ = Y * Z; g.W_in = W_in; g.H_in = H_in;
    g.sB = (long long)J * N; g.sJ = (int)N; g.sX = Y * Z; g.sY = Z; g.dense = 1; g.vec4 = 1;
    g.Lx = grid_size[0]; g.Ly = grid_size[1]; g.Lz = grid_size[2];
    g.rW_in = 1.0f / (float)W_in; g.rH_in = 1.0f / (float)H_in;
    g.rw1 = w > 1 ? 1.0f / (float)(w - 1) : 0.0f; g.rh1 = h > 1 ? 1.0f / (float)(h - 1) : 0.0f;
    {   // torch.linspace step in fp32: (end - start) / (n - 1) with start = -(L/2), end = L/2
        const float L[3] = {g.Lx, g.Ly, g.Lz};
        const int n[3] = {X, Y, Z};
        float st[3];
        for (int a = 0; a < 3; ++a) {
            volatile float start = -(L[a] / 2.0f), end = L[a] / 2.0f;
            volatile float diff = end - start;
            st[a] = n[a] > 1 ? diff / (float)(n[a] - 1) : 0.0f;
        }
        g.stepx = st[0]; g.stepy = st[1]; g.stepz = st[2];
    }
    g.magicYZ = (uint32_t)((0x100000000ull / (uint64_t)(Y * Z)) + 1ull);
    g.magicZ = (uint32_t)((0x100000000ull / (uint64_t)Z) + 1ull);
    return SP3D_OK;
}

inline int load_views(Views &v, const float *const *hm_views, int V)
{
    if (!hm_views) return SP3D_ENULL;
    for (int c = 0; c < SP3D_MAX_VIEWS; ++c) v.p[c] = nullptr;
    for (int c = 0; c < V; ++c) {
        if (!hm_views[c]) return SP3D_ENULL;
        v.p[c] = hm_views[c];
    }
    return SP3D_OK;
}

// Kernel tables, one per kernel signature.  A row is a key, the kernel and its printable name (as a kernel trace shows it,
// without namespace and parameter list), all three from the same template arguments.  A missing row is SP3D_EUNSUPPORTED.
// The tables are written as functions, a row being one `if`: an array of kernel pointers and names in a shared object is
// relocated, hence writable, data, and the library keeps none (tests/test_host_cabi.py).
// A key is plain ints compared with memcmp.  It is spelled with its field names, in the order below; a field that is not named
// is zero - a family names exactly what its template varies in.
struct KernelKey {
    int jp, ps, cl;         // channels gathered; channels between pixels; channels-last result
    int taps16, cubes16;    // 2-byte (bf16) heat-map taps; 2-byte result
    int xcd, unroll, waves; // tile, pipe: XCD-aware tile map; tile: voxels in flight per lane; pipe: waves per workgroup
    int zd;                 // brick, one-channel: z-spectrum result
    int views, chunk, mask; // one-channel: view slots; how many of them a gather chunk holds; the kernel that also writes the pass mask
};
template <typename T> constexpr int is16() { return sizeof(T) == 2 ? 1 : 0; }
using PackFn = void (*)(Views, float *, int, int, int);
using PlanarFn = void (*)(Views, const float *, const float *, const uint8_t *, float *, float *, Geom);
using TileFn = void (*)(Views, const float *, const float *, const uint8_t *, float *, float *, Geom, int, int);   // tile and pipe
using BrickFn = void (*)(Views, const float *, const float *, const uint8_t *, float *, float *, Geom, int, int, int, int);
using OneFn = void (*)(Views, const float *, const float *, const uint8_t *, float *, float *, Geom, long long, int, int);

inline bool same_key(const KernelKey &a, const KernelKey &b) { return !memcmp(&a, &b, sizeof(a)); }

#define SP3D_ROW(FN_, KEY_, K_, ...) \
    if (same_key(key, KEY_)) \
        return fn = reinterpret_cast<const void *>(static_cast<FN_>(K_<__VA_ARGS__>)), name = #K_ "<" #__VA_ARGS__ ">", SP3D_OK;

// the tables; sp3d_unproject_<family>.hip defines find_<family>_kernel (the tile file also the planar and the pack rows)
int find_planar_kernel(const KernelKey &key, const void *&fn, const char *&name);
int find_pack_kernel(const KernelKey &key, const void *&fn, const char *&name);
int find_tile_kernel(const KernelKey &key, const void *&fn, const char *&name);
int find_pipe_kernel(const KernelKey &key, const void *&fn, const char *&name);
int find_brick_kernel(const KernelKey &key, const void *&fn, const char *&name);
int find_one_kernel(const KernelKey &key, const void *&fn, const char *&name);
int find_one_zd_kernel(const KernelKey &key, const void *&fn, const char *&name);

#ifdef SP3D_TIMELINE
// measurement builds only: the timeline buffer is a __device__ variable, and one of those cannot cross files (the library
// is built without relocatable device code), so the two files whose kernels stamp keep a copy each
int set_pipe_timeline(unsigned long long *dev_buffer);
int set_brick_timeline(unsigned long long *dev_buffer);
#endif

} // namespace sp3d
#endif
