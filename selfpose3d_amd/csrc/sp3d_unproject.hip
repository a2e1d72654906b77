// sp3d_unproject.hip - ProjectLayer.get_voxel, host side: the forward launch plan and the forward C-ABI entry points
// (include/sp3d.h).  Pure host arithmetic: the kernels are in the files of their families,
//   sp3d_unproject_tile.hip   unproject_planar_kernel, pack_nhwc_kernel, unproject_nhwc_kernel; sp3d_pack_heatmaps[_ex]
//   sp3d_unproject_pipe.hip   unproject_pipe_kernel
//   sp3d_unproject_brick.hip  unproject_brick_kernel, unproject_brick_h_kernel
//   sp3d_unproject_one.hip    unproject_one_kernel, unproject_one_zd_kernel, unproject_one_bwd_kernel; sp3d_unproject_one_bwd[_det]
//   sp3d_unproject_bwd.hip    unproject_bwd_kernel, unproject_bwd2_kernel, unproject_bwd3_kernel; sp3d_unproject_bwd*
// and this file reaches them through the kernel tables sp3d_unproject_host.h declares.
//
// Reference path: lib/models/project_layer.py:42-102 of the reference and its helpers
// lib/utils/cameras.py:27-55, lib/utils/transforms.py:119-123.  The reference runs this as a
// Python batch x view loop of ~90 tiny kernels; here one launch covers the whole batch.
//
// Also here, because they belong to no kernel family: sp3d_abi_version, sp3d_camera_finish, sp3d_error_string and the
// measurement entries of sp3d_tuning.h.
#include <stdio.h>
#include <string.h>

#include "sp3d_tuning.h"
#include "sp3d_unproject_host.h"

namespace sp3d {

// ------------------------------------------------------------------------------------------
// Forward unprojection, host side: an entry's arguments -> decode_fwd() -> FwdRequest -> resolve_fwd() -> launch records -> launch_fwd().
// ------------------------------------------------------------------------------------------
// The tuning word of sp3d_unproject_fwd_variant, decoded: one field per bit group documented in sp3d_tuning.h (the only
// place the word's layout is written down).  All int, no padding: tunings compare with memcmp.
struct FwdTuning {
    int unroll;          // tile kernel: voxels in flight per lane (1, 2, 4)
    int no_xcd_map;      // tile / pipe kernels: plain blockIdx order instead of the XCD-aware tile map
    int pipe;            // per-wave software-pipelined kernel (unproject_pipe_kernel)
    int one_wave;        // pipe kernel: one wave per workgroup instead of four
    int brick;           // 4x4x4 voxels per wave, a z-stack of bricks per workgroup
    int brick_own_wg;    // every brick its own workgroup
    int z_fastest;       // z-fastest chunk order (xcd_order bit 1); the bricks keep the chunk map
    int view_sync;       // round-5 L1-residency experiment (measurement only): view-synchronous brick workgroups
    int ballast;         // same experiment: n * 20 KB of unused LDS per brick workgroup caps the workgroups resident on a CU
    int forced_chunk;    // log2(tiles per XCD chunk) + 1; 0: the default chunk size
    int plain_sweep;     // chunks in sweep order instead of centre first
    int chunk_map;       // bricks: round-5 chunk map instead of blocks / octants
};

static FwdTuning decode_tuning(int variant)
{
    FwdTuning t;
    t.unroll = (variant & 3) == 0 ? 1 : ((variant & 3) == 2 ? 4 : 2);
    t.no_xcd_map = (variant >> 2) & 1;
    t.pipe = (variant >> 3) & 1;
    t.one_wave = (variant >> 4) & 1;
    t.brick = (variant >> 5) & 1;
    t.brick_own_wg = (variant >> 6) & 1;
    t.z_fastest = (variant >> 8) & 1;
    t.view_sync = (variant >> 10) & 1;
    t.ballast = (variant >> 11) & 7;
    t.forced_chunk = (variant >> 17) & 15;
    t.plain_sweep = (variant >> 21) & 1;
    t.chunk_map = (variant >> 22) & 1;
    return t;
}

// The three defaults.  All: pipelined, one wave per workgroup, XCD-aware tile map, centre-first chunks of the default size.
enum FwdDefault { FWD_PIPE, FWD_BRICK_STACKS, FWD_BRICK_EACH };
static FwdTuning default_tuning(FwdDefault d)
{
    FwdTuning t = {};
    t.unroll = t.pipe = t.one_wave = 1;
    t.brick = d != FWD_PIPE;
    t.brick_own_wg = d == FWD_BRICK_EACH;
    return t;
}
// Default kernel per result layout and grid (profiles/r02_ab_brick.json, same-box A/B, bit-identical results):
//   channels-last result     4x4x4 bricks, one brick per workgroup: -5 % on the root grid, -20 % on 64^3 person
//                            cubes, -30 % on the 160x160x40 grid - fewer distinct 128-B lines per wave-load
//   planar result, Z % 32==0 brick stacks of 8: the workgroup store writes whole 128-B z-runs (64^3 cubes: -20 %)
//   planar result, other Z   64 consecutive voxels per wave: a 20- or 40-voxel z-run does not fill store lines from a
//                            brick stack, and the stack's barrier costs more than the gather saves (root grid: +30 %)
static FwdTuning default_tuning(const Geom &g, bool out_cl)
{
    return default_tuning(out_cl ? FWD_BRICK_EACH : (g.Z % 32 == 0 ? FWD_BRICK_STACKS : FWD_PIPE));
}

// What a forward entry asks for, in the terms the kernels are chosen by (decode_fwd below writes it, from an entry's arguments
// or from the plan entry's).  `g` carries J, the image, the grid and the result strides; the entry adds sample_of and pass_mask.
enum Read { READ_PLANAR, READ_PACKED, READ_ONE_PLANAR, READ_ONE_PACKED, READ_UNKNOWN };    // READ_ONE_*: SP3D_HM_ONE_CHANNEL / _ONE_ZSPECTRUM
enum Result { RESULT_PLANAR, RESULT_CHANNELS_LAST, RESULT_ZSPECTRUM };                    // planar: dense or strided, Geom has the strides
enum Mask { MASK_NONE, MASK_ONE_PLANE, MASK_TWO_PLANES };                                  // two: SP3D_HM_WIDE_MASK, a plane per channel group
struct FwdRequest {
    int entry;              // SP3D_PLAN_*: which entry asks
    Read read; Result result; Mask mask;
    int taps16, cubes16;    // element types of the kernels: 2-byte taps (SP3D_HM_BF16, _BF16_IN, _BF16_TRAIN), 2-byte result (SP3D_OUT_BF16)
    int Jp;                 // packed: elements of a pixel; one channel: pixel stride (packed) or channel count (planar)
    Geom g;
};
static bool one_channel(const FwdRequest &rq) { return rq.read == READ_ONE_PLANAR || rq.read == READ_ONE_PACKED; }
// the pipelined kernels clamp a 2x2 block (needs a 2x2 image) and form pixel indices with 24-bit multiplies
static bool has_2x2(const Geom &g) { return g.w >= 2 && g.h >= 2; }
static bool pipelined_image(const Geom &g) { return has_2x2(g) && (int64_t)g.h * g.w <= (1 << 24); }

// What an entry knows from its pointers and the plan entry can only state (all there, aligned, no grids, SZ as built)
struct CallFacts {
    bool ptrs, views, grids;    // every required pointer but the views is there; hm_views and its V entries are there; `grids` was given
    unsigned misaligned;        // the result address modulo 128
    int SZ;                     // sp3d_unproject_fwd_zdft only: the length of the z transform asked for
};

// one kernel launch.  scalar[0..nscalars): the kernel arguments after Geom, each in a 64-bit slot - an `int` parameter
// reads the low half of its slot (little-endian host), the one-channel kernel's `long long` all of it
struct Launch {
    const void *fn;
    const char *name;
    unsigned grid, grid_y, block;
    size_t lds;
    Geom g;
    int nscalars;
    long long scalar[4];
    size_t view_off, out_off;    // second channel group of Jp = 32: byte offsets of its views and its result; it writes no grids
    bool grids;
};

static void set_launch(Launch &L, unsigned grid, unsigned block, size_t lds, int nscalars, long long s0, int s1, int s2 = 0, int s3 = 0)
{
    L.grid = grid; L.block = block; L.lds = lds;
    L.nscalars = nscalars; L.scalar[0] = s0; L.scalar[1] = s1; L.scalar[2] = s2; L.scalar[3] = s3;
}

// Default chunk size of the XCD tile map for 64-voxel tiles: 2-4 chunks per serving XCD - compact enough that an XCD's
// L2 sees a fraction of each view (fabric reads 93 MB -> 81 MB on the bench workload), fine enough to balance visibility
static int default_xcd_chunk(const Geom &g, int tiles)
{
    const int xps = (g.B <= 8 && (8 % g.B) == 0) ? 8 / g.B : 1;
    int k = 1;
    while (k * 2 * xps * 2 <= tiles) k *= 2;
    return k;
}

// Default chunk order: centre of the volume first (cheap edge tiles form the tail) when a sample is spread over >= 4 XCDs
// (-2.5 % at B = 1); with 2 XCDs per sample it buys no time and costs L2 locality (HBM-side reads 75 -> 92 MB on the bench
// workload), so the plain sweep stays there
static int default_xcd_order(const Geom &g) { return g.B <= 2 ? 1 : 0; }

// One NHWC launch of `jp` channels read at a pixel stride of `ps`: brick, pipe or tile kernel, its grid and its Geom.
// `t` is final here (resolve_fwd applied the downgrades).  A missing table row is the refusal.
static int resolve_group(const FwdRequest &rq, const FwdTuning &t, const Geom &g, int jp, int ps, Launch &L)
{
    const int wlds = jp * WOSTR > WREC ? jp * WOSTR : WREC;      // per-wave LDS floats of the pipe and brick kernels
    const int cl = rq.result == RESULT_CHANNELS_LAST;
    L.g = g;
    if (t.brick) {   // 4x4x4 voxels per wave, a z-stack of `zw` bricks per workgroup
        const int nbx = (g.X + BR - 1) / BR, nby = (g.Y + BR - 1) / BR, nwz = (g.Z + BR - 1) / BR;
        int nzc = (nwz + 7) / 8, zw = (nwz + nzc - 1) / nzc;
        if (t.brick_own_wg) { zw = 1; nzc = nwz; }
        const int wgs = nbx * nby * nzc;
        // 2-4 chunks of consecutive workgroups (x-slabs of the volume) per serving XCD
        L.g.xcd_chunk = t.forced_chunk ? 1 << (t.forced_chunk - 1) : default_xcd_chunk(g, wgs);
        set_xcd_fields(L.g, wgs);
        set_brick_fields(L.g, nbx * nby, nby);
        // default since round 6 (B in {1, 2, 4}): one block of brick columns per XCD - octants at B = 1, quadrants at B = 2,
        // halves at B = 4 - instead of round-robin chunks; same results, L2 fills 138 -> 60 MB on the 160x160x40 grid,
        // 75 -> 56 MB on the root grid at B = 4 (profiles/r06_pmc_blocks.json).  The chunk-map tuning restores the chunks.
        const int block_grid = (t.chunk_map || t.z_fastest) ? 0 : set_block_fields(L.g, nbx, nby, nzc);
        // view-synchronous workgroups only when every wave of every workgroup lies inside the volume, so that all of them
        // reach the per-view barrier
        if (t.view_sync && nwz % zw == 0 && nzc * zw == nwz) L.g.xcd_order |= 4;
        set_launch(L, block_grid ? block_grid : xcd_grid_blocks(g.B, wgs, L.g.xcd_chunk), 64 * zw,
                   (size_t)zw * wlds * sizeof(float) + (size_t)t.ballast * 20480, 4, wgs, nby, nzc, zw);
        return find_brick_kernel(KernelKey{.jp = jp, .ps = ps, .cl = cl, .taps16 = rq.taps16, .cubes16 = rq.cubes16, .zd = rq.result == RESULT_ZSPECTRUM}, L.fn, L.name);
    }
    if (t.pipe) {    // 64 consecutive voxels per wave
        const int nw = t.one_wave ? 1 : 4;
        const int ptiles = (g.N + 64 * nw - 1) / (64 * nw), ptotal = ptiles * g.B;
        set_xcd_fields(L.g, ptiles);
        set_launch(L, t.no_xcd_map ? ptotal : xcd_grid_blocks(g.B, ptiles, g.xcd_chunk), 64 * nw, 0, 2, ptiles, ptotal);
        return find_pipe_kernel(KernelKey{.jp = jp, .ps = ps, .cl = cl, .taps16 = rq.taps16, .cubes16 = rq.cubes16, .xcd = !t.no_xcd_map, .waves = nw}, L.fn, L.name);
    }
    const int tiles = (g.N + TILE - 1) / TILE, total = tiles * g.B;
    set_launch(L, t.no_xcd_map ? total : xcd_grid_blocks(g.B, tiles, g.xcd_chunk), TILE,
               (size_t)(jp * OSTR + 2 * g.V * TILE + TILE) * sizeof(float), 2, tiles, total);
    return find_tile_kernel(KernelKey{.jp = jp, .ps = ps, .cl = cl, .taps16 = rq.taps16, .cubes16 = rq.cubes16, .xcd = !t.no_xcd_map, .unroll = t.unroll}, L.fn, L.name);
}

// The one-channel reads (SP3D_HM_ONE_CHANNEL, SP3D_HM_ONE_ZSPECTRUM; include/sp3d.h).  Their kernels take the sample stride, the
// row stride and the pixel stride of the tensor the channel lies in, and exist per view-slot count, gathered in chunks.
static int64_t one_px(const FwdRequest &rq) { return rq.read == READ_ONE_PACKED ? rq.Jp : 1; }
static void set_one_launch(const FwdRequest &rq, Launch &L, unsigned grid, unsigned block, size_t lds)
{
    const Geom &g = L.g;
    const int64_t row = g.w * one_px(rq);
    set_launch(L, grid, block, lds, 3, rq.read == READ_ONE_PACKED ? g.h * row : (int64_t)rq.Jp * g.h * g.w, (int)row, (int)one_px(rq));
}
static KernelKey one_slots_key(const FwdRequest &rq)
{
    const int V = rq.g.V, vt = V <= 6 ? V : (V <= 8 ? 8 : (V <= 10 ? 10 : (V <= 12 ? 12 : 16)));
    return KernelKey{.jp = 1, .ps = 1, .cl = rq.result == RESULT_CHANNELS_LAST, .taps16 = rq.taps16, .zd = rq.result == RESULT_ZSPECTRUM,
                     .views = vt, .chunk = vt > 8 ? 8 : 4, .mask = rq.mask != MASK_NONE};
}

// The one place a decoded request becomes launches: the downgrades, and the refusals of packed pixels that follow from the
// tuning and the kernel tables.  Pure host arithmetic.
static int resolve_fwd(const FwdRequest &rq, FwdTuning t, Launch (&plan)[SP3D_PLAN_RECORDS], int &n)
{
    n = 1;
    Launch &L = plan[0];
    L = Launch{};
    L.g = rq.g; L.grid_y = 1; L.grids = rq.result != RESULT_ZSPECTRUM;      // a z-spectrum launch writes no grids (its entries take none)
    Geom g = rq.g;
    if (one_channel(rq) && rq.result == RESULT_ZSPECTRUM) {
        // unproject_one_zd_kernel: one workgroup of ZDZ / BR waves per 4 x 4 tile of z columns, exactly P * tiles of them (the
        // kernel deals them to the XCDs itself), a slab of 16 x ZDZ floats of LDS
        const int nby = g.Y / BR, tiles = (g.X / BR) * nby;
        set_xcd_fields(L.g, tiles);
        set_brick_fields(L.g, tiles, nby);
        set_one_launch(rq, L, (unsigned)(g.B * tiles), 64 * (ZDZ / BR), (size_t)16 * ZDZ * sizeof(float));
        return find_one_zd_kernel(one_slots_key(rq), L.fn, L.name);
    }
    if (one_channel(rq)) {
        // unproject_one_kernel: g.J = channels written (1, or 4 = value + three zero channels), the pipe kernel's tile map -
        // 64-voxel tiles dealt to a sample's XCDs in chunks
        const int ptiles = (g.N + 63) / 64;
        L.g.xcd_order = default_xcd_order(g);
        L.g.xcd_chunk = default_xcd_chunk(g, ptiles);
        set_xcd_fields(L.g, ptiles);
        set_one_launch(rq, L, xcd_grid_blocks(g.B, ptiles, L.g.xcd_chunk), 64, 0);
        return find_one_kernel(one_slots_key(rq), L.fn, L.name);
    }
    if (rq.read == READ_PLANAR) {
        set_launch(L, (g.N + TILE - 1) / TILE, TILE, 0, 0, 0, 0);
        L.grid_y = g.B;
        const int jc = g.J == 1 ? 1 : (g.J <= 4 ? 4 : 16);
        return find_planar_kernel(KernelKey{.jp = jc, .ps = jc}, L.fn, L.name);
    }
    g.xcd_order = (t.plain_sweep ? 0 : default_xcd_order(g)) | (t.z_fastest ? 2 : 0);
    g.xcd_chunk = t.forced_chunk ? 1 << (t.forced_chunk - 1) : default_xcd_chunk(g, (g.N + 63) / 64);
    const FwdTuning asked = t, pipe = default_tuning(FWD_PIPE), stacks = default_tuning(FWD_BRICK_STACKS);
    const bool tile_only = !pipelined_image(g);
    if (rq.result == RESULT_ZSPECTRUM) g.sB = (long long)g.J * (ZDSZ / 2 + 1) * (g.X / BR) * (g.Y / BR) * 16;
    if (tile_only) t.pipe = t.brick = 0;
    if (t.brick) t.pipe = 1;
    if (rq.taps16 || rq.cubes16) t.one_wave = 1;    // bf16 taps or cubes: one wave per workgroup only
    if (rq.Jp != WIDE_PS) {
        if (rq.Jp < g.J || (rq.Jp & 3) || rq.Jp > 16) return SP3D_EUNSUPPORTED;
        return resolve_group(rq, t, g, rq.Jp, rq.Jp, L);
    }
    // Jp = 32 (17..32 joints: the 17 COCO joints of the Shelf / Campus configurations).  A packed fp32 pixel is exactly one
    // 128-byte line.  It is gathered as two channel groups, one launch each, both reading pixels at a stride of PS = 32:
    //   group 0   channels 0-15 through the JP = 16 kernel;
    //   group 1   channels 16..J-1 through a launch of width ceil4(J - 16) (16 with bf16 maps or cubes, whose kernels
    //             exist at JP = 16 only).  Its view pointers start 16 channels into the pixel (the wave-uniform row base moves,
    //             no VGPR does), its result pointer 16 channel planes further, and its Geom has J - 16 channels.
    // The per-channel arithmetic is the 16-channel kernels', so each group is bit-identical to the oracle by construction.  Only
    // group 0 writes grids; a sample that `valid` skips gets zeros in each group.  Planar results only (dense or strided: the
    // strided path already carries full-volume strides), the two planar defaults only (pipe / brick stacks).  A pass mask only
    // in two planes (SP3D_HM_WIDE_MASK): each group writes the 16-bit words of its own channels into its own plane of P * N
    // words - group 1's mask pointer lies P * N words further, bit j of its words being channel 16 + j.
    // RESULT_ZSPECTRUM: the same two groups through the ZD brick kernels.  The spectrum is (P, J, K, X/4, Y/4, 16) complex over
    // ALL J channels, so the sample stride comes from here (Geom.sB, in complex elements - the ZD form reads no other result
    // stride) and group 1 starts 16 channel planes = 16 * K * (X/4) * (Y/4) * 16 complex values further.
    if (g.J > WIDE_PS || rq.result == RESULT_CHANNELS_LAST || rq.mask == MASK_ONE_PLANE || tile_only) return SP3D_EUNSUPPORTED;
    if (memcmp(&asked, &pipe, sizeof(t)) && memcmp(&asked, &stacks, sizeof(t))) return SP3D_EUNSUPPORTED;
    Geom gg = g;
    gg.J = g.J < 16 ? g.J : 16;
    int rc = resolve_group(rq, t, gg, 16, WIDE_PS, L);
    if (rc || g.J <= 16) return rc;
    Launch &L1 = plan[n++];
    L1 = L;
    gg.J = g.J - 16;
    if (g.pass_mask) gg.pass_mask = g.pass_mask + (size_t)g.B * g.N;
    L1.view_off = 16 * (rq.taps16 ? 2 : 4);
    L1.out_off = rq.result == RESULT_ZSPECTRUM ? (size_t)16 * (ZDSZ / 2 + 1) * (g.X / BR) * (g.Y / BR) * 16 * 8
                                               : (size_t)16 * g.sJ * (rq.cubes16 ? 2 : 4);
    L1.grids = false;
    return resolve_group(rq, t, gg, (rq.taps16 || rq.cubes16) ? 16 : (gg.J + 3) / 4 * 4, WIDE_PS, L1);
}

// the one place a forward kernel is launched
static int launch_fwd(Launch L, Views v, const float *cam, const float *centers, const uint8_t *valid, float *cubes,
                      float *grids, hipStream_t s)
{
    for (int c = 0; c < SP3D_MAX_VIEWS; ++c)
        if (v.p[c]) v.p[c] = reinterpret_cast<const float *>(reinterpret_cast<const char *>(v.p[c]) + L.view_off);
    cubes = reinterpret_cast<float *>(reinterpret_cast<char *>(cubes) + L.out_off);
    if (!L.grids) grids = nullptr;
    if (L.lds > 65536) {     // only the LDS ballast gets there
        const hipError_t ea = hipFuncSetAttribute(L.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds);
        if (ea != hipSuccess) return (int)ea;
    }
    void *args[12] = {&v, &cam, &centers, &valid, &cubes, &grids, &L.g};
    for (int i = 0; i < L.nscalars; ++i) args[7 + i] = &L.scalar[i];
    (void)hipLaunchKernel(L.fn, dim3(L.grid, L.grid_y), dim3(L.block), args, L.lds, s);
    return launch_status();
}

// result strides of sp3d_unproject_fwd_strided into the Geom; 16-byte pieces are allowed on a 16-byte aligned result only
static int set_result_strides(Geom &g, const int64_t *out_strides, unsigned misaligned)
{
    const int64_t sB = out_strides[0], sJ = out_strides[1], sX = out_strides[2], sY = out_strides[3];
    // the planes must not overlap and must fit 32-bit in-plane offsets
    if (sY < g.Z || sX < (int64_t)g.Y * sY || sJ < (int64_t)g.X * sX || sB < (int64_t)g.J * sJ) return SP3D_EINVAL;
    if (sJ > 0x7fffffff) return SP3D_ERANGE;
    g.sB = sB; g.sJ = (int)sJ; g.sX = (int)sX; g.sY = (int)sY;
    g.dense = (sY == g.Z && sX == (int64_t)g.Y * g.Z && sJ == (int64_t)g.N && sB == (int64_t)g.J * g.N) ? 1 : 0;
    // 16-byte pieces need 4-element aligned rows (and a 16-byte aligned base pointer); otherwise the kernels take their
    // scalar store path, which is correct for any stride but slow
    g.vec4 = ((g.dense || ((sY | sX | sJ | sB) & 3) == 0) && (misaligned & 15) == 0) ? 1 : 0;
    return SP3D_OK;
}

// ------------------------------------------------------------------------------------------
// The rules: which request an entry's arguments spell, or why none (include/sp3d.h gives the same rules as prose, flag by flag).
// Two tables of plain ints and two functions for what a table cannot hold.  Every entry and the plan entry decode through them.
// ------------------------------------------------------------------------------------------
enum : int { F_CL = SP3D_OUT_CHANNELS_LAST, F_HB = SP3D_HM_BF16, F_OB = SP3D_OUT_BF16, F_ONE = SP3D_HM_ONE_CHANNEL, F_WM = SP3D_HM_WIDE_MASK,
             F_ZS = SP3D_OUT_ZSPECTRUM, F_OZ = SP3D_HM_ONE_ZSPECTRUM, F_IN16 = SP3D_HM_BF16_IN, F_TR16 = SP3D_HM_BF16_TRAIN, F_ALL = 0x1ff00 };

// Per entry, in the order of SP3D_PLAN_*: the layout byte it reads (-1: the caller's), the flags it implies, the flags it does not
// read, the flags it refuses outright, and whether it writes a pass mask.  The last two entries take no layout word; what their
// plans answer for a word with flag bits is written here, and nowhere else: the word's layout byte is not read, sp3d_unproject_fwd_zdft
// refuses four flags and ignores the rest, sp3d_unproject_fwd_variant refuses one, ignores the rest and takes F_CL from its tuning word.
struct EntryRule { int layout, implied, unread, refused, mask; };
static const EntryRule ENTRY_RULES[] = {
    /* _INDEXED   */ {-1, 0, 0, 0, 0},
    /* _STRIDED   */ {-1, 0, 0, F_CL | F_ZS | F_OZ, 0},
    /* _TRAIN     */ {-1, 0, 0, F_HB | F_OB | F_ONE | F_ZS | F_OZ | F_IN16, 1},
    /* _ZDFT      */ {SP3D_LAYOUT_NHWC, F_ZS, F_CL | F_HB | F_OB | F_ONE | F_ZS, F_WM | F_OZ | F_IN16 | F_TR16, 0},
    /* _TUNING    */ {SP3D_LAYOUT_NHWC, 0, F_ALL & ~F_TR16, F_TR16, 0},
    /* _ONE_TRAIN */ {-1, F_ONE, 0, F_ZS | F_OZ | F_IN16, 1},
};
// Per flag: the flags that may stand next to it, the flags one of which must, and whether it needs an entry with a pass mask.
// Rows 0-3 are answered before the layout byte is (SP3D_EINVAL), the others after it - see decode_fwd.
struct FlagRule { int flag, beside, one_of, mask; };
static const FlagRule FLAG_RULES[] = {
    {F_TR16, F_CL | F_ONE | F_WM, 0, 1},
    {F_IN16, F_CL | F_ONE | F_ZS | F_OZ, F_ONE | F_ZS | F_OZ, 0},
    {F_WM, F_TR16, 0, 1},
    {F_ZS, F_IN16, 0, 0},
    {F_OZ, F_IN16, 0, 0},
    {F_ONE, F_CL | F_IN16 | F_TR16, 0, 0},
    {F_CL, F_HB | F_OB | F_ONE | F_IN16 | F_TR16, 0, 0},
    {F_HB, F_CL | F_OB, 0, 0},
    {F_OB, F_CL | F_HB, 0, 0},
};

// the one-channel kernels form the tap offset with 24-bit multiplies and address it with a 32-bit byte offset
static bool one_addressable(const FwdRequest &rq)
{
    const int64_t row = rq.g.w * one_px(rq);
    return pipelined_image(rq.g) && row < (1 << 24) && rq.g.h * row * (rq.taps16 ? 2 : 4) <= (int64_t)0x7fffffff;
}
// the layout, Jp, J, image and grid a flag needs
static bool flag_needs(int flag, const FwdRequest &rq, const CallFacts &f)
{
    const Geom &g = rq.g;
    const bool zgrid = g.Z == ZDZ && g.X % BR == 0 && g.Y % BR == 0;         // the one grid shape the z-DFT is built for
    switch (flag) {
    case F_CL: return rq.read != READ_PLANAR && (g.J & 3) == 0 && (!one_channel(rq) || (f.misaligned & 15) == 0);   // rows of 16-B multiples
    case F_HB: case F_OB: return rq.read == READ_PACKED;
    case F_ONE: return (g.J == 1 || g.J == 4) && one_addressable(rq);
    case F_WM: return rq.read == READ_PACKED && rq.Jp == WIDE_PS;
    case F_ZS: return rq.read == READ_PACKED && (rq.Jp == 16 || rq.Jp == WIDE_PS) && zgrid && pipelined_image(g);
    case F_OZ: return g.J == 1 && zgrid && g.dense && one_addressable(rq);
    case F_TR16:     // the one-channel read has F_ONE's limits; packed pixels of 16 elements, or of 32 with the two-plane mask
        return rq.read != READ_PLANAR && (rq.read != READ_PACKED || (rq.Jp == (rq.mask == MASK_TWO_PLANES ? WIDE_PS : 16) && pipelined_image(g)));
    default: return true;
    }
}
static bool breaks(const FlagRule &r, int flags, const FwdRequest &rq, const CallFacts &f)
{
    return (flags & r.flag) && ((flags & ~r.flag & ~r.beside) || (r.one_of && !(flags & r.one_of)) || (r.mask && rq.mask == MASK_NONE) ||
                                !flag_needs(r.flag, rq, f));
}
// what an entry needs beyond its row: of its layout byte, its image and its pointers
static bool entry_needs(const FwdRequest &rq, int flags, const CallFacts &f)
{
    switch (rq.entry) {
    case SP3D_PLAN_INDEXED: return !(flags & (F_ZS | F_OZ)) || (!f.grids && !f.misaligned);    // a spectrum: whole 128-byte lines, no grids
    case SP3D_PLAN_STRIDED: return (rq.read == READ_PACKED || (flags & F_ONE)) && has_2x2(rq.g);   // the one-channel read takes either layout
    case SP3D_PLAN_TRAIN: return rq.read == READ_PACKED && has_2x2(rq.g);
    case SP3D_PLAN_ZDFT: return rq.Jp == 16 && f.SZ == ZDSZ && !f.misaligned && flag_needs(F_ZS, rq, f);
    default: return true;
    }
}

struct Shape { int B, V, J, h, w, X, Y, Z; const float *grid_size; int W_in, H_in; };      // the shape arguments every entry has
// (entry, its arguments, the facts about its pointers) -> the request and its tuning, or the refusal.  The order is the order of
// the return codes: the shape (make_geom), required pointers, the entry's own rule, the result strides, the views, the flags
// answered before the layout byte, the layout byte, everything else.
static int decode_fwd(FwdRequest &rq, FwdTuning &t, int entry, int hm_layout, int Jp, const int64_t *out_strides, int variant,
                      const CallFacts &f, const Shape &s)
{
    int rc = make_geom(rq.g, s.B, s.V, s.J, s.h, s.w, s.X, s.Y, s.Z, s.grid_size, s.W_in, s.H_in);
    if (rc) return rc;
    if (!f.ptrs) return SP3D_ENULL;
    const EntryRule &e = ENTRY_RULES[entry];
    const int layout = e.layout < 0 ? (hm_layout & 0xff) : e.layout;
    const int flags = (hm_layout & F_ALL & ~e.unread) | e.implied | ((entry == SP3D_PLAN_TUNING && (variant & SP3D_TUNING_CHANNELS_LAST)) ? F_CL : 0);
    const bool one = (flags & (F_ONE | F_OZ)) != 0;
    rq.entry = entry; rq.Jp = Jp;
    rq.read = layout == SP3D_LAYOUT_PLANAR ? (one ? READ_ONE_PLANAR : READ_PLANAR)
                                           : (layout == SP3D_LAYOUT_NHWC ? (one ? READ_ONE_PACKED : READ_PACKED) : READ_UNKNOWN);
    rq.result = (flags & (F_ZS | F_OZ)) ? RESULT_ZSPECTRUM : ((flags & F_CL) ? RESULT_CHANNELS_LAST : RESULT_PLANAR);
    rq.mask = !e.mask ? MASK_NONE : ((flags & F_WM) ? MASK_TWO_PLANES : MASK_ONE_PLANE);
    rq.taps16 = (flags & (F_HB | F_IN16 | F_TR16)) ? 1 : 0;
    rq.cubes16 = (flags & F_OB) ? 1 : 0;
    // a spectrum: the brick stacks as sp3d_unproject_fwd_zdft (the one-channel form has one kernel, the tuning is not read)
    t = rq.result == RESULT_ZSPECTRUM ? default_tuning(one ? FWD_PIPE : FWD_BRICK_STACKS) : default_tuning(rq.g, rq.result == RESULT_CHANNELS_LAST);
    if (entry == SP3D_PLAN_TUNING) t = decode_tuning(variant);
    if ((hm_layout & e.refused) || !entry_needs(rq, flags, f)) return SP3D_EUNSUPPORTED;
    if (entry == SP3D_PLAN_STRIDED && out_strides && (rc = set_result_strides(rq.g, out_strides, f.misaligned))) return rc;
    if (!f.views) return SP3D_ENULL;
    const int early = (flags & F_OZ) ? 1 : 4;       // the one-channel spectrum answers its layout byte before its other refusals
    for (int i = 0; i < early; ++i)
        if (breaks(FLAG_RULES[i], flags, rq, f)) return SP3D_EUNSUPPORTED;
    if (rq.read == READ_UNKNOWN || (one && Jp < 1)) return SP3D_EINVAL;
    for (const FlagRule &r : FLAG_RULES)
        if (breaks(r, flags, rq, f)) return SP3D_EUNSUPPORTED;
    return SP3D_OK;
}

// What every forward entry is: the facts about its pointers, decode_fwd, the two pointers the Geom carries, the views, the plan,
// its launches.  `ptrs`: every required pointer but the views is there.
static int run_entry(int entry, int hm_layout, int Jp, const int64_t *out_strides, int variant, int SZ, const Shape &s, bool ptrs,
                     const float *const *hm_views, const float *cam, const int32_t *sample_of, const float *centers, const uint8_t *valid,
                     float *cubes, float *grids, uint16_t *pass_mask, void *stream)
{
    bool views = hm_views != nullptr;
    for (int c = 0; views && c < s.V && c < SP3D_MAX_VIEWS; ++c) views = hm_views[c] != nullptr;
    FwdRequest rq;
    FwdTuning t;
    int rc = decode_fwd(rq, t, entry, hm_layout, Jp, out_strides, variant,
                        CallFacts{ptrs && cam && centers && valid && cubes, views, grids != nullptr, (unsigned)((uintptr_t)cubes & 127), SZ}, s);
    if (rc) return rc;
    rq.g.sample_of = sample_of;
    rq.g.pass_mask = pass_mask;
    Views v;
    Launch plan[SP3D_PLAN_RECORDS];
    int n;
    if ((rc = load_views(v, hm_views, s.V)) || (rc = resolve_fwd(rq, t, plan, n))) return rc;
    // two mask planes at J <= 16: no second group, so nobody writes plane 1 - it is zeros
    if (rq.mask == MASK_TWO_PLANES && n == 1)
        rc = (int)hipMemsetAsync(pass_mask + (size_t)s.B * rq.g.N, 0, (size_t)s.B * rq.g.N * sizeof(uint16_t), (hipStream_t)stream);
    for (int i = 0; !rc && i < n; ++i) rc = launch_fwd(plan[i], v, cam, centers, valid, cubes, grids, (hipStream_t)stream);
    return rc;
}

} // namespace sp3d

using namespace sp3d;

extern "C" int sp3d_abi_version(void) { return SP3D_ABI_VERSION; }

extern "C" int sp3d_camera_finish(float *t, int records)
{
    if (!t) return SP3D_ENULL;
    if (records < 0) return SP3D_EINVAL;
    for (int r = 0; r < records; ++r, t += SP3D_CAM_STRIDE) {
        for (int c = 0; c < 3; ++c) {
            t[SP3D_CAM_RXY + 2 * c] = t[SP3D_CAM_R + c]; t[SP3D_CAM_RXY + 2 * c + 1] = t[SP3D_CAM_R + 3 + c];
            t[SP3D_CAM_AXY + 2 * c] = t[SP3D_CAM_A + c]; t[SP3D_CAM_AXY + 2 * c + 1] = t[SP3D_CAM_A + 3 + c];
            t[SP3D_CAM_RZ + c] = t[SP3D_CAM_R + 6 + c];
            t[SP3D_CAM_K2 + c] = t[SP3D_CAM_K + c];
        }
        t[SP3D_CAM_TXY] = t[SP3D_CAM_T]; t[SP3D_CAM_TXY + 1] = t[SP3D_CAM_T + 1]; t[SP3D_CAM_TZ] = t[SP3D_CAM_T + 2];
        t[SP3D_CAM_P2] = t[SP3D_CAM_P]; t[SP3D_CAM_P2 + 1] = t[SP3D_CAM_P + 1];
        t[SP3D_CAM_F2] = t[SP3D_CAM_F]; t[SP3D_CAM_F2 + 1] = t[SP3D_CAM_F + 1];
        t[SP3D_CAM_C2] = t[SP3D_CAM_C]; t[SP3D_CAM_C2 + 1] = t[SP3D_CAM_C + 1];
        t[SP3D_CAM_WH] = t[SP3D_CAM_W0]; t[SP3D_CAM_WH + 1] = t[SP3D_CAM_H0];
        t[SP3D_CAM_FLIP2] = t[SP3D_CAM_FLIP];
        uint32_t m = 0;                     // the per-view test of the projection: every |A| <= 1e30f, as integers (NaN / inf are larger)
        for (int i = 0; i < 6; ++i) {
            uint32_t a;
            memcpy(&a, &t[SP3D_CAM_A + i], 4);
            a &= 0x7fffffffu;
            m = a > m ? a : m;
        }
        t[SP3D_CAM_TAME] = m <= 0x7149f2cau ? 1.0f : 0.0f;
        t[30] = t[31] = t[63] = 0.0f;
    }
    return SP3D_OK;
}

extern "C" const char *sp3d_error_string(int code)
{
    switch (code) {
    case SP3D_OK: return "ok";
    case SP3D_EINVAL: return "invalid argument (dimension <= 0, too many views, unknown layout)";
    case SP3D_ENULL: return "required pointer is NULL";
    case SP3D_ERANGE: return "size overflows 32-bit kernel indexing";
    case SP3D_EUNSUPPORTED: return "unsupported combination";
    case SP3D_EFFT: return "hipFFT plan creation or execution failed";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown sp3d error";
    }
}

// The forward entries (include/sp3d.h): each is run_entry with its own SP3D_PLAN_* value; every rule is decode_fwd's.
extern "C" int sp3d_unproject_fwd_indexed(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                          const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                          float *cubes, float *grids, int P, int V, int J, int h, int w, int X, int Y,
                                          int Z, const float *grid_size, int W_in, int H_in, void *stream)
{
    return run_entry(SP3D_PLAN_INDEXED, hm_layout, Jp, nullptr, 0, ZDSZ, Shape{P, V, J, h, w, X, Y, Z, grid_size, W_in, H_in}, true, hm_views,
                     cam, sample_of, centers, valid, cubes, grids, nullptr, stream);
}

extern "C" int sp3d_unproject_fwd_strided(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                          const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                          float *cubes, const int64_t *out_strides, int P, int V, int J, int h, int w,
                                          int X, int Y, int Z, const float *grid_size, int W_in, int H_in, void *stream)
{
    return run_entry(SP3D_PLAN_STRIDED, hm_layout, Jp, out_strides, 0, ZDSZ, Shape{P, V, J, h, w, X, Y, Z, grid_size, W_in, H_in},
                     out_strides != nullptr, hm_views, cam, sample_of, centers, valid, cubes, nullptr, nullptr, stream);
}

extern "C" int sp3d_unproject_fwd_zdft(const float *const *hm_views, int Jp, const float *cam, const float *centers,
                                       const uint8_t *valid, float *spec, int B, int V, int J, int h, int w, int X, int Y,
                                       int Z, const float *grid_size, int W_in, int H_in, int SZ, void *stream)
{
    return run_entry(SP3D_PLAN_ZDFT, 0, Jp, nullptr, 0, SZ, Shape{B, V, J, h, w, X, Y, Z, grid_size, W_in, H_in}, true, hm_views, cam, nullptr,
                     centers, valid, spec, nullptr, nullptr, stream);
}

extern "C" int sp3d_unproject_fwd(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                  const float *centers, const uint8_t *valid, float *cubes, float *grids, int B,
                                  int V, int J, int h, int w, int X, int Y, int Z, const float *grid_size, int W_in,
                                  int H_in, void *stream)
{
    return sp3d_unproject_fwd_indexed(hm_views, hm_layout, Jp, cam, nullptr, centers, valid, cubes, grids, B, V, J, h,
                                      w, X, Y, Z, grid_size, W_in, H_in, stream);
}

// Not part of the drop-in ABI (declared in csrc/sp3d_tuning.h, which documents the word): same as sp3d_unproject_fwd for
// the NHWC layout, with an explicit kernel choice, for A/B measurements (tools/ab_variants.py).
extern "C" int sp3d_unproject_fwd_variant(const float *const *hm_views, int Jp, const float *cam, const float *centers,
                                          const uint8_t *valid, float *cubes, float *grids, int B, int V, int J,
                                          int h, int w, int X, int Y, int Z, const float *grid_size, int W_in,
                                          int H_in, int variant, void *stream)
{
    return run_entry(SP3D_PLAN_TUNING, 0, Jp, nullptr, variant, ZDSZ, Shape{B, V, J, h, w, X, Y, Z, grid_size, W_in, H_in}, true, hm_views, cam,
                     nullptr, centers, valid, cubes, grids, nullptr, stream);
}

// Measurement only (sp3d_tuning.h): the launches an entry's request resolves to, for a request given as shapes.  An entry without
// pointers: their facts are stated (all there, aligned, no grids), the launches are copied out instead of run.  No HIP call.
extern "C" int sp3d_unproject_fwd_plan(int entry, int hm_layout, int Jp, const int64_t *out_strides, int B, int V, int J, int h,
                                       int w, int X, int Y, int Z, int variant, char *names, int32_t *fields, int32_t *tuning,
                                       int32_t *records)
{
    if (!names || !fields || !tuning || !records) return SP3D_ENULL;
    if (entry < SP3D_PLAN_INDEXED || entry > SP3D_PLAN_ONE_TRAIN) return SP3D_EINVAL;
    const float grid_size[3] = {1.0f, 1.0f, 1.0f};
    FwdRequest rq;
    FwdTuning t;
    int rc = decode_fwd(rq, t, entry, hm_layout, Jp, out_strides, variant, CallFacts{true, true, false, 0, ZDSZ},
                        Shape{B, V, J, h, w, X, Y, Z, grid_size, 1, 1});
    if (rc) return rc;
    memcpy(tuning, &t, sizeof(t));
    Launch plan[SP3D_PLAN_RECORDS];
    rc = resolve_fwd(rq, t, plan, *records);
    if (rc) return rc;
    for (int i = 0; i < *records; ++i, names += SP3D_PLAN_NAME, fields += SP3D_PLAN_FIELDS) {
        const Launch &L = plan[i];
        const Geom &g = L.g;
        snprintf(names, SP3D_PLAN_NAME, "%s", L.name);
        const int32_t f[SP3D_PLAN_FIELDS] = {
            (int32_t)(L.grid * L.grid_y), (int32_t)L.block, (int32_t)L.lds, L.nscalars, (int32_t)L.scalar[0], (int32_t)L.scalar[1],
            (int32_t)L.scalar[2], (int32_t)L.scalar[3], g.J, g.xcd_chunk, g.xcd_order, g.xm_mode, g.xm_log2xps, g.xm_log2K, g.xm_rows,
            g.xm_tiles, (int32_t)g.xm_magic_tiles, g.bk_nxy, g.bk_nby, (int32_t)g.bk_magic_nxy, (int32_t)g.bk_magic_nby,
            g.blk_log2py, g.blk_w, g.blk_h, g.blk_nbx, g.blk_nzc, (int32_t)g.blk_magic_wh, (int32_t)g.blk_magic_h,
            (int32_t)L.view_off, (int32_t)L.out_off, L.grids ? 1 : 0};
        memcpy(fields, f, sizeof(f));
    }
    return SP3D_OK;
}

// forward with the gradient pass mask (uint16 per voxel, bit j = channel j passes gradient) for
// sp3d_unproject_bwd_packed.  NHWC input only (the pipelined kernels): fp32 pixels, or bf16 pixels with SP3D_HM_BF16_TRAIN.
extern "C" int sp3d_unproject_fwd_train(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                        const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                        float *cubes, float *grids, uint16_t *pass_mask, int P, int V, int J, int h,
                                        int w, int X, int Y, int Z, const float *grid_size, int W_in, int H_in,
                                        void *stream)
{
    return run_entry(SP3D_PLAN_TRAIN, hm_layout, Jp, nullptr, 0, ZDSZ, Shape{P, V, J, h, w, X, Y, Z, grid_size, W_in, H_in}, pass_mask != nullptr,
                     hm_views, cam, sample_of, centers, valid, cubes, grids, pass_mask, stream);
}

// One-channel training forward: sp3d_unproject_fwd_indexed with SP3D_HM_ONE_CHANNEL (implied) + the pass mask at J = 1, in
// the words of sp3d_unproject_fwd_train.  SP3D_HM_BF16_TRAIN reads 2-byte taps.
extern "C" int sp3d_unproject_one_fwd_train(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                            const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                            float *cubes, float *grids, uint16_t *pass_mask, int P, int V, int J, int h,
                                            int w, int X, int Y, int Z, const float *grid_size, int W_in, int H_in,
                                            void *stream)
{
    return run_entry(SP3D_PLAN_ONE_TRAIN, hm_layout, Jp, nullptr, 0, ZDSZ, Shape{P, V, J, h, w, X, Y, Z, grid_size, W_in, H_in}, pass_mask != nullptr,
                     hm_views, cam, sample_of, centers, valid, cubes, grids, pass_mask, stream);
}

// measurement only: one thread writes the chip-wide 100 MHz clock (s_memrealtime) to *slot.  Two of them around a kernel
// inside a captured HIP graph give the kernel's time in the replayed step (bench.py roofline.in_step_graph_stamps; PyTorch's
// ROCm build refuses timing events inside a capture).
namespace sp3d {
__global__ void stamp_kernel(unsigned long long *slot) { *slot = wall_clock64(); }
} // namespace sp3d
extern "C" int sp3d_debug_stamp(uint64_t *slot, void *stream)
{
    if (!slot) return SP3D_ENULL;
    hipLaunchKernelGGL(sp3d::stamp_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, reinterpret_cast<unsigned long long *>(slot));
    return launch_status();
}

// measurement only: which -DSP3D_ABLATE mask this library carries (tools/diag_ablate.py)
extern "C" int sp3d_debug_set_diag(int flags)
{
    (void)flags;
    return SP3D_ABLATE;      // the ablation mask this library was compiled with (0 = the shipped kernels)
}

// measurement only: set / clear the per-wave timeline buffer of the pipelined kernel
extern "C" int sp3d_debug_set_timeline(void *dev_buffer)
{
#ifdef SP3D_TIMELINE
    unsigned long long *p = (unsigned long long *)dev_buffer;
    const int rc = set_pipe_timeline(p);
    return rc ? rc : set_brick_timeline(p);
#else
    (void)dev_buffer;
    return SP3D_EUNSUPPORTED;       // the shipped library carries no stamps; tools/wave_timeline.py builds its own
#endif
}
