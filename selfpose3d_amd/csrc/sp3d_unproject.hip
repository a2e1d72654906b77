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
// Forward unprojection, host side: request (fwd_request) -> resolve_fwd() -> launch records -> launch_fwd().
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

// what a forward entry point asks for; `g` carries J, the image, the grid, the result strides and the pass mask
struct FwdRequest {
    int layout, Jp;      // SP3D_LAYOUT_* without the flag bits; channels (pixel stride) of a packed pixel
    int io;              // bit 0 = the heat-maps are bf16, bit 1 = the cubes are bf16
    bool one, out_cl, zd, out_aligned;   // one-channel read; channels-last result; z-spectrum result; result 16-byte aligned
    bool one_train;      // one-channel read that also writes the pass mask (sp3d_unproject_one_fwd_train)
    bool wide_mask;      // SP3D_HM_WIDE_MASK: the pass mask has two planes of P * N words, one per channel group of Jp = 32
    bool one_zd;         // SP3D_HM_ONE_ZSPECTRUM: the one-channel read with the z-spectrum result
    bool hm16;           // SP3D_HM_BF16_IN: bf16 maps into an fp32 result, next to exactly one of zd, one, one_zd
    bool hm16_train;     // SP3D_HM_BF16_TRAIN: bf16 maps into the fp32 results and the pass mask of the two training forwards
    Geom g;
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
// `t` is final here (resolve_fwd applied the downgrades).
static int resolve_group(const FwdRequest &rq, const FwdTuning &t, const Geom &g, int jp, int ps, Launch &L)
{
    const int wlds = jp * WOSTR > WREC ? jp * WOSTR : WREC;      // per-wave LDS floats of the pipe and brick kernels
    const int io = rq.io | ((rq.hm16 || rq.hm16_train) ? 1 : 0);  // bf16 taps: the storage flag, or either mixed flag (fp32 results)
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
        if (rq.zd && (rq.io || rq.out_cl || g.Z != ZDZ || nzc != 1 || zw != ZDZ / BR || (g.X % BR) || (g.Y % BR) || g.pass_mask))
            return SP3D_EUNSUPPORTED;
        set_launch(L, block_grid ? block_grid : xcd_grid_blocks(g.B, wgs, L.g.xcd_chunk), 64 * zw,
                   (size_t)zw * wlds * sizeof(float) + (size_t)t.ballast * 20480, 4, wgs, nby, nzc, zw);
        return find_brick_kernel(KernelKey{jp, ps, rq.zd, 0, rq.out_cl, io}, L.fn, L.name);
    }
    if (t.pipe) {    // 64 consecutive voxels per wave
        const int nw = t.one_wave ? 1 : 4;
        const int ptiles = (g.N + 64 * nw - 1) / (64 * nw), ptotal = ptiles * g.B;
        set_xcd_fields(L.g, ptiles);
        set_launch(L, t.no_xcd_map ? ptotal : xcd_grid_blocks(g.B, ptiles, g.xcd_chunk), 64 * nw, 0, 2, ptiles, ptotal);
        return find_pipe_kernel(KernelKey{jp, ps, !t.no_xcd_map, nw, rq.out_cl, io}, L.fn, L.name);
    }
    const int tiles = (g.N + TILE - 1) / TILE, total = tiles * g.B;
    set_launch(L, t.no_xcd_map ? total : xcd_grid_blocks(g.B, tiles, g.xcd_chunk), TILE,
               (size_t)(jp * OSTR + 2 * g.V * TILE + TILE) * sizeof(float), 2, tiles, total);
    return find_tile_kernel(KernelKey{jp, ps, !t.no_xcd_map, t.unroll, rq.out_cl, rq.io}, L.fn, L.name);
}

// SP3D_HM_ONE_CHANNEL (include/sp3d.h): g.J = channels written (1, or 4 = value + three zero channels), g.sB.. = planar
// result strides (dense or strided).  The pipe kernel's tile map: 64-voxel tiles dealt to a sample's XCDs in chunks.
static int resolve_one(const FwdRequest &rq, Launch &L)
{
    Geom &g = L.g;
    if ((rq.layout != SP3D_LAYOUT_PLANAR && rq.layout != SP3D_LAYOUT_NHWC) || rq.Jp < 1) return SP3D_EINVAL;
    if (rq.io || (g.pass_mask && !rq.one_train) || (rq.hm16 && rq.one_train)) return SP3D_EUNSUPPORTED;
    if (!(g.J == 4 || (g.J == 1 && !rq.out_cl))) return SP3D_EUNSUPPORTED;
    if (g.w < 2 || g.h < 2 || (int64_t)g.h * g.w > (1 << 24)) return SP3D_EUNSUPPORTED;
    if (rq.out_cl && !rq.out_aligned) return SP3D_EUNSUPPORTED;
    const int64_t px = rq.layout == SP3D_LAYOUT_NHWC ? rq.Jp : 1, row = (int64_t)g.w * px;
    // 24-bit multiplies form the tap offset, a 32-bit byte offset addresses it (bf16 maps: 2-byte elements)
    if (row >= (1 << 24) || (int64_t)g.h * row * ((rq.hm16 || rq.hm16_train) ? 2 : 4) > (int64_t)0x7fffffff) return SP3D_EUNSUPPORTED;
    const int ptiles = (g.N + 63) / 64;
    g.xcd_order = default_xcd_order(g);
    g.xcd_chunk = default_xcd_chunk(g, ptiles);
    set_xcd_fields(g, ptiles);
    const int64_t sample = rq.layout == SP3D_LAYOUT_NHWC ? (int64_t)g.h * row : (int64_t)rq.Jp * g.h * g.w;
    set_launch(L, xcd_grid_blocks(g.B, ptiles, g.xcd_chunk), 64, 0, 3, sample, (int)row, (int)px);
    const int vt = g.V <= 6 ? g.V : (g.V <= 8 ? 8 : (g.V <= 10 ? 10 : (g.V <= 12 ? 12 : 16)));
    return find_one_kernel(KernelKey{1, 1, vt, vt > 8 ? 8 : 4, rq.out_cl, g.pass_mask ? (rq.hm16_train ? 5 : 4) : (rq.hm16 ? 1 : 0)}, L.fn, L.name);
}

// SP3D_HM_ONE_ZSPECTRUM (include/sp3d.h): the one-channel read with the z-spectrum result of the brick ZD form at J = 1,
// unproject_one_zd_kernel.  One workgroup of ZDZ / BR waves per 4 x 4 tile of z columns, exactly P * tiles of them (the kernel
// deals them to the XCDs itself), a slab of 16 x ZDZ floats of LDS.  Nothing may stand next to the flag.
static int resolve_one_zd(const FwdRequest &rq, Launch &L)
{
    Geom &g = L.g;
    if ((rq.layout != SP3D_LAYOUT_PLANAR && rq.layout != SP3D_LAYOUT_NHWC) || rq.Jp < 1) return SP3D_EINVAL;
    if (rq.io || rq.one || rq.out_cl || rq.wide_mask || rq.zd || rq.one_train || g.pass_mask) return SP3D_EUNSUPPORTED;
    if (g.J != 1 || g.Z != ZDZ || (g.X % BR) || (g.Y % BR) || !g.dense) return SP3D_EUNSUPPORTED;
    if (g.w < 2 || g.h < 2 || (int64_t)g.h * g.w > (1 << 24)) return SP3D_EUNSUPPORTED;
    const int64_t px = rq.layout == SP3D_LAYOUT_NHWC ? rq.Jp : 1, row = (int64_t)g.w * px;
    // 24-bit multiplies form the tap offset, a 32-bit byte offset addresses it (bf16 maps: 2-byte elements)
    if (row >= (1 << 24) || (int64_t)g.h * row * (rq.hm16 ? 2 : 4) > (int64_t)0x7fffffff) return SP3D_EUNSUPPORTED;
    const int nby = g.Y / BR, tiles = (g.X / BR) * nby;
    set_xcd_fields(g, tiles);
    set_brick_fields(g, tiles, nby);
    const int64_t sample = rq.layout == SP3D_LAYOUT_NHWC ? (int64_t)g.h * row : (int64_t)rq.Jp * g.h * g.w;
    set_launch(L, (unsigned)(g.B * tiles), 64 * (ZDZ / BR), (size_t)16 * ZDZ * sizeof(float), 3, sample, (int)row, (int)px);
    L.grids = false;
    const int vt = g.V <= 6 ? g.V : (g.V <= 8 ? 8 : (g.V <= 10 ? 10 : (g.V <= 12 ? 12 : 16)));
    return find_one_zd_kernel(KernelKey{1, 1, vt, vt > 8 ? 8 : 4, false, rq.hm16 ? 9 : 8}, L.fn, L.name);
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
// with SP3D_HM_WIDE_MASK (sp3d_unproject_fwd_train): each group writes the 16-bit words of its own channels into its own
// plane of P * N words - group 1's mask pointer lies P * N words further, bit j of its words being channel 16 + j.
// SP3D_OUT_ZSPECTRUM (rq.zd): the same two groups through the ZD brick kernels.  The spectrum is (P, J, K, X/4, Y/4, 16)
// complex over ALL J channels, so the sample stride comes from here (Geom.sB, in complex elements - the ZD form reads no
// other result stride) and group 1 starts 16 channel planes = 16 * K * (X/4) * (Y/4) * 16 complex values further.

// The one place a forward request becomes launches: every downgrade and refusal, in this order.  Pure host arithmetic.
static int resolve_fwd(const FwdRequest &rq, FwdTuning t, Launch (&plan)[SP3D_PLAN_RECORDS], int &n)
{
    n = 1;
    Launch &L = plan[0];
    L = Launch{};
    L.g = rq.g; L.grid_y = 1; L.grids = !rq.zd;      // a z-spectrum launch writes no grids (its entries take none)
    // bf16 maps into a training forward (SP3D_HM_BF16_TRAIN): a form of the two entries that write a pass mask and of nothing
    // else - not of the bf16 storage pair, of the inference flag or of either spectrum; packed pixels of 16 elements, or of 32
    // with the two-plane mask, on the kernels that clamp a 2x2 block; the one-channel read has resolve_one's limits
    if (rq.hm16_train) {
        if (!rq.g.pass_mask || rq.io || rq.hm16 || rq.zd || rq.one_zd) return SP3D_EUNSUPPORTED;
        if (!rq.one && (rq.layout == SP3D_LAYOUT_PLANAR || (rq.layout == SP3D_LAYOUT_NHWC && rq.Jp != (rq.wide_mask ? WIDE_PS : 16)) ||
                        rq.g.w < 2 || rq.g.h < 2 || (int64_t)rq.g.h * rq.g.w > (1 << 24)))
            return SP3D_EUNSUPPORTED;
    }
    if (rq.one_zd) return resolve_one_zd(rq, L);
    // bf16 maps into an fp32 result (SP3D_HM_BF16_IN): a form of the z-spectrum result and of the one-channel read, of nothing
    // else - not of the bf16 storage pair, not of the two-plane mask, channels-last only from the one-channel kernel
    if (rq.hm16 && (!(rq.zd || rq.one) || rq.io || rq.wide_mask || (rq.out_cl && !rq.one))) return SP3D_EUNSUPPORTED;
    // the two-plane mask belongs to the Jp = 32 training forward with a planar fp32 result, and to nothing else
    if (rq.wide_mask && (rq.one || !rq.g.pass_mask || rq.layout != SP3D_LAYOUT_NHWC || rq.Jp != WIDE_PS || rq.out_cl || rq.io))
        return SP3D_EUNSUPPORTED;
    // the z-spectrum result: packed fp32 maps at Jp = 16 or 32, the one grid shape the z-DFT is built for, nothing else next to it
    if (rq.zd && (rq.one || rq.wide_mask || rq.layout != SP3D_LAYOUT_NHWC || rq.io || rq.out_cl || rq.g.pass_mask ||
                  (rq.Jp != 16 && rq.Jp != WIDE_PS) || rq.g.Z != ZDZ || (rq.g.X % BR) || (rq.g.Y % BR)))
        return SP3D_EUNSUPPORTED;
    if (rq.one) return resolve_one(rq, L);
    if (rq.layout == SP3D_LAYOUT_PLANAR) {
        if (rq.out_cl || rq.io) return SP3D_EUNSUPPORTED;
        set_launch(L, (rq.g.N + TILE - 1) / TILE, TILE, 0, 0, 0, 0);
        L.grid_y = rq.g.B;
        const int jc = rq.g.J == 1 ? 1 : (rq.g.J <= 4 ? 4 : 16);
        return find_planar_kernel(KernelKey{jc, jc, 0, 0, 0, 0}, L.fn, L.name);
    }
    if (rq.layout != SP3D_LAYOUT_NHWC) return SP3D_EINVAL;
    Geom g = rq.g;
    g.xcd_order = (t.plain_sweep ? 0 : default_xcd_order(g)) | (t.z_fastest ? 2 : 0);
    g.xcd_chunk = t.forced_chunk ? 1 << (t.forced_chunk - 1) : default_xcd_chunk(g, (g.N + 63) / 64);
    const FwdTuning asked = t, pipe = default_tuning(FWD_PIPE), stacks = default_tuning(FWD_BRICK_STACKS);
    // the pipelined kernels clamp a 2x2 block (needs a 2x2 image) and form pixel indices with 24-bit multiplies
    const bool tile_only = g.w < 2 || g.h < 2 || (int64_t)g.h * g.w > (1 << 24);
    if (rq.zd) {
        if (tile_only) return SP3D_EUNSUPPORTED;
        g.sB = (long long)g.J * (ZDSZ / 2 + 1) * (g.X / BR) * (g.Y / BR) * 16;
    }
    if (tile_only) t.pipe = t.brick = 0;
    if (t.brick) t.pipe = 1;
    if (rq.io || rq.hm16_train) t.one_wave = 1;    // bf16 taps: one wave per workgroup only
    if (rq.Jp == WIDE_PS) {
        if (g.J > WIDE_PS || rq.out_cl || (g.pass_mask && !rq.wide_mask) || tile_only) return SP3D_EUNSUPPORTED;
        if (memcmp(&asked, &pipe, sizeof(t)) && memcmp(&asked, &stacks, sizeof(t))) return SP3D_EUNSUPPORTED;
        Geom gg = g;
        gg.J = g.J < 16 ? g.J : 16;
        int rc = resolve_group(rq, t, gg, 16, WIDE_PS, L);
        if (rc || g.J <= 16) return rc;
        Launch &L1 = plan[n++];
        L1 = L;
        gg.J = g.J - 16;
        if (g.pass_mask) gg.pass_mask = g.pass_mask + (size_t)g.B * g.N;
        L1.view_off = 16 * (((rq.io & 1) || rq.hm16 || rq.hm16_train) ? 2 : 4);
        L1.out_off = rq.zd ? (size_t)16 * (ZDSZ / 2 + 1) * (g.X / BR) * (g.Y / BR) * 16 * 8
                           : (size_t)16 * g.sJ * ((rq.io & 2) ? 2 : 4);
        L1.grids = false;
        return resolve_group(rq, t, gg, (rq.io || rq.hm16 || rq.hm16_train) ? 16 : (gg.J + 3) / 4 * 4, WIDE_PS, L1);
    }
    if (rq.Jp < g.J || (rq.Jp & 3) || rq.Jp > 16) return SP3D_EUNSUPPORTED;
    if (rq.out_cl && (g.J & 3)) return SP3D_EUNSUPPORTED;        // channels-last rows must be 16-B multiples
    if (rq.io && !t.pipe) return SP3D_EUNSUPPORTED;
    return resolve_group(rq, t, g, rq.Jp, rq.Jp, L);
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

// The steps every forward entry point starts with: the Geom, the null check (`ptrs`: all its required pointers are there)
// and the flag bits of hm_layout.
static int fwd_request(FwdRequest &rq, int hm_layout, int Jp, bool ptrs, int B, int V, int J, int h, int w, int X,
                       int Y, int Z, const float *grid_size, int W_in, int H_in)
{
    const int rc = make_geom(rq.g, B, V, J, h, w, X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    if (!ptrs) return SP3D_ENULL;
    rq.layout = hm_layout & 0xff; rq.Jp = Jp;
    rq.io = ((hm_layout & SP3D_HM_BF16) ? 1 : 0) | ((hm_layout & SP3D_OUT_BF16) ? 2 : 0);
    rq.one = (hm_layout & SP3D_HM_ONE_CHANNEL) != 0;
    rq.out_cl = (hm_layout & SP3D_OUT_CHANNELS_LAST) != 0;
    rq.wide_mask = (hm_layout & SP3D_HM_WIDE_MASK) != 0;
    rq.zd = (hm_layout & SP3D_OUT_ZSPECTRUM) != 0;
    rq.one_zd = (hm_layout & SP3D_HM_ONE_ZSPECTRUM) != 0;
    rq.hm16 = (hm_layout & SP3D_HM_BF16_IN) != 0;
    rq.hm16_train = (hm_layout & SP3D_HM_BF16_TRAIN) != 0;
    rq.out_aligned = true; rq.one_train = false;
    return SP3D_OK;
}

// ... and end with: the views, the plan, its launches
static int run_fwd(const FwdRequest &rq, const FwdTuning &t, const float *const *hm_views, const float *cam, const float *centers,
                   const uint8_t *valid, float *cubes, float *grids, void *stream)
{
    Views v;
    int rc = load_views(v, hm_views, rq.g.V);
    if (rc) return rc;
    Launch plan[SP3D_PLAN_RECORDS];
    int n;
    rc = resolve_fwd(rq, t, plan, n);
    // SP3D_HM_WIDE_MASK at J <= 16: no second group, so nobody writes plane 1 - it is zeros
    if (!rc && rq.wide_mask && n == 1)
        rc = (int)hipMemsetAsync(rq.g.pass_mask + (size_t)rq.g.B * rq.g.N, 0, (size_t)rq.g.B * rq.g.N * sizeof(uint16_t), (hipStream_t)stream);
    for (int i = 0; !rc && i < n; ++i) rc = launch_fwd(plan[i], v, cam, centers, valid, cubes, grids, (hipStream_t)stream);
    return rc;
}

// result strides of sp3d_unproject_fwd_strided into the Geom; `cubes` decides whether 16-byte pieces are allowed
static int set_result_strides(Geom &g, const int64_t *out_strides, const void *cubes)
{
    const int64_t sB = out_strides[0], sJ = out_strides[1], sX = out_strides[2], sY = out_strides[3];
    // the planes must not overlap and must fit 32-bit in-plane offsets
    if (sY < g.Z || sX < (int64_t)g.Y * sY || sJ < (int64_t)g.X * sX || sB < (int64_t)g.J * sJ) return SP3D_EINVAL;
    if (sJ > 0x7fffffff) return SP3D_ERANGE;
    g.sB = sB; g.sJ = (int)sJ; g.sX = (int)sX; g.sY = (int)sY;
    g.dense = (sY == g.Z && sX == (int64_t)g.Y * g.Z && sJ == (int64_t)g.N && sB == (int64_t)g.J * g.N) ? 1 : 0;
    // 16-byte pieces need 4-element aligned rows (and a 16-byte aligned base pointer); otherwise the kernels take their
    // scalar store path, which is correct for any stride but slow
    g.vec4 = ((g.dense || ((sY | sX | sJ | sB) & 3) == 0) && ((uintptr_t)cubes & 15) == 0) ? 1 : 0;
    return SP3D_OK;
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

extern "C" int sp3d_unproject_fwd_indexed(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                          const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                          float *cubes, float *grids, int P, int V, int J, int h, int w, int X, int Y,
                                          int Z, const float *grid_size, int W_in, int H_in, void *stream)
{
    FwdRequest rq;
    const int rc = fwd_request(rq, hm_layout, Jp, cam && centers && valid && cubes, P, V, J, h, w, X, Y, Z,
                               grid_size, W_in, H_in);
    if (rc) return rc;
    rq.g.sample_of = sample_of;
    rq.out_aligned = ((uintptr_t)cubes & 15) == 0;
    if (rq.one_zd) {    // SP3D_HM_ONE_ZSPECTRUM: `cubes` is the spectrum of the one channel, whole 128-byte lines, no grids
        if (grids || ((uintptr_t)cubes & 127)) return SP3D_EUNSUPPORTED;
        return run_fwd(rq, default_tuning(FWD_PIPE), hm_views, cam, centers, valid, cubes, nullptr, stream);
    }
    if (rq.zd) {    // SP3D_OUT_ZSPECTRUM: `cubes` is the spectrum, whole 128-byte lines; the brick stacks as sp3d_unproject_fwd_zdft
        if (grids || ((uintptr_t)cubes & 127)) return SP3D_EUNSUPPORTED;
        return run_fwd(rq, default_tuning(FWD_BRICK_STACKS), hm_views, cam, centers, valid, cubes, nullptr, stream);
    }
    return run_fwd(rq, default_tuning(rq.g, rq.out_cl), hm_views, cam, centers, valid, cubes, grids, stream);
}

extern "C" int sp3d_unproject_fwd_strided(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                          const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                          float *cubes, const int64_t *out_strides, int P, int V, int J, int h, int w,
                                          int X, int Y, int Z, const float *grid_size, int W_in, int H_in, void *stream)
{
    FwdRequest rq;
    int rc = fwd_request(rq, hm_layout, Jp, cam && centers && valid && cubes && out_strides, P, V, J, h, w,
                         X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    // the one-channel read takes either layout
    if ((!rq.one && rq.layout != SP3D_LAYOUT_NHWC) || rq.out_cl || rq.zd || rq.one_zd || w < 2 || h < 2) return SP3D_EUNSUPPORTED;
    rc = set_result_strides(rq.g, out_strides, cubes);
    if (rc) return rc;
    rq.g.sample_of = sample_of;
    return run_fwd(rq, default_tuning(rq.g, false), hm_views, cam, centers, valid, cubes, nullptr, stream);
}

extern "C" int sp3d_unproject_fwd_zdft(const float *const *hm_views, int Jp, const float *cam, const float *centers,
                                       const uint8_t *valid, float *spec, int B, int V, int J, int h, int w, int X, int Y,
                                       int Z, const float *grid_size, int W_in, int H_in, int SZ, void *stream)
{
    FwdRequest rq;
    const int rc = fwd_request(rq, SP3D_LAYOUT_NHWC, Jp, cam && centers && valid && spec, B, V, J, h, w, X, Y, Z,
                               grid_size, W_in, H_in);
    if (rc) return rc;
    if (Jp != 16 || Z != ZDZ || SZ != ZDSZ || (X % BR) || (Y % BR) || w < 2 || h < 2 || (int64_t)h * w > (1 << 24) ||
        ((uintptr_t)spec & 127))
        return SP3D_EUNSUPPORTED;
    rq.zd = true;
    return run_fwd(rq, default_tuning(FWD_BRICK_STACKS), hm_views, cam, centers, valid, spec, nullptr, stream);
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
    FwdRequest rq;
    const int rc = fwd_request(rq, SP3D_LAYOUT_NHWC | ((variant & SP3D_TUNING_CHANNELS_LAST) ? SP3D_OUT_CHANNELS_LAST : 0),
                               Jp, cam && centers && valid && cubes, B, V, J, h, w, X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    return run_fwd(rq, decode_tuning(variant), hm_views, cam, centers, valid, cubes, grids, stream);
}

// Measurement only (sp3d_tuning.h): the launches resolve_fwd() decides on for a request given as shapes.  No HIP call.
extern "C" int sp3d_unproject_fwd_plan(int entry, int hm_layout, int Jp, const int64_t *out_strides, int B, int V, int J, int h,
                                       int w, int X, int Y, int Z, int variant, char *names, int32_t *fields, int32_t *tuning,
                                       int32_t *records)
{
    if (!names || !fields || !tuning || !records) return SP3D_ENULL;
    if (entry < SP3D_PLAN_INDEXED || entry > SP3D_PLAN_ONE_TRAIN) return SP3D_EINVAL;
    const float grid_size[3] = {1.0f, 1.0f, 1.0f};
    const bool hm16_train = (hm_layout & SP3D_HM_BF16_TRAIN) != 0;       // as asked: two entries below rewrite the word
    if (entry == SP3D_PLAN_ZDFT) hm_layout = SP3D_LAYOUT_NHWC | (hm_layout & (SP3D_HM_WIDE_MASK | SP3D_HM_ONE_ZSPECTRUM | SP3D_HM_BF16_IN));     // the entry has no layout word; the flags are kept to be refused
    if (entry == SP3D_PLAN_TUNING) hm_layout = SP3D_LAYOUT_NHWC | ((variant & SP3D_TUNING_CHANNELS_LAST) ? SP3D_OUT_CHANNELS_LAST : 0);
    if (entry == SP3D_PLAN_ONE_TRAIN) hm_layout |= SP3D_HM_ONE_CHANNEL;
    FwdRequest rq;
    int rc = fwd_request(rq, hm_layout, Jp, true, B, V, J, h, w, X, Y, Z, grid_size, 1, 1);
    if (!rc && entry == SP3D_PLAN_STRIDED && out_strides) rc = set_result_strides(rq.g, out_strides, nullptr);
    if (rc) return rc;
    // SP3D_OUT_ZSPECTRUM belongs to the indexed entry alone; sp3d_unproject_fwd_zdft keeps its own Jp == 16
    if ((rq.zd || rq.one_zd) && entry != SP3D_PLAN_INDEXED) return SP3D_EUNSUPPORTED;
    if (entry == SP3D_PLAN_ZDFT && (Jp != 16 || rq.hm16)) return SP3D_EUNSUPPORTED;
    if ((entry == SP3D_PLAN_TRAIN || entry == SP3D_PLAN_ONE_TRAIN) && rq.hm16) return SP3D_EUNSUPPORTED;     // as the two entries answer
    if (hm16_train && entry != SP3D_PLAN_TRAIN && entry != SP3D_PLAN_ONE_TRAIN) return SP3D_EUNSUPPORTED;   // no pass mask, no such form
    rq.one_train = entry == SP3D_PLAN_ONE_TRAIN;
    if (entry == SP3D_PLAN_TRAIN || rq.one_train) rq.g.pass_mask = reinterpret_cast<uint16_t *>(records);    // "there is one": never dereferenced
    rq.zd = rq.zd || entry == SP3D_PLAN_ZDFT;
    const FwdTuning t = entry == SP3D_PLAN_TUNING ? decode_tuning(variant)
                                                  : (rq.zd ? default_tuning(FWD_BRICK_STACKS) : default_tuning(rq.g, rq.out_cl));
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
// sp3d_unproject_bwd_packed.  NHWC input only (the pipelined kernels): fp32 pixels, or bf16 pixels with SP3D_HM_BF16_TRAIN
// (resolve_fwd holds that flag's refusals).
extern "C" int sp3d_unproject_fwd_train(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                        const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                        float *cubes, float *grids, uint16_t *pass_mask, int P, int V, int J, int h,
                                        int w, int X, int Y, int Z, const float *grid_size, int W_in, int H_in,
                                        void *stream)
{
    FwdRequest rq;
    const int rc = fwd_request(rq, hm_layout, Jp, cam && centers && valid && cubes && pass_mask, P, V, J, h, w,
                               X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    if (rq.layout != SP3D_LAYOUT_NHWC || rq.io || rq.one || rq.zd || rq.one_zd || rq.hm16 || w < 2 || h < 2) return SP3D_EUNSUPPORTED;
    rq.g.sample_of = sample_of;
    rq.g.pass_mask = pass_mask;
    return run_fwd(rq, default_tuning(rq.g, rq.out_cl), hm_views, cam, centers, valid, cubes, grids, stream);
}

// One-channel training forward: sp3d_unproject_fwd_indexed with SP3D_HM_ONE_CHANNEL (implied) + the pass mask at J = 1, in
// the words of sp3d_unproject_fwd_train.  The refusals are resolve_one's; SP3D_HM_BF16_TRAIN reads 2-byte taps.
extern "C" int sp3d_unproject_one_fwd_train(const float *const *hm_views, int hm_layout, int Jp, const float *cam,
                                            const int32_t *sample_of, const float *centers, const uint8_t *valid,
                                            float *cubes, float *grids, uint16_t *pass_mask, int P, int V, int J, int h,
                                            int w, int X, int Y, int Z, const float *grid_size, int W_in, int H_in,
                                            void *stream)
{
    FwdRequest rq;
    const int rc = fwd_request(rq, hm_layout | SP3D_HM_ONE_CHANNEL, Jp, cam && centers && valid && cubes && pass_mask, P, V,
                               J, h, w, X, Y, Z, grid_size, W_in, H_in);
    if (rc) return rc;
    if (rq.zd || rq.one_zd || rq.hm16) return SP3D_EUNSUPPORTED;
    rq.one_train = true;
    rq.g.sample_of = sample_of;
    rq.g.pass_mask = pass_mask;
    rq.out_aligned = ((uintptr_t)cubes & 15) == 0;
    return run_fwd(rq, default_tuning(rq.g, rq.out_cl), hm_views, cam, centers, valid, cubes, grids, stream);
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
