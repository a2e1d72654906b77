/* sp3d_tuning.h - measurement-only entry points of libsp3d.so (NOT part of the drop-in ABI
 * in include/sp3d.h).  Used by tools/ab_variants.py for within-process A/B of kernel variants. */
#ifndef SP3D_TUNING_H
#define SP3D_TUNING_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The tuning word `variant` of sp3d_unproject_fwd_variant - this comment is the one place its layout is written down
 * (sp3d_unproject.hip, the host plan, decodes it once, into FwdTuning):
 *   bits 1:0    tile kernel (the first NHWC kernel): voxels in flight per lane - 0: 1, 2: 4, else 2
 *   bit 2       no XCD-aware tile map (tile and pipe kernels)
 *   bit 3       pipe: the per-wave software-pipelined kernel
 *   bit 4       one wave per workgroup (pipe kernel; bf16 storage implies it)
 *   bit 5       brick: 4x4x4 voxels per wave, a z-stack of bricks per workgroup (implies bit 3)
 *   bit 6       with bit 5, every brick its own workgroup
 *   bit 8       z-fastest chunk order; the bricks then keep the chunk map
 *   bit 10      with bit 5, a workgroup barrier per view (view-synchronous workgroups; round-5 measurement)
 *   bits 13:11  n: n * 20 KB of unused LDS per brick workgroup, which caps the workgroups resident on a CU (same)
 *   bits 20:17  log2(tiles per XCD chunk) + 1; 0: the default chunk size
 *   bit 21      chunks in plain sweep order instead of centre first
 *   bit 22      bricks: the round-5 chunk map instead of one block of brick columns (or octant) per XCD
 *   bit 24      channels-last result (not a tuning: it describes the result buffer)
 * Every other bit is ignored.  An image narrower or lower than 2 pixels, or of more than 2^24 pixels, takes the tile
 * kernel whatever the word says.  Library defaults: 120 (channels-last result), 56 (planar result, Z % 32 == 0), else 24. */
#define SP3D_TUNING_CHANNELS_LAST (1 << 24)
int sp3d_unproject_fwd_variant(const float *const *hm_views, int Jp, const float *cam, const float *centers,
                               const uint8_t *valid, float *cubes, float *grids, int B, int V, int J, int h, int w,
                               int X, int Y, int Z, const float *grid_size, int W_in, int H_in, int variant,
                               void *stream);
/* The launches a forward-unprojection request resolves to, for a request given as shapes: launches nothing, makes no HIP
 * call, runs without a GPU.  The plan answers what the entry answers: the entries and this function decode their arguments
 * with the same function (decode_fwd, sp3d_unproject.hip), which holds every refusal once; this function only has no
 * pointers - it states what an entry reads from them: all there, the result 128-byte aligned, no grids, SZ = 28 - and copies
 * the launches out instead of running them.
 *   entry        which entry point asks: _INDEXED (hm_layout with its flag bits as in include/sp3d.h), _STRIDED (the same,
 *                with out_strides, NULL = dense), _TRAIN (the same, with a pass mask), _ONE_TRAIN
 *                (sp3d_unproject_one_fwd_train: SP3D_HM_ONE_CHANNEL implied, with a pass mask), and the two entries that
 *                take no layout word: _ZDFT (sp3d_unproject_fwd_zdft) and _TUNING (sp3d_unproject_fwd_variant: NHWC fp32
 *                and the word `variant`, bit 24 included; `variant` is read for this entry only).  For these two the layout
 *                byte of hm_layout is not read and a word with flag bits is answered by one rule each (ENTRY_RULES,
 *                sp3d_unproject.hip): _ZDFT refuses SP3D_HM_WIDE_MASK, SP3D_HM_ONE_ZSPECTRUM, SP3D_HM_BF16_IN and
 *                SP3D_HM_BF16_TRAIN and ignores every other flag; _TUNING refuses SP3D_HM_BF16_TRAIN and ignores every other
 *                flag.  With hm_layout = 0 they answer exactly what their entries answer
 *   names        SP3D_PLAN_NAME bytes per launch: the kernel with its template arguments, as a kernel trace prints it
 *                without namespaces and parameter list
 *   fields       SP3D_PLAN_FIELDS int32 per launch: workgroups, workgroup size, dynamic LDS bytes, number of kernel
 *                arguments after Geom and the first four of them (low word of a 64-bit one), then of the launch's Geom J,
 *                xcd_chunk, xcd_order, xm_mode, xm_log2xps, xm_log2K, xm_rows, xm_tiles, xm_magic_tiles, bk_nxy, bk_nby,
 *                bk_magic_nxy, bk_magic_nby, blk_log2py, blk_w, blk_h, blk_nbx, blk_nzc, blk_magic_wh, blk_magic_h, then the
 *                byte offsets into views and result of a second channel group and whether the launch writes grids
 *   tuning       SP3D_PLAN_TUNING_FIELDS int32: the decoded tuning in the order of the list above (bits 1:0 as the count 1, 2, 4)
 *   records      number of launches (at most SP3D_PLAN_RECORDS)
 * Returns SP3D_OK or the refusal. */
enum { SP3D_PLAN_INDEXED, SP3D_PLAN_STRIDED, SP3D_PLAN_TRAIN, SP3D_PLAN_ZDFT, SP3D_PLAN_TUNING, SP3D_PLAN_ONE_TRAIN };
enum { SP3D_PLAN_RECORDS = 2, SP3D_PLAN_NAME = 96, SP3D_PLAN_FIELDS = 31, SP3D_PLAN_TUNING_FIELDS = 12 };
int sp3d_unproject_fwd_plan(int entry, int hm_layout, int Jp, const int64_t *out_strides, int B, int V, int J, int h, int w,
                            int X, int Y, int Z, int variant, char *names, int32_t *fields, int32_t *tuning, int32_t *records);
/* per-wave s_memtime timeline of the pipelined kernel (18 uint64 per wave: start, after P1(0), after each
 * view, ..., [17] = number of cameras seeing the lane-0 voxel); NULL switches it off (tools/wave_timeline.py) */
int sp3d_debug_set_timeline(void *dev_buffer);
/* one-thread kernel: *slot = the chip-wide 100 MHz clock.  Two around a kernel inside a captured graph time it in the step. */
int sp3d_debug_stamp(uint64_t *slot, void *stream);
#ifdef __cplusplus
}
#endif
#endif
