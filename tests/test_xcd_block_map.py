"""The brick unprojection's workgroup -> (sample, brick stack) maps, emulated on the host: every (sample, tile) exactly once.

The brick kernels (selfpose3d_amd/csrc/sp3d_unproject_brick.hip; launched by resolve_group, sp3d_unproject.hip) decode blockIdx.x through xcd_map_fast() with
fields the host fills in set_xcd_fields(), set_block_fields() and set_brick_fields() (selfpose3d_amd/csrc/sp3d_device.h:396-504);
udiv_magic() is sp3d_device.h:80-86.  Since round 6 the default for B in {1, 2, 4} is the block map: octants of the (x, y)
plane of brick columns at B = 1 on a square grid with an even side >= 4 (xm_mode 4, with a float square root and two
correcting loops), 2 x 4 / 2 x 2 / 1 x 2 blocks otherwise (xm_mode 3).  Any other batch keeps the chunk maps (xm_mode 0, 1,
2), and tuning bit 22 restores them for B in {1, 2, 4} too.

This file replays that integer arithmetic bit for bit in numpy (float32 for the octant's square root, like
__builtin_sqrtf) over every grid of 1..40 x 1..40 brick columns and 1..3 z-chunks, and asserts that the launch's grid
covers each (sample, tile) exactly once and that every workgroup that returns early maps to a place outside the grid.  It is
a property test of the map's algebra; tests/test_gpu_unproject_block_map.py checks the kernels themselves against the
oracle over whole volumes at the shapes the map serves."""
import numpy as np
import pytest

U32 = np.uint64(0xFFFFFFFF)


def ilog2(v):                                   # sp3d_device.h:398, :429 (smallest l with 2^l >= v)
    l = 0
    while (1 << l) < v:
        l += 1
    return l


def magic(d):                                   # (uint32_t)(2^32 / d + 1)
    return ((1 << 32) // max(d, 1) + 1) & 0xFFFFFFFF


def udiv_magic(n, d, m):
    """sp3d_device.h:80-86 on int64 arrays: qq = d == 1 ? n : umulhi(n, magic); one fix-up step"""
    n = n.astype(np.uint64)
    if d == 1:
        qq = n.astype(np.int64)
    else:
        qq = ((n * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
    rr = n.astype(np.int64) - qq * d
    fix = rr < 0
    qq = np.where(fix, qq - 1, qq)
    rr = np.where(fix, rr + d, rr)
    return qq, rr


def xcd_slots_per_xcd(B, tiles, K):            # sp3d_device.h:356-365
    if B <= 8 and 8 % B == 0:
        xps = 8 // B
        chunks = (tiles + K - 1) // K
        return ((chunks + xps - 1) // xps) * K
    if B > 8 and B % 8 == 0:
        return (B // 8) * tiles
    return (B * tiles + 7) // 8


def launch_geom(B, nbx, nby, nzc, chunks=False):
    """the host side of the brick launch (sp3d_unproject.hip resolve_fwd / resolve_group): chunk size K, xcd_order bit 0
    (centre-out for B <= 2), set_xcd_fields, set_brick_fields, set_block_fields -> (fields, grid size);
    tests/test_fwd_launch_plan.py holds it against the library's own plan"""
    wgs = nbx * nby * nzc
    g = dict(B=B, xcd_order=1 if B <= 2 else 0)
    xps = 8 // B if (B <= 8 and 8 % B == 0) else 1
    k = 1
    while k * 2 * xps * 2 <= wgs:
        k *= 2
    g["xcd_chunk"] = k
    # set_xcd_fields (sp3d_device.h:396-412)
    g["xm_tiles"], g["xm_magic_tiles"] = wgs, magic(wgs)
    if B <= 8 and 8 % B == 0 and k > 0 and (k & (k - 1)) == 0:
        g.update(xm_mode=0, xm_log2xps=ilog2(xps), xm_log2K=ilog2(k), xm_rows=((wgs + k - 1) // k + xps - 1) // xps)
    else:
        g.update(xm_mode=1 if (B > 8 and B % 8 == 0) else 2, xm_log2xps=0, xm_log2K=0, xm_rows=0)
    # set_brick_fields (sp3d_device.h:441-447)
    g.update(bk_nxy=nbx * nby, bk_nby=nby, bk_magic_nxy=magic(nbx * nby), bk_magic_nby=magic(nby))
    # set_block_fields (sp3d_device.h:413-440), skipped under tuning bit 22
    block_grid = 0
    if not chunks and B in (1, 2, 4):
        if B == 1 and nbx == nby and nbx % 2 == 0 and nbx >= 4:
            h = nbx // 2
            per = h * (h - 1) // 2 + (h + 1) // 2
            g.update(xm_mode=4, blk_w=h, blk_h=per, blk_nbx=nbx, blk_nzc=nzc, blk_log2py=0, blk_magic_h=magic(per))
            block_grid = 8 * nzc * per
        else:
            xps = 8 // B
            px = 2 if xps in (8, 4) else 1
            py = xps // px
            bw, bh = (nbx + px - 1) // px, (nby + py - 1) // py
            g.update(xm_mode=3, xm_log2xps=ilog2(xps), blk_log2py=ilog2(py), blk_w=bw, blk_h=bh, blk_nbx=nbx, blk_nzc=nzc,
                     blk_magic_wh=magic(bw * bh), blk_magic_h=magic(bh))
            block_grid = 8 * nzc * bw * bh
    grid = block_grid if block_grid else 8 * xcd_slots_per_xcd(B, wgs, k)
    return g, grid


def xcd_map_fast(bid, g):
    """sp3d_device.h:450-502 over an array of block ids -> (ok, b, tile, inside) where `inside` says whether the decoded
    place lies in the grid (what a false return must not)"""
    x, slot = bid & 7, bid >> 3
    m = g["xm_mode"]
    if m == 0:
        b = x >> g["xm_log2xps"]
        sub = x & ((1 << g["xm_log2xps"]) - 1)
        row = slot >> g["xm_log2K"]
        if g["xcd_order"] & 1:
            mid = g["xm_rows"] // 2
            row = mid + np.where(row & 1, -((row + 1) >> 1), row >> 1)
        chunk = (row << g["xm_log2xps"]) + sub
        tile = (chunk << g["xm_log2K"]) + (slot & ((1 << g["xm_log2K"]) - 1))
        ok = tile < g["xm_tiles"]
        return ok, b, tile, (tile >= 0) & (tile < g["xm_tiles"]) & (b < g["B"])
    if m == 3:
        b = x >> g["xm_log2xps"]
        sub = x & ((1 << g["xm_log2xps"]) - 1)
        pxi, pyi = sub >> g["blk_log2py"], sub & ((1 << g["blk_log2py"]) - 1)
        zc, t = udiv_magic(slot, g["blk_w"] * g["blk_h"], g["blk_magic_wh"])
        lx, ly = udiv_magic(t, g["blk_h"], g["blk_magic_h"])
        bx, by = pxi * g["blk_w"] + lx, pyi * g["blk_h"] + ly
        tile = (zc * g["blk_nbx"] + bx) * g["bk_nby"] + by
        ok = (zc < g["blk_nzc"]) & (bx < g["blk_nbx"]) & (by < g["bk_nby"])
        return ok, b, tile, ok & (bx >= 0) & (by >= 0)
    if m == 4:
        b = np.zeros_like(x)
        quad, upper, h = x >> 1, x & 1, g["blk_w"]
        tri = (h * (h - 1)) >> 1
        zc, k = udiv_magic(slot, g["blk_h"], g["blk_magic_h"])
        kf = k.astype(np.float32)
        u = ((np.float32(1.0) + np.sqrt(np.float32(1.0) + np.float32(8.0) * kf)) * np.float32(0.5)).astype(np.int64)
        while True:                                         # while (u (u-1) / 2 > k) --u
            s = ((u * (u - 1)) >> 1) > k
            if not s.any():
                break
            u = np.where(s, u - 1, u)
        while True:                                         # while ((u+1) u / 2 <= k) ++u
            s = (((u + 1) * u) >> 1) <= k
            if not s.any():
                break
            u = np.where(s, u + 1, u)
        v = k - ((u * (u - 1)) >> 1)
        diag = 2 * (k - tri) + np.where(upper == 1, 0, 1)
        lo = k < tri
        u, v = np.where(lo, u, diag), np.where(lo, v, diag)
        u, v = np.where(upper == 1, u, v), np.where(upper == 1, v, u)
        cx = g["blk_nbx"] >> 1
        bx = np.where(quad & 2, cx + u, cx - 1 - u)
        by = np.where(quad & 1, cx + v, cx - 1 - v)
        tile = (zc * g["blk_nbx"] + bx) * g["bk_nby"] + by
        ok = (zc < g["blk_nzc"]) & (u < h) & (v < h)
        inside = (zc < g["blk_nzc"]) & (bx >= 0) & (bx < g["blk_nbx"]) & (by >= 0) & (by < g["bk_nby"])
        return ok, b, tile, inside
    if m == 1:
        q, r = udiv_magic(slot, g["xm_tiles"], g["xm_magic_tiles"])
        b = x + 8 * q
        ok = b < g["B"]
        return ok, b, r, ok
    q, r = udiv_magic(slot * 8 + x, g["xm_tiles"], g["xm_magic_tiles"])
    ok = q < g["B"]
    return ok, q, r, ok


def check_bijection(B, nbx, nby, nzc, chunks=False):
    g, grid = launch_geom(B, nbx, nby, nzc, chunks)
    wgs = nbx * nby * nzc
    bid = np.arange(grid, dtype=np.int64)
    ok, b, tile, inside = xcd_map_fast(bid, g)
    where = (B, nbx, nby, nzc, chunks, g["xm_mode"])
    assert not (~ok & inside).any(), ("a workgroup returns early on a tile of the grid", where)
    assert ((tile[ok] >= 0) & (tile[ok] < wgs) & (b[ok] >= 0) & (b[ok] < B)).all(), where
    key = b[ok] * wgs + tile[ok]
    hits = np.bincount(key, minlength=B * wgs)
    assert hits.size == B * wgs and (hits == 1).all(), (where, int((hits == 0).sum()), int((hits > 1).sum()))
    # the brick kernels' decode of the tile (sp3d_unproject_brick.hip: udiv_magic by bk_nxy, then by bk_nby) lands in the grid
    zc, t = udiv_magic(tile[ok], g["bk_nxy"], g["bk_magic_nxy"])
    bx, by = udiv_magic(t, g["bk_nby"], g["bk_magic_nby"])
    assert ((zc < nzc) & (bx < nbx) & (by < nby)).all(), where
    return g["xm_mode"]


@pytest.mark.parametrize("B", [1, 2, 4])
def test_block_map_covers_every_tile_once(B):
    modes = set()
    for nzc in (1, 2, 3):
        for nbx in range(1, 41):
            for nby in range(1, 41):
                modes.add(check_bijection(B, nbx, nby, nzc))
    # the sweep really reaches the octants (B = 1) and the rectangular blocks
    assert modes == ({3, 4} if B == 1 else {3}), modes


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8, 16])
def test_chunk_maps_cover_every_tile_once(B):
    """xm_mode 0 (B | 8, centre-out rows for B <= 2), 1 (B a multiple of 8 above 8), 2 (any other batch); B in {1, 2, 4}
    through tuning bit 22"""
    modes = set()
    for nzc in (1, 2, 3):
        for nbx in range(1, 41, 3 if B in (1, 2, 4) else 1):
            for nby in range(1, 41):
                modes.add(check_bijection(B, nbx, nby, nzc, chunks=True))
    assert modes == {{3: 2, 5: 2, 16: 1}.get(B, 0)}, modes


def test_production_grids_take_the_intended_map():
    """the grids the project runs: root grid 80 x 80 x 20 (20 x 20 columns, one z-chunk), 64^3 pose cubes (16 x 16, two),
    160 x 160 x 40 (40 x 40, two), and the odd shapes of tests/test_gpu_unproject_block_map.py"""
    def cols(X, Y, Z):
        nwz = (Z + 3) // 4
        return (X + 3) // 4, (Y + 3) // 4, (nwz + 7) // 8
    assert launch_geom(1, *cols(80, 80, 20))[0]["xm_mode"] == 4
    assert launch_geom(1, *cols(40, 40, 12))[0]["blk_w"] == 5                  # octants with odd h
    assert launch_geom(1, *cols(88, 88, 8))[0]["blk_w"] == 11
    assert launch_geom(2, *cols(76, 60, 20))[0]["xm_mode"] == 3                 # odd nbx = 19, nby = 15
    assert launch_geom(4, *cols(64, 64, 64))[0]["xm_mode"] == 3
    assert launch_geom(3, *cols(64, 64, 64))[0]["xm_mode"] == 2
    for B, shape in ((1, (80, 80, 20)), (2, (80, 80, 20)), (4, (80, 80, 20)), (1, (64, 64, 64)), (2, (64, 64, 64)),
                     (4, (64, 64, 64)), (3, (64, 64, 64)), (8, (64, 64, 64)), (2, (160, 160, 40)), (2, (76, 60, 20)),
                     (4, (76, 60, 20)), (1, (40, 40, 12)), (1, (88, 88, 8))):
        check_bijection(B, *cols(*shape))
