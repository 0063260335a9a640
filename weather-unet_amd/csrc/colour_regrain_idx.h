// Index arithmetic of the regraining kernels (colour_regrain.hip): the level-size rule, the tile / halo walk of the Jacobi solve and the
// clamped neighbour reads.  Plain C++ with no HIP in it: the kernels include it, and scratch/regrain_emu.cpp runs the same functions on the
// CPU under the sanitizers, checking every LDS and global index against its bound.
#pragma once

#if defined(__HIPCC__)
#define RG_HD __host__ __device__ inline
#else
#define RG_HD inline
#endif

constexpr int kRgMaxLevels = 6;                 // iteration counts of a call, finest level first
constexpr int kRgMaxN = 1 << 21;                // pixels of an image
constexpr int kRgThreads = 512;                 // threads of a solve workgroup
constexpr int kRgCells = 8;                     // cells of the region per thread: weights and constant terms stay in registers
static_assert(kRgCells <= 8, "one 4-bit neighbour mask per cell in 32 bits");
constexpr int kRgRegion = kRgThreads * kRgCells;   // cells of a region (tile + halo) in LDS, three channels of 8 bytes each: 96 KiB
constexpr int kRgSide = 64;                     // a tiled region is at most kRgSide x kRgSide
constexpr int kRgMaxT = 8;                      // iterations per tiled launch = the halo: the owned tile is (kRgSide - 2 T)^2

RG_HD int rg_half(int v) { return (v + 1) / 2; }

// levels of an h x w image: level l + 1 exists iff l + 1 < n_iters and both halved sides (rounded up) exceed min_side
RG_HD int rg_level_count(int h, int w, int n_iters, int min_side) {
    int l = 1;
    while (l < n_iters && rg_half(h) > min_side && rg_half(w) > min_side) {
        h = rg_half(h), w = rg_half(w);
        ++l;
    }
    return l;
}

RG_HD void rg_level_size(int H, int W, int level, int* h, int* w) {
    for (int l = 0; l < level; ++l) H = rg_half(H), W = rg_half(W);
    *h = H, *w = W;
}

// a level that fits one region runs all its iterations in one launch of one workgroup per image
RG_HD bool rg_whole(int h, int w) { return (long long)h * w <= kRgRegion; }

// iterations of the next launch when `left` remain
RG_HD int rg_launch_iters(int h, int w, int left) { return rg_whole(h, w) || left < kRgMaxT ? left : kRgMaxT; }

RG_HD int rg_tile_side(int T) { return kRgSide - 2 * T; }

RG_HD int rg_tiles(int h, int w, int T, int* tiles_x) {
    if (rg_whole(h, w)) {
        *tiles_x = 1;
        return 1;
    }
    const int S = rg_tile_side(T);
    *tiles_x = (w + S - 1) / S;
    return *tiles_x * ((h + S - 1) / S);
}

struct RgTile {
    int x0, y0, x1, y1;          // the region in LDS: the owned cells and a halo of T, clipped to the image
    int ox0, oy0, ox1, oy1;      // the cells this workgroup writes back
};

RG_HD RgTile rg_tile(int h, int w, int T, int tiles_x, int t) {
    RgTile r;
    if (rg_whole(h, w)) {
        r.x0 = r.ox0 = 0, r.y0 = r.oy0 = 0, r.x1 = r.ox1 = w, r.y1 = r.oy1 = h;
        return r;
    }
    const int S = rg_tile_side(T);
    r.ox0 = (t % tiles_x) * S, r.oy0 = (t / tiles_x) * S;
    r.ox1 = r.ox0 + S < w ? r.ox0 + S : w;
    r.oy1 = r.oy0 + S < h ? r.oy0 + S : h;
    r.x0 = r.ox0 - T > 0 ? r.ox0 - T : 0;
    r.y0 = r.oy0 - T > 0 ? r.oy0 - T : 0;
    r.x1 = r.ox1 + T < w ? r.ox1 + T : w;
    r.y1 = r.oy1 + T < h ? r.oy1 + T : h;
    return r;
}

// Cell e = ry rw + rx of an rw x rh region; neighbour j = 0 up, 1 down, 2 left, 3 right, clamped to the REGION.  Where the region's edge is
// the image's edge this is the rule's clamp; elsewhere the read is wrong, and what it spoils moves one cell inwards per iteration: after T
// iterations it has not reached the owned cells, T cells from every such edge.
RG_HD int rg_nbr(int e, int rw, int rh, int j) {
    const int ry = e / rw, rx = e % rw;
    if (j == 0) return ry > 0 ? e - rw : e;
    if (j == 1) return ry < rh - 1 ? e + rw : e;
    if (j == 2) return rx > 0 ? e - 1 : e;
    return rx < rw - 1 ? e + 1 : e;
}

// the same through a mask computed once per cell: bit j set where neighbour j lies inside the region
RG_HD int rg_nbr_mask(int e, int rw, int rh) {
    const int ry = e / rw, rx = e % rw;
    return (ry > 0 ? 1 : 0) | (ry < rh - 1 ? 2 : 0) | (rx > 0 ? 4 : 0) | (rx < rw - 1 ? 8 : 0);
}
RG_HD int rg_nbr_at(int e, int rw, unsigned mask, int j) {
    const int step = j == 0 ? -rw : (j == 1 ? rw : (j == 2 ? -1 : 1));
    return (mask >> j) & 1u ? e + step : e;
}

RG_HD int rg_clamp(int v, int last) { return v < 0 ? 0 : (v > last ? last : v); }

// down: fine indices of coarse index d; up: coarse indices (near, far) of fine index d over a coarse axis of `nc`
RG_HD int rg_down_second(int d, int fine) { return 2 * d + 1 < fine ? 2 * d + 1 : fine - 1; }
RG_HD int rg_up_far(int d, int nc) { return rg_clamp((d & 1) ? d / 2 + 1 : d / 2 - 1, nc - 1); }

// doubles of workspace per image: weights (5) and constant terms (3) of every level, the ping-pong copy of the finest level (3), and for
// every coarser level the original, the downsampled transfer (c0) and the running result (3 each)
RG_HD long long rg_workspace_doubles(int H, int W, int levels) {
    long long total = 3ll * H * W;
    for (int l = 0; l < levels; ++l) {
        int h, w;
        rg_level_size(H, W, l, &h, &w);
        total += (8ll + (l > 0 ? 9 : 0)) * h * w;
    }
    return total;
}
