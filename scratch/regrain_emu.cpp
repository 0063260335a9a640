// CPU walk of the regraining kernels' index arithmetic (weather-unet_amd/csrc/colour_regrain_idx.h, the header colour_regrain.hip
// includes): the level-size rule, the tile / halo walk of regrain_solve_kernel with its LDS and global indices, and the down / up reads.
// A stand-alone host program for the sanitizers; it never touches a GPU:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scratch/regrain_emu.cpp -o /tmp/regrain_emu && /tmp/regrain_emu
// Every buffer is allocated at exactly the size the kernel has, so an index off by one is an AddressSanitizer report as well as a failed
// check.  Besides the bounds it proves the halo argument per launch: a cell counts as correct after iteration t only if all four of its
// region-clamped reads hit the cell the RULE names (the image-clamped neighbour) and that cell was correct after t - 1; after T iterations
// every owned cell must be correct, and every pixel must be owned by exactly one workgroup.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../weather-unet_amd/csrc/colour_regrain_idx.h"

static long long g_checks = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        ++g_checks;                           \
        if (!(cond)) {                        \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");       \
            std::exit(1);                     \
        }                                     \
    } while (0)

static void solve_launch(int h, int w, int T) {
    int tiles_x = 0;
    const int tiles = rg_tiles(h, w, T, &tiles_x);
    const long long n = (long long)h * w;
    std::vector<int> owners(n, 0);
    std::vector<double> global(3 * n, 0.0);
    for (int t = 0; t < tiles; ++t) {
        const RgTile tl = rg_tile(h, w, T, tiles_x, t);
        const int rw = tl.x1 - tl.x0, rh = tl.y1 - tl.y0, cells = rw * rh;
        CHECK(rw >= 1 && rh >= 1 && cells <= kRgRegion, "%dx%d T %d tile %d: region %dx%d exceeds %d cells", h, w, T, t, rw, rh, kRgRegion);
        CHECK(tl.x0 >= 0 && tl.y0 >= 0 && tl.x1 <= w && tl.y1 <= h, "%dx%d T %d tile %d: region outside the image", h, w, T, t);
        CHECK(tl.ox0 >= tl.x0 && tl.oy0 >= tl.y0 && tl.ox1 <= tl.x1 && tl.oy1 <= tl.y1 && tl.ox0 < tl.ox1 && tl.oy0 < tl.oy1,
              "%dx%d T %d tile %d: owned cells outside the region", h, w, T, t);
        std::vector<double> lds(3 * (size_t)kRgRegion, 0.0);           // ir[3][kRgRegion]
        std::vector<char> ok(cells, 1), next(cells, 1);
        // the load: thread tid, cell k
        for (int tid = 0; tid < kRgThreads; ++tid)
            for (int k = 0; k < kRgCells; ++k) {
                const int e = tid + k * kRgThreads;
                if (e >= cells) continue;
                const long long g = (long long)(tl.y0 + e / rw) * w + tl.x0 + e % rw;
                CHECK(g >= 0 && g < n, "%dx%d T %d tile %d: global index %lld of cell %d", h, w, T, t, g, e);
                for (int c = 0; c < 3; ++c) lds.at((size_t)c * kRgRegion + e) = global.at(c * n + g);
            }
        for (int it = 0; it < T; ++it) {
            for (int e = 0; e < cells; ++e) {
                const int y = tl.y0 + e / rw, x = tl.x0 + e % rw;
                const int want_y[4] = {rg_clamp(y - 1, h - 1), rg_clamp(y + 1, h - 1), y, y};
                const int want_x[4] = {x, x, rg_clamp(x - 1, w - 1), rg_clamp(x + 1, w - 1)};
                const unsigned mask = (unsigned)rg_nbr_mask(e, rw, rh);
                bool good = ok[e];
                for (int j = 0; j < 4; ++j) {
                    const int q = rg_nbr(e, rw, rh, j);
                    CHECK(q == rg_nbr_at(e, rw, mask, j), "%dx%d tile %d cell %d: the masked neighbour %d differs", h, w, t, e, j);
                    CHECK(q >= 0 && q < cells, "%dx%d T %d tile %d cell %d: LDS index %d of neighbour %d", h, w, T, t, e, q, j);
                    for (int c = 0; c < 3; ++c) (void)lds.at((size_t)c * kRgRegion + q);
                    const bool same = tl.y0 + q / rw == want_y[j] && tl.x0 + q % rw == want_x[j];
                    good = good && same && ok[q];
                }
                next[e] = good;
            }
            ok.swap(next);
        }
        for (int e = 0; e < cells; ++e) {
            const int y = tl.y0 + e / rw, x = tl.x0 + e % rw;
            if (y >= tl.oy0 && y < tl.oy1 && x >= tl.ox0 && x < tl.ox1) {
                CHECK(ok[e], "%dx%d T %d tile %d: owned cell (%d, %d) is reached by a region-edge read", h, w, T, t, y, x);
                ++owners.at((long long)y * w + x);
            }
        }
    }
    for (long long p = 0; p < n; ++p) CHECK(owners[p] == 1, "%dx%d T %d: pixel %lld is written by %d workgroups", h, w, T, p, owners[p]);
}

static void level(int h, int w, int iters) {
    for (int left = iters; left > 0;) {
        const int T = rg_launch_iters(h, w, left);
        CHECK(T >= 1 && T <= left && (rg_whole(h, w) || T <= kRgMaxT), "%dx%d: %d iterations in a launch with %d left", h, w, T, left);
        CHECK(rg_whole(h, w) || rg_tile_side(T) >= 1, "%dx%d: no owned cells at T %d", h, w, T);
        solve_launch(h, w, T);
        left -= T;
    }
}

static void pyramid(int H, int W, const std::vector<int>& iters, int min_side) {
    const int levels = rg_level_count(H, W, (int)iters.size(), min_side);
    CHECK(levels >= 1 && levels <= (int)iters.size() && levels <= kRgMaxLevels, "%dx%d: %d levels", H, W, levels);
    long long doubles = 3ll * H * W;
    for (int l = 0; l < levels; ++l) {
        int h, w;
        rg_level_size(H, W, l, &h, &w);
        CHECK(h >= 1 && w >= 1, "%dx%d level %d: empty", H, W, l);
        doubles += (l > 0 ? 17ll : 8ll) * h * w;
        if (l + 1 < levels) {
            int hc, wc;
            rg_level_size(H, W, l + 1, &hc, &wc);
            CHECK(hc == (h + 1) / 2 && wc == (w + 1) / 2 && hc > min_side && wc > min_side, "%dx%d level %d: size %dx%d", H, W, l + 1, hc, wc);
            std::vector<double> fine((size_t)h * w, 0.0), coarse((size_t)hc * wc, 0.0);
            for (int dy = 0; dy < hc; ++dy)
                for (int dx = 0; dx < wc; ++dx) {
                    const int ys[2] = {2 * dy, rg_down_second(dy, h)}, xs[2] = {2 * dx, rg_down_second(dx, w)};
                    for (int a = 0; a < 2; ++a)
                        for (int b = 0; b < 2; ++b) {
                            CHECK(ys[a] >= 0 && ys[a] < h && xs[b] >= 0 && xs[b] < w, "down (%d, %d) of %dx%d reads (%d, %d)", dy, dx, h, w, ys[a], xs[b]);
                            (void)fine.at((size_t)ys[a] * w + xs[b]);
                        }
                }
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const int ys[2] = {y / 2, rg_up_far(y, hc)}, xs[2] = {x / 2, rg_up_far(x, wc)};
                    for (int a = 0; a < 2; ++a)
                        for (int b = 0; b < 2; ++b) {
                            CHECK(ys[a] >= 0 && ys[a] < hc && xs[b] >= 0 && xs[b] < wc, "up (%d, %d) to %dx%d reads (%d, %d)", y, x, h, w, ys[a], xs[b]);
                            (void)coarse.at((size_t)ys[a] * wc + xs[b]);
                        }
                }
        } else if ((int)iters.size() > levels) {
            CHECK((h + 1) / 2 <= min_side || (w + 1) / 2 <= min_side, "%dx%d: level %d should exist", H, W, levels);
        }
        level(h, w, iters[l]);
    }
    CHECK(doubles == rg_workspace_doubles(H, W, levels), "%dx%d: workspace %lld against %lld", H, W, doubles, rg_workspace_doubles(H, W, levels));
}

int main() {
    const std::vector<int> def = {4, 16, 32, 64, 64, 64};
    struct Case { int h, w; std::vector<int> iters; int min_side; };
    const std::vector<Case> cases = {
        {1, 1, {3}, 20}, {1, 7, {3}, 20}, {2, 3, {2}, 20}, {7, 1, {5}, 20}, {9, 7, {2, 3, 4}, 0}, {33, 18, {2, 3, 4}, 0}, {1, 1, {1, 2, 3}, 0},
        {150, 170, {9, 3}, 0}, {70, 150, {5, 3}, 0}, {42, 42, def, 20}, {40, 40, def, 20}, {48, 40, {4, 16}, 20}, {224, 224, def, 20},
        {256, 256, def, 20}, {512, 512, def, 20}, {64, 64, def, 20}, {64, 65, {8, 17}, 20}, {1, 4097, {9}, 20}, {4097, 1, {20}, 20},
        {3, 2000, {7, 1}, 0}, {96, 120, def, 20}, {16, 12, def, 20},
    };
    for (const Case& c : cases) pyramid(c.h, c.w, c.iters, c.min_side);
    // every halo depth on shapes around the tile sizes
    for (int T = 1; T <= kRgMaxT; ++T)
        for (int h : {65, 97, 130})
            for (int w : {64, 100, 193}) solve_launch(h, w, T);
    CHECK(rg_level_count(224, 224, 6, 20) == 4 && rg_level_count(42, 42, 6, 20) == 2 && rg_level_count(40, 40, 6, 20) == 1, "level counts");
    std::printf("regrain_emu: %lld checks passed\n", g_checks);
    return 0;
}
