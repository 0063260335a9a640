// Kernel Inception Distance: the unbiased polynomial-kernel MMD^2 of S random subsets of two feature banks, two launches in all.
//   * kid_gram_kernel    one 64 x 64 tile of a subset's xx / yy / xy kernel matrix per workgroup: rows gathered through the index array,
//                        <x_i, y_j> on the fp64 matrix cores (gram_f64.h: the tile, its LDS staging and its fragment maps), and the
//                        epilogue k = (gamma g + coef0)^degree summed to ONE double per tile -- the kernel matrix is never stored;
//   * kid_finish_kernel  one wave per subset: the tiles' partial sums per block in tile order, then mmd2.
// No atomics anywhere and every reduction in a fixed order: two runs give the same bits.
#include "gram_f64.h"

// the epilogue and mmd2 round every product and sum on its own, as the numpy restatement (tests/_kid_ref.py) does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

__host__ __device__ inline int kid_tiles_side(int m) { return (m + kGramTile - 1) / kGramTile; }
__host__ __device__ inline long long kid_tiles_tri(int T) { return (long long)T * (T + 1) / 2; }
__host__ __device__ inline long long kid_tiles(int m) {
    const int T = kid_tiles_side(m);
    return 2 * kid_tiles_tri(T) + (long long)T * T;
}

// grid (tiles, S).  Tile order inside a subset: the upper-triangular tiles of xx row by row ((0,0), (0,1), .. (0,T-1), (1,1), ..), the same
// for yy, then the T x T tiles of xy row-major.  idx: (S, 2, m) positions into x (row 0) and y (row 1).
__global__ __launch_bounds__(256) void kid_gram_kernel(const float* __restrict__ x, int ldx, int n1, const float* __restrict__ y, int ldy, int n2,
                                                       const int* __restrict__ idx, int m, int D, int degree, double gamma, double coef0,
                                                       double* __restrict__ partial) {
    __shared__ double sP[kGramTile * kGramLd];    // tile rows   [row][k]
    __shared__ double sQ[kGramTile * kGramLd];    // tile columns [row][k]
    __shared__ double sRed[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y;
    const int T = kid_tiles_side(m);
    const int tri = (int)kid_tiles_tri(T);

    // which block (0 xx, 1 yy, 2 xy) and which tile of it: wave-uniform integer work
    int t = blockIdx.x, block, ti, tj;
    if (t < 2 * tri) {
        block = t >= tri ? 1 : 0;
        t -= block * tri;
        ti = 0;
        while (t >= T - ti) {
            t -= T - ti;
            ++ti;
        }
        tj = ti + t;
    } else {
        block = 2;
        t -= 2 * tri;
        ti = t / T;
        tj = t - ti * T;
    }
    const float* pbase = block == 1 ? y : x;
    const float* qbase = block == 0 ? x : y;
    const int pld = block == 1 ? ldy : ldx, qld = block == 0 ? ldx : ldy;
    const int pn = block == 1 ? n2 : n1, qn = block == 0 ? n1 : n2;
    const int* pidx = idx + ((size_t)s * 2 + (block == 1 ? 1 : 0)) * m;
    const int* qidx = idx + ((size_t)s * 2 + (block == 0 ? 0 : 1)) * m;

    // the tile's inner products (gram_f64.h).  Positions past m read the subset's last row (their entries are zeroed below); indices are
    // clamped into the bank, so nothing reads out of bounds.
    f64x4_t acc[2][2];
    gram_tile_f64([&](int r) { return pbase + (size_t)min(max(pidx[min(ti * kGramTile + r, m - 1)], 0), pn - 1) * pld; },
                  [&](int r) { return qbase + (size_t)min(max(qidx[min(tj * kGramTile + r, m - 1)], 0), qn - 1) * qld; }, D, sP, sQ, acc);

    // epilogue, on gram_f64.h's C/D map
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const bool diag = block < 2 && ti == tj;
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = ti * kGramTile + wr + 16 * a + g + 4 * r;
                const int gj = tj * kGramTile + wc + 16 * b + l15;
                const double tt = acc[a][b][r] * gamma + coef0;
                double kv = tt;
                for (int p = 1; p < degree; ++p) kv *= tt;
                const bool keep = gi < m && gj < m && !(diag && gi == gj);
                sum += keep ? kv : 0.0;
            }
    if (block < 2 && ti < tj) sum *= 2.0;          // a strictly-upper tile stands for its mirror image too
    sum = wave_sum_f64(sum);
    if (lane == 0) sRed[wave] = sum;
    __syncthreads();
    if (tid == 0) partial[(size_t)s * gridDim.x + blockIdx.x] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// one wave per subset: lane l adds tiles l, l + 64, .. of a block in that order, the lanes are then summed in wave_sum_f64's order
__global__ __launch_bounds__(64) void kid_finish_kernel(const double* __restrict__ partial, int m, double* __restrict__ sums,
                                                        double* __restrict__ mmd2) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int T = kid_tiles_side(m);
    const int tri = (int)kid_tiles_tri(T);
    const int ntiles = 2 * tri + T * T;
    const double* p = partial + (size_t)s * ntiles;
    double v[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const int lo = b * tri, hi = b == 2 ? ntiles : lo + tri;
        double acc = 0.0;
        for (int t = lo + lane; t < hi; t += 64) acc += p[t];
        v[b] = wave_sum_f64(acc);
    }
    if (lane == 0) {
        const double sxx = v[0], syy = v[1], sxy = v[2];
        sums[3 * s + 0] = sxx;
        sums[3 * s + 1] = syy;
        sums[3 * s + 2] = sxy;
        const double mm1 = (double)((long long)m * (m - 1)), mm = (double)((long long)m * m);
        mmd2[s] = (sxx + syy) / mm1 - 2.0 * sxy / mm;
    }
}

constexpr int kKidMaxM = 1 << 20;     // 2 T^2 + T tiles stay far below 2^31

}  // namespace

extern "C" size_t wu_kid_workspace_bytes(int S, int m) {
    if (S <= 0 || S > 65535 || m < 2 || m > kKidMaxM) return 0;
    return (size_t)S * (size_t)kid_tiles(m) * sizeof(double);
}

extern "C" int wu_kid_mmd(const float* x, int ldx, int n1, const float* y, int ldy, int n2, const int* idx, int S, int m, int D, int degree,
                          double gamma, double coef0, void* workspace, double* sums, double* mmd2, void* stream) {
    WU_REQUIRE(m >= 2, "wu_kid_mmd: subset size m %d must be at least 2", m);
    WU_REQUIRE(n1 > 0 && n2 > 0 && m <= (n1 < n2 ? n1 : n2), "wu_kid_mmd: subset size m %d exceeds min(n1 %d, n2 %d)", m, n1, n2);
    WU_REQUIRE(m <= kKidMaxM, "wu_kid_mmd: subset size m %d over %d", m, kKidMaxM);
    WU_REQUIRE(degree >= 1, "wu_kid_mmd: degree %d must be at least 1", degree);
    WU_REQUIRE(S >= 1 && S <= 65535, "wu_kid_mmd: S %d outside 1..65535", S);
    WU_REQUIRE(D >= 1 && ldx >= D && ldy >= D, "wu_kid_mmd: D %d / ldx %d / ldy %d (ld >= D >= 1)", D, ldx, ldy);
    WU_REQUIRE(x && y && idx && workspace && sums && mmd2, "wu_kid_mmd: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kid_gram_kernel, dim3((unsigned)kid_tiles(m), (unsigned)S), dim3(256), 0, s, x, ldx, n1, y, ldy, n2, idx, m, D, degree,
                       gamma, coef0, (double*)workspace);
    WU_LAUNCH_CHECK("kid_gram_kernel");
    hipLaunchKernelGGL(kid_finish_kernel, dim3((unsigned)S), dim3(64), 0, s, (const double*)workspace, m, sums, mmd2);
    WU_LAUNCH_CHECK("kid_finish_kernel");
    return 0;
}
