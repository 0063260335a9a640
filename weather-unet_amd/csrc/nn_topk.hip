// Top-k nearest bank rows of every query row (wu/retrieval.py): the tile walk of prdc.hip's k-NN radii that also keeps WHICH column each of
// the smallest squared distances belongs to.  No distance matrix and no tile of one reaches global memory.
//   * nn_norms_kernel   |row|^2 in fp64, one wave per row, prdc_norms_kernel's order;
//   * nn_topk_kernel    grid (query row tiles, bank column splits): a workgroup walks the column tiles of its split, <q_i, b_j> on the fp64
//                       matrix cores (gram_f64.h: its LDS staging, fragment maps and barrier contract), d^2 = max((|q|^2 + |b|^2) - 2 g, 0)
//                       handed through LDS to one thread per query row, which keeps the row's k best (d^2, bank index) pairs in a sorted
//                       LDS list;
//   * nn_topk_finish    one thread per query row merges the splits' lists and writes dist2[nq][k] and index[nq][k].
// Pairs are ordered lexicographically: the smaller d^2 first, on equal d^2 the smaller bank index.  That is a total order on the columns of
// a row, so the k best are one fixed set in one fixed sequence whatever the number of splits, the order the tiles are walked in or the
// order workgroups finish in; nothing is summed across workgroups.  Norms, d^2 and tile are formed exactly as prdc.hip forms them: the
// k-th entry of a bank queried against itself is wu_knn_radii's radius bit for bit.
// Every index stored comes from a loop counter and every LDS / global position from tid, blockIdx and the checked arguments: non-finite
// features give meaningless neighbours, never an access outside a buffer.
#include <climits>
#include <cstdint>

#include "gram_f64.h"

// every product and sum of d^2 rounds on its own, as in prdc.hip and in the numpy restatement (tests/_nn_ref.py): no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kNnDistLd = kGramTile + 1;  // LDS row stride of a d^2 tile: 64 x 65 doubles fit in the two staging buffers (2 x 64 x 33)
constexpr int kNnMaxK = 16;               // largest k (prdc.hip's kMaxK)
constexpr int kNnListLd = kNnMaxK + 1;    // LDS stride of a row's list: odd, so the 64 owning threads sit in 64 different banks
constexpr int kNnMaxN = 1 << 21;          // rows per side: row tiles fit grid.x, a bank index fits an int
constexpr int kNnMaxSplits = 1024;        // forced column splits (grid.y)
constexpr int kNnTargetWorkgroups = 512;  // two per compute unit of a 256-CU part: what col_splits = 0 aims for

__host__ __device__ inline int nn_tiles(int n) { return (n + kGramTile - 1) / kGramTile; }

// col_splits = 0: as many splits as it takes to reach kNnTargetWorkgroups, at most one per column tile (prdc_splits' rule)
inline int nn_splits(int rows, int cols, int col_splits) {
    if (col_splits > 0) return col_splits;
    const int tr = nn_tiles(rows), tc = nn_tiles(cols);
    const int s = (kNnTargetWorkgroups + tr - 1) / tr;
    return s < 1 ? 1 : (s > tc ? tc : s);
}

// one wave per row: lane l adds the squares of features l, l + 64, .. in that order, then the lanes in wave_sum_f64's order
__global__ __launch_bounds__(256) void nn_norms_kernel(const float* __restrict__ x, int ldx, int n, int D, double* __restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                          // wave-uniform
    const float* p = x + (size_t)row * ldx;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)p[d];
        s += v * v;
    }
    s = wave_sum_f64(s);
    if (lane == 0) norms[row] = s;
}

__device__ __forceinline__ double nn_dist2(double na, double nb, double g) {
    const double d = (na + nb) - 2.0 * g;
    return d > 0.0 ? d : 0.0;
}

// (d, i) before (e, j) in the lexicographic order
__device__ __forceinline__ bool nn_before(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// grid (query row tiles, splits).  dlist / ilist: (nq, splits, k), ascending in the pair order, padded with (+inf, INT_MAX).  Three waves
// per SIMD, the d^2 tile living in the staging buffers between two tiles: the shape prdc_radii_kernel settled on.
__global__ __launch_bounds__(256, 3) void nn_topk_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ b, int ldb,
                                                         int nb, int D, int k, int self_offset, const double* __restrict__ qnorms,
                                                         const double* __restrict__ bnorms, double* __restrict__ dlist,
                                                         int* __restrict__ ilist) {
    __shared__ double sStage[2 * kGramTile * kGramLd];     // the staged chunks; between two tiles the d^2 tile [row][column], stride kNnDistLd
    __shared__ double sTopD[kGramTile * kNnListLd];        // per tile row the k best pairs so far: d^2 ..
    __shared__ int sTopI[kGramTile * kNnListLd];           // .. and bank index
    __shared__ double sNr[kGramTile];
    static_assert(kGramTile * kNnDistLd <= 2 * kGramTile * kGramLd, "the d^2 tile must fit in the staging buffers");
    double* sP = sStage;
    double* sQ = sStage + kGramTile * kGramLd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const int ti = blockIdx.x, split = blockIdx.y, S = gridDim.y;
    const int T = nn_tiles(nb);
    const int per = (T + S - 1) / S;
    const int t0 = split * per, t1 = min(T, t0 + per);
    const int gi = ti * kGramTile + tid;                   // the query row of threads 0..63
    const bool owner = tid < kGramTile && gi < nq;

    // threads 0..63 own one tile row's list each, from here to the end: no other thread touches sTopD / sTopI
    if (tid < kGramTile) {
        for (int j = 0; j < k; ++j) {
            sTopD[tid * kNnListLd + j] = __builtin_huge_val();
            sTopI[tid * kNnListLd + j] = INT_MAX;
        }
        sNr[tid] = qnorms[min(gi, nq - 1)];        // |q_i|^2 of the tile rows: read behind the first tile's barriers
    }

    for (int tj = t0; tj < t1; ++tj) {
        f64x4_t acc[2][2];
        // positions past nq / nb read the last row of their side; such rows write nothing and such columns are never scanned
        gram_tile_f64([&](int r) { return q + (size_t)min(ti * kGramTile + r, nq - 1) * ldq; },
                      [&](int r) { return b + (size_t)min(tj * kGramTile + r, nb - 1) * ldb; }, D, sP, sQ, acc);
        __syncthreads();                           // every wave is done with the staged chunks
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int cj = wc + 16 * bb + l15;
            const double nc = bnorms[min(tj * kGramTile + cj, nb - 1)];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ri = wr + 16 * a + g + 4 * r;        // rows by gram_f64.h's C/D map
                    sStage[ri * kNnDistLd + cj] = nn_dist2(sNr[ri], nc, acc[a][bb][r]);
                }
        }
        __syncthreads();
        if (owner) {
            double* L = sTopD + tid * kNnListLd;
            int* I = sTopI + tid * kNnListLd;
            const double* row = sStage + tid * kNnDistLd;
            const int c0 = tj * kGramTile;
            const int cn = min(kGramTile, nb - c0);            // columns past nb never enter
            // the bank column that is this query row itself, if it lies in this tile: never equal to a c >= 0 without a self_offset
            const int cself = self_offset >= 0 ? self_offset + gi - c0 : -1;
            double wd = L[k - 1];
            int wi = I[k - 1];
            for (int c = 0; c < cn; ++c) {
                const double v = row[c];
                const int gj = c0 + c;
                if (nn_before(v, gj, wd, wi) && c != cself) {
                    int j = k - 1;
                    while (j > 0 && nn_before(v, gj, L[j - 1], I[j - 1])) {
                        L[j] = L[j - 1];
                        I[j] = I[j - 1];
                        --j;
                    }
                    L[j] = v;
                    I[j] = gj;
                    wd = L[k - 1];
                    wi = I[k - 1];
                }
            }
        }
        // the next tile's first barrier (gram_tile_f64) keeps the staging stores behind this scan
    }
    if (owner) {
        const size_t o = ((size_t)gi * S + split) * (size_t)k;
        for (int j = 0; j < k; ++j) {
            dlist[o + j] = sTopD[tid * kNnListLd + j];
            ilist[o + j] = sTopI[tid * kNnListLd + j];
        }
    }
}

// one thread per query row: the splits' lists go through a sorted register list of 16 pairs (a compare-exchange chain with constant
// indices); the first k are the answer
__global__ __launch_bounds__(256) void nn_topk_finish(const double* __restrict__ dlist, const int* __restrict__ ilist, int nq, int k, int S,
                                                      double* __restrict__ dist2, int* __restrict__ index) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    double bd[kNnMaxK];
    int bi[kNnMaxK];
#pragma unroll
    for (int j = 0; j < kNnMaxK; ++j) {
        bd[j] = __builtin_huge_val();
        bi[j] = INT_MAX;
    }
    const size_t o = (size_t)i * S * (size_t)k;
    const int total = S * k;
    for (int t = 0; t < total; ++t) {
        double v = dlist[o + t];
        int c = ilist[o + t];
#pragma unroll
        for (int j = 0; j < kNnMaxK; ++j) {
            const bool first = nn_before(v, c, bd[j], bi[j]);
            const double lod = first ? v : bd[j], hid = first ? bd[j] : v;
            const int loi = first ? c : bi[j], hii = first ? bi[j] : c;
            bd[j] = lod;
            bi[j] = loi;
            v = hid;
            c = hii;
        }
    }
#pragma unroll
    for (int j = 0; j < kNnMaxK; ++j)
        if (j < k) {
            dist2[(size_t)i * k + j] = bd[j];
            index[(size_t)i * k + j] = bi[j];
        }
}

inline bool nn_args_ok(int nq, int nb, int k, int col_splits) {
    return k >= 1 && k <= kNnMaxK && nq >= 1 && nq <= kNnMaxN && nb >= k && nb <= kNnMaxN && col_splits >= 0 && col_splits <= kNnMaxSplits;
}

// the workspace: both sides' norms and the splits' d^2 lists (doubles), then the splits' index lists (ints)
inline size_t nn_list_entries(int nq, int nb, int k, int col_splits) {
    return (size_t)nq * (size_t)nn_splits(nq, nb, col_splits) * (size_t)k;
}

}  // namespace

extern "C" size_t wu_nn_workspace_bytes(int nq, int nb, int k, int col_splits) {
    if (!nn_args_ok(nq, nb, k, col_splits)) return 0;
    const size_t e = nn_list_entries(nq, nb, k, col_splits);
    return ((size_t)nq + (size_t)nb + e) * sizeof(double) + e * sizeof(int);
}

extern "C" int wu_nn_topk(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, int k, int self_offset, int col_splits,
                          void* ws, size_t ws_bytes, double* dist2, int* index, void* stream) {
    WU_REQUIRE(k >= 1 && k <= kNnMaxK, "wu_nn_topk: k %d outside 1..%d", k, kNnMaxK);
    WU_REQUIRE(nq >= 1 && nq <= kNnMaxN, "wu_nn_topk: nq %d outside 1..%d", nq, kNnMaxN);
    WU_REQUIRE(nb <= kNnMaxN, "wu_nn_topk: nb %d over %d", nb, kNnMaxN);
    WU_REQUIRE(self_offset >= -1, "wu_nn_topk: self_offset %d (-1: none)", self_offset);
    if (self_offset < 0) {
        WU_REQUIRE(nb >= k, "wu_nn_topk: nb %d bank rows, need at least k = %d", nb, k);
    } else {
        WU_REQUIRE(nb >= k + 1, "wu_nn_topk: nb %d bank rows, need at least k + 1 = %d with the row itself excluded", nb, k + 1);
        WU_REQUIRE(self_offset <= nb - nq, "wu_nn_topk: self_offset %d + nq %d over nb %d", self_offset, nq, nb);
    }
    WU_REQUIRE(D >= 1 && ldq >= D && ldb >= D, "wu_nn_topk: D %d / ldq %d / ldb %d (ld >= D >= 1)", D, ldq, ldb);
    WU_REQUIRE(col_splits >= 0 && col_splits <= kNnMaxSplits, "wu_nn_topk: col_splits %d outside 0..%d", col_splits, kNnMaxSplits);
    WU_REQUIRE(q && b && ws && dist2 && index, "wu_nn_topk: NULL pointer");
    WU_REQUIRE(((uintptr_t)ws & 7u) == 0, "wu_nn_topk: workspace not aligned to 8 bytes");
    const size_t need = wu_nn_workspace_bytes(nq, nb, k, col_splits);
    WU_REQUIRE(ws_bytes >= need, "wu_nn_topk: workspace of %zu bytes, need %zu", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int S = nn_splits(nq, nb, col_splits);
    const size_t e = nn_list_entries(nq, nb, k, col_splits);
    double* qnorms = (double*)ws;
    double* bnorms = qnorms + nq;
    double* dlist = bnorms + nb;
    int* ilist = (int*)(dlist + e);
    hipLaunchKernelGGL(nn_norms_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, q, ldq, nq, D, qnorms);
    WU_LAUNCH_CHECK("nn_norms_kernel");
    hipLaunchKernelGGL(nn_norms_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, b, ldb, nb, D, bnorms);
    WU_LAUNCH_CHECK("nn_norms_kernel");
    hipLaunchKernelGGL(nn_topk_kernel, dim3((unsigned)nn_tiles(nq), (unsigned)S), dim3(256), 0, s, q, ldq, nq, b, ldb, nb, D, k, self_offset,
                       (const double*)qnorms, (const double*)bnorms, dlist, ilist);
    WU_LAUNCH_CHECK("nn_topk_kernel");
    hipLaunchKernelGGL(nn_topk_finish, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const double*)dlist, (const int*)ilist, nq, k, S,
                       dist2, index);
    WU_LAUNCH_CHECK("nn_topk_finish");
    return 0;
}
