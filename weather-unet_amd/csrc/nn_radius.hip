// Every pair under a radius, and per-row realism / rarity scores, on feature rows (wu/retrieval.py): two more epilogues on the tile walk of
// nn_topk.hip and prdc.hip.  No distance matrix and no tile of one reaches global memory.
//   * nr_norms_kernel    |row|^2 in fp64, one wave per row, nn_norms_kernel's order;
//   * nr_count_kernel    grid (query row tiles, bank column splits): a workgroup walks the column tiles of its split, <q_i, b_j> on the fp64
//                        matrix cores (gram_f64.h: its LDS staging, fragment maps and barrier contract), d^2 = max((|q|^2 + |b|^2) - 2 g, 0)
//                        handed through LDS to one thread per query row, which counts the row's members in the split; one byte per tile
//                        says whether the tile holds a member at all;
//   * nr_scan_kernel     one workgroup: the (row, split) counts become exclusive int64 offsets in place, and row_ptr;
//   * nr_fill_kernel     the walk again over the tiles that hold a member; the owning thread writes the row's members, in column order,
//                        from its (row, split) offset.  A workgroup whose 64 rows have no member in its split returns before its first
//                        tile, and the walk ends with the tile that completes its rows;
//   * nr_ball_kernel     the walk with the bank's squared k-NN radii: per (row, split) the membership count, the smallest ball that holds
//                        the row and the maximiser of r2_j / d2_ij;
//   * nr_ball_finish     one thread per query row merges the splits.
// A (row, split) slot is written by one thread and columns ascend within it, so the CSR bytes and the scores are one fixed result whatever
// the number of splits or the order workgroups finish in.  Nothing crosses workgroups but plain stores read by a later launch: no atomics,
// no tickets, no workgroup waits on another.  Norms, d^2 and tile are formed exactly as nn_topk.hip and prdc.hip form them, so every d^2
// here is the same bits as wu_nn_topk's and wu_knn_radii's.
// Every index stored comes from a loop counter and every LDS / global position from tid, blockIdx and the checked arguments; an output
// position is also checked against the row's range and the capacity before the store: non-finite features or a row_ptr that does not
// belong to the workspace give a meaningless result, never an access outside a buffer.
#include <cmath>
#include <cstdint>

#include "gram_f64.h"

// every product and sum of d^2 rounds on its own, as in nn_topk.hip and in the numpy restatement (tests/_radius_ref.py): no fused
// multiply-add.  The quotient r2 / d2 is one IEEE division.
#pragma clang fp contract(off)

namespace {

constexpr int kNrDistLd = kGramTile + 1;  // LDS row stride of a d^2 tile: 64 x 65 doubles fit in the two staging buffers (2 x 64 x 33)
constexpr int kNrMaxN = 1 << 21;          // rows per side: row tiles fit grid.x, a bank index fits an int
constexpr int kNrMaxSplits = 1024;        // forced column splits (grid.y)
constexpr int kNrSlots = 768;             // resident workgroups of a 256-CU part at three 4-wave workgroups per CU: what col_splits = 0 fills
constexpr int kNrMaxAutoSplits = 8;       // splits col_splits = 0 may still choose once the row tiles alone exceed the slots
constexpr int kNrScanThreads = 1024;

__host__ __device__ inline int nr_tiles(int n) { return (n + kGramTile - 1) / kGramTile; }

// col_splits = 0: the workgroups run in rounds of kNrSlots, and a last round that is nearly empty costs a whole one (profiles/nn_bench.md:
// 782 workgroups on 768 slots).  Among 1 .. max(kNrSlots / row tiles, kNrMaxAutoSplits) splits, at most one per column tile, take the
// one whose rows x splits fill their rounds best, the fewer splits on a tie.  Integers only: the same choice on every host.
inline int nr_splits(int rows, int cols, int col_splits) {
    if (col_splits > 0) return col_splits;
    const long long tr = nr_tiles(rows), tc = nr_tiles(cols);
    long long cap = kNrSlots / tr > kNrMaxAutoSplits ? kNrSlots / tr : kNrMaxAutoSplits;
    cap = cap > tc ? tc : cap;
    long long best = 1, best_w = tr, best_r = (tr + kNrSlots - 1) / kNrSlots;      // filled share = w / (r kNrSlots)
    for (long long s = 2; s <= cap; ++s) {
        const long long w = tr * s, r = (w + kNrSlots - 1) / kNrSlots;
        if (w * best_r > best_w * r) {
            best = s;
            best_w = w;
            best_r = r;
        }
    }
    return (int)best;
}

// one wave per row: lane l adds the squares of features l, l + 64, .. in that order, then the lanes in wave_sum_f64's order
__global__ __launch_bounds__(256) void nr_norms_kernel(const float* __restrict__ x, int ldx, int n, int D, double* __restrict__ norms) {
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

__device__ __forceinline__ double nr_dist2(double na, double nb, double g) {
    const double d = (na + nb) - 2.0 * g;
    return d > 0.0 ? d : 0.0;
}

// the column tiles [t0, t1) of a workgroup's split; with upper_only the tiles that lie wholly at or below the first row's own column hold
// no member of any of its rows and are left out
__device__ __forceinline__ void nr_split_range(int nb, int ti, int self_offset, int upper_only, int& t0, int& t1) {
    const int split = blockIdx.y, S = gridDim.y;
    const int T = nr_tiles(nb);
    const int per = (T + S - 1) / S;
    t0 = split * per;
    t1 = min(T, t0 + per);
    if (upper_only) t0 = max(t0, (self_offset + ti * kGramTile + 1) / kGramTile);
}

// d^2 of tile (ti, tj) into sStage, [row][column] with stride kNrDistLd, seen by every thread on return.  sNr: |q_i|^2 of the tile rows.
// Positions past nq / nb read the last row of their side; such rows write nothing and such columns are never scanned.  All 256 threads
// make the call; the caller's next call (its first barrier) keeps the staging stores behind the caller's scan.
__device__ __forceinline__ void nr_dist_tile(const float* __restrict__ q, int ldq, int nq, int ti, const float* __restrict__ b, int ldb, int nb,
                                             int tj, int D, const double* __restrict__ bnorms, const double* sNr, double* sStage) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    f64x4_t acc[2][2];
    gram_tile_f64([&](int r) { return q + (size_t)min(ti * kGramTile + r, nq - 1) * ldq; },
                  [&](int r) { return b + (size_t)min(tj * kGramTile + r, nb - 1) * ldb; }, D, sStage, sStage + kGramTile * kGramLd, acc);
    __syncthreads();                               // every wave is done with the staged chunks
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        const int cj = wc + 16 * bb + l15;
        const double nc = bnorms[min(tj * kGramTile + cj, nb - 1)];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ri = wr + 16 * a + g + 4 * r;            // rows by gram_f64.h's C/D map
                sStage[ri * kNrDistLd + cj] = nr_dist2(sNr[ri], nc, acc[a][bb][r]);
            }
    }
    __syncthreads();
}

// the columns [lo, cn) of tile tj that query row gi may pair with, and the one among them it may not (cself, -1: none)
__device__ __forceinline__ void nr_columns(int nb, int tj, int gi, int self_offset, int upper_only, int& lo, int& cn, int& cself) {
    const int c0 = tj * kGramTile;
    cn = min(kGramTile, nb - c0);                  // columns past nb never enter
    cself = self_offset >= 0 ? self_offset + gi - c0 : -1;
    lo = upper_only ? max(0, cself + 1) : 0;
}

// grid (query row tiles, splits).  counts: (nq, splits) int64, every slot written (an empty split writes 0).  flags: (row tiles, column
// tiles) bytes, 1 where the tile holds a member; a workgroup writes the bytes of the tiles it walks and nr_fill_kernel, whose workgroup
// walks the same tiles, reads no others.
__global__ __launch_bounds__(256, 3) void nr_count_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ b, int ldb,
                                                          int nb, int D, double radius2, int self_offset, int upper_only,
                                                          const double* __restrict__ qnorms, const double* __restrict__ bnorms,
                                                          long long* __restrict__ counts, unsigned char* __restrict__ flags) {
    __shared__ double sStage[2 * kGramTile * kGramLd];     // the staged chunks; between two tiles the d^2 tile
    __shared__ double sNr[kGramTile];
    static_assert(kGramTile * kNrDistLd <= 2 * kGramTile * kGramLd, "the d^2 tile must fit in the staging buffers");
    const int tid = threadIdx.x, ti = blockIdx.x;
    const int gi = ti * kGramTile + tid;                   // the query row of threads 0..63
    const bool owner = tid < kGramTile && gi < nq;
    int t0, t1;
    nr_split_range(nb, ti, self_offset, upper_only, t0, t1);
    if (tid < kGramTile) sNr[tid] = qnorms[min(gi, nq - 1)];       // read behind the first tile's barriers
    int n = 0;
    for (int tj = t0; tj < t1; ++tj) {
        nr_dist_tile(q, ldq, nq, ti, b, ldb, nb, tj, D, bnorms, sNr, sStage);
        const int before = n;
        if (owner) {
            const double* row = sStage + tid * kNrDistLd;
            int lo, cn, cself;
            nr_columns(nb, tj, gi, self_offset, upper_only, lo, cn, cself);
            for (int c = lo; c < cn; ++c) n += (row[c] <= radius2 && c != cself) ? 1 : 0;
        }
        const int any = __syncthreads_or(n > before ? 1 : 0);      // the barrier also ends the scan
        if (tid == 0) flags[(size_t)ti * nr_tiles(nb) + tj] = any ? 1 : 0;
    }
    if (owner) counts[(size_t)gi * gridDim.y + blockIdx.y] = n;
}

// one workgroup: offs[0 .. n) hold counts and become their exclusive prefix sums, offs[n] the total; row_ptr[i] = offs[i * S].  Thread t
// takes the t-th run of ceil(n / 1024) slots; integers, so the order of the additions is free.
__global__ __launch_bounds__(kNrScanThreads) void nr_scan_kernel(long long* __restrict__ offs, long long n, int S, long long* __restrict__ row_ptr,
                                                                 int nq) {
    __shared__ long long sTot[kNrScanThreads];
    const int tid = threadIdx.x;
    const long long per = (n + kNrScanThreads - 1) / kNrScanThreads;
    const long long i0 = min(n, tid * per), i1 = min(n, i0 + per);
    long long s = 0;
    for (long long i = i0; i < i1; ++i) s += offs[i];
    sTot[tid] = s;
    __syncthreads();
    for (int off = 1; off < kNrScanThreads; off <<= 1) {
        const long long v = tid >= off ? sTot[tid - off] : 0;
        __syncthreads();
        sTot[tid] += v;
        __syncthreads();
    }
    long long run = sTot[tid] - s;                 // the slots before this thread's
    long long row = i0 / S, rem = i0 - row * S;    // slot i = row * S + rem
    for (long long i = i0; i < i1; ++i) {
        const long long c = offs[i];
        offs[i] = run;
        if (rem == 0) row_ptr[row] = run;
        run += c;
        if (++rem == S) {
            rem = 0;
            ++row;
        }
    }
    if (tid == kNrScanThreads - 1) {
        offs[n] = sTot[tid];
        row_ptr[nq] = sTot[tid];
    }
}

// grid (query row tiles, splits), nr_count_kernel's walk without the tiles whose flag is 0.  offs: nr_scan_kernel's.  A store goes to
// position p only if
// row_ptr[i] <= p < min(row_ptr[i + 1], capacity).
__global__ __launch_bounds__(256, 3) void nr_fill_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ b, int ldb,
                                                         int nb, int D, double radius2, int self_offset, int upper_only,
                                                         const double* __restrict__ qnorms, const double* __restrict__ bnorms,
                                                         const long long* __restrict__ offs, const unsigned char* __restrict__ flags,
                                                         const long long* __restrict__ row_ptr, long long capacity, int* __restrict__ col, double* __restrict__ dist2) {
    __shared__ double sStage[2 * kGramTile * kGramLd];
    __shared__ double sNr[kGramTile];
    const int tid = threadIdx.x, ti = blockIdx.x;
    const int gi = ti * kGramTile + tid;
    const bool owner = tid < kGramTile && gi < nq;
    long long pos = 0, end = 0, first = 0, last = 0;
    if (owner) {
        const size_t slot = (size_t)gi * gridDim.y + blockIdx.y;
        pos = offs[slot];
        end = offs[slot + 1];
        first = row_ptr[gi];
        last = min(row_ptr[gi + 1], capacity);
    }
    if (!__syncthreads_or(pos < end ? 1 : 0)) return;      // no row of this tile has a member in this split: uniform
    int t0, t1;
    nr_split_range(nb, ti, self_offset, upper_only, t0, t1);
    if (tid < kGramTile) sNr[tid] = qnorms[min(gi, nq - 1)];
    for (int tj = t0; tj < t1; ++tj) {
        if (!flags[(size_t)ti * nr_tiles(nb) + tj]) continue;      // no member in this tile: uniform
        nr_dist_tile(q, ldq, nq, ti, b, ldb, nb, tj, D, bnorms, sNr, sStage);
        if (pos < end) {                                   // owners only
            const double* row = sStage + tid * kNrDistLd;
            int lo, cn, cself;
            nr_columns(nb, tj, gi, self_offset, upper_only, lo, cn, cself);
            for (int c = lo; c < cn && pos < end; ++c) {
                const double v = row[c];
                if (v <= radius2 && c != cself) {
                    if (pos >= first && pos < last) {
                        col[pos] = tj * kGramTile + c;
                        dist2[pos] = v;
                    }
                    ++pos;
                }
            }
        }
        if (!__syncthreads_or(pos < end ? 1 : 0)) break;   // every row of the tile is complete; the barrier also ends the scan
    }
}

// grid (query row tiles, splits).  Per (row, split) slot: pd[3 slot ..] = rarity r2, realism r2, realism d2; pi[3 slot ..] = count, rarity
// column, realism column (-1: none in this split).  Columns ascend in a slot, so a strict comparison keeps the smaller column on a tie.
__global__ __launch_bounds__(256, 3) void nr_ball_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ b, int ldb,
                                                         int nb, int D, const double* __restrict__ r2, int self_offset,
                                                         const double* __restrict__ qnorms, const double* __restrict__ bnorms,
                                                         double* __restrict__ pd, int* __restrict__ pi) {
    __shared__ double sStage[2 * kGramTile * kGramLd];
    __shared__ double sNr[kGramTile];
    __shared__ double sRc[2][kGramTile];                   // r2 of the tile's columns, two tiles in flight: no barrier of its own
    const double inf = __builtin_huge_val();
    const int tid = threadIdx.x, ti = blockIdx.x;
    const int gi = ti * kGramTile + tid;
    const bool owner = tid < kGramTile && gi < nq;
    int t0, t1;
    nr_split_range(nb, ti, self_offset, 0, t0, t1);
    if (tid < kGramTile) sNr[tid] = qnorms[min(gi, nq - 1)];
    int cnt = 0, rar_i = -1, rl_i = -1;
    double rar_r2 = inf, rl_rho = -inf, rl_r2 = 0.0, rl_d2 = 0.0;
    for (int tj = t0; tj < t1; ++tj) {
        double* rc = sRc[tj & 1];
        // the scan of tile tj - 1 read the other half; the one of tile tj - 2 lies before the barriers of tile tj - 1
        if (tid < kGramTile) rc[tid] = r2[min(tj * kGramTile + tid, nb - 1)];
        nr_dist_tile(q, ldq, nq, ti, b, ldb, nb, tj, D, bnorms, sNr, sStage);
        if (owner) {
            const double* row = sStage + tid * kNrDistLd;
            int lo, cn, cself;
            nr_columns(nb, tj, gi, self_offset, 0, lo, cn, cself);
            for (int c = lo; c < cn; ++c) {
                if (c == cself) continue;
                const double v = row[c], r = rc[c];
                const int gj = tj * kGramTile + c;
                if (v <= r) {
                    ++cnt;
                    if (r < rar_r2) {
                        rar_r2 = r;
                        rar_i = gj;
                    }
                }
                const double rho = v == 0.0 ? inf : r / v;
                if (rho > rl_rho) {
                    rl_rho = rho;
                    rl_r2 = r;
                    rl_d2 = v;
                    rl_i = gj;
                }
            }
        }
    }
    if (owner) {
        const size_t o = 3 * ((size_t)gi * gridDim.y + blockIdx.y);
        pd[o] = rar_r2;
        pd[o + 1] = rl_r2;
        pd[o + 2] = rl_d2;
        pi[o] = cnt;
        pi[o + 1] = rar_i;
        pi[o + 2] = rl_i;
    }
}

// one thread per query row: counts add (integers); the rarity pair is the smallest (r2, column), the realism pair the largest quotient, on
// equal quotients the smaller column.  The quotient is formed again from the operands: the same division, the same bits.
__global__ __launch_bounds__(256) void nr_ball_finish(const double* __restrict__ pd, const int* __restrict__ pi, int nq, int S,
                                                      unsigned* __restrict__ count, double* __restrict__ rarity_r2, int* __restrict__ rarity_index,
                                                      double* __restrict__ realism_r2, double* __restrict__ realism_d2,
                                                      int* __restrict__ realism_index) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const double inf = __builtin_huge_val();
    unsigned cnt = 0u;
    int rar_i = -1, rl_i = -1;
    double rar_r2 = inf, rl_rho = -inf, rl_r2 = 0.0, rl_d2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const size_t o = 3 * ((size_t)i * S + s);
        cnt += (unsigned)pi[o];
        const int ai = pi[o + 1], li = pi[o + 2];
        if (ai >= 0) {
            const double r = pd[o];
            if (rar_i < 0 || r < rar_r2 || (r == rar_r2 && ai < rar_i)) {
                rar_r2 = r;
                rar_i = ai;
            }
        }
        if (li >= 0) {
            const double r = pd[o + 1], v = pd[o + 2];
            const double rho = v == 0.0 ? inf : r / v;
            if (rl_i < 0 || rho > rl_rho || (rho == rl_rho && li < rl_i)) {
                rl_rho = rho;
                rl_r2 = r;
                rl_d2 = v;
                rl_i = li;
            }
        }
    }
    count[i] = cnt;
    rarity_r2[i] = rar_r2;
    rarity_index[i] = rar_i;
    realism_r2[i] = rl_r2;
    realism_d2[i] = rl_d2;
    realism_index[i] = rl_i;
}

inline bool nr_sizes_ok(int nq, int nb, int col_splits) {
    return nq >= 1 && nq <= kNrMaxN && nb >= 1 && nb <= kNrMaxN && col_splits >= 0 && col_splits <= kNrMaxSplits;
}

inline size_t nr_slots(int nq, int nb, int col_splits) { return (size_t)nq * (size_t)nr_splits(nq, nb, col_splits); }

// bytes of the tile flags, rounded up to whole doubles
inline size_t nr_flag_bytes(int nq, int nb) { return ((size_t)nr_tiles(nq) * (size_t)nr_tiles(nb) + 7) / 8 * 8; }

// what the three entry points check alike; 0 when the arguments stand
int nr_check(const char* who, const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, int self_offset, int col_splits,
             const void* ws) {
    WU_REQUIRE(nq >= 1 && nq <= kNrMaxN, "%s: nq %d outside 1..%d", who, nq, kNrMaxN);
    WU_REQUIRE(nb >= 1 && nb <= kNrMaxN, "%s: nb %d outside 1..%d", who, nb, kNrMaxN);
    WU_REQUIRE(self_offset >= -1, "%s: self_offset %d (-1: none)", who, self_offset);
    if (self_offset >= 0) WU_REQUIRE(self_offset <= nb - nq, "%s: self_offset %d + nq %d over nb %d", who, self_offset, nq, nb);
    WU_REQUIRE(D >= 1 && ldq >= D && ldb >= D, "%s: D %d / ldq %d / ldb %d (ld >= D >= 1)", who, D, ldq, ldb);
    WU_REQUIRE(col_splits >= 0 && col_splits <= kNrMaxSplits, "%s: col_splits %d outside 0..%d", who, col_splits, kNrMaxSplits);
    WU_REQUIRE(q && b && ws, "%s: NULL pointer", who);
    WU_REQUIRE(((uintptr_t)ws & 7u) == 0, "%s: workspace not aligned to 8 bytes", who);
    return 0;
}

int nr_check_join(const char* who, double radius2, int self_offset, int upper_only) {
    WU_REQUIRE(std::isfinite(radius2) && radius2 >= 0.0, "%s: radius2 %g must be finite and >= 0", who, radius2);
    WU_REQUIRE(upper_only == 0 || self_offset >= 0, "%s: upper_only needs a self_offset >= 0", who);
    return 0;
}

void nr_launch_norms(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, double* qnorms, double* bnorms, hipStream_t s) {
    hipLaunchKernelGGL(nr_norms_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, q, ldq, nq, D, qnorms);
    hipLaunchKernelGGL(nr_norms_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, b, ldb, nb, D, bnorms);
}

}  // namespace

// the join's workspace: both sides' norms (doubles), then nq x splits + 1 int64 offsets, then one byte per 64 x 64 tile
extern "C" size_t wu_nn_radius_workspace_bytes(int nq, int nb, int col_splits) {
    if (!nr_sizes_ok(nq, nb, col_splits)) return 0;
    return ((size_t)nq + (size_t)nb) * sizeof(double) + (nr_slots(nq, nb, col_splits) + 1) * sizeof(long long) + nr_flag_bytes(nq, nb);
}

extern "C" int wu_nn_radius_count(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, double radius2, int self_offset,
                                  int upper_only, int col_splits, void* ws, size_t ws_bytes, long long* row_ptr, void* stream) {
    const char* who = "wu_nn_radius_count";
    if (int rc = nr_check(who, q, ldq, nq, b, ldb, nb, D, self_offset, col_splits, ws)) return rc;
    if (int rc = nr_check_join(who, radius2, self_offset, upper_only)) return rc;
    WU_REQUIRE(row_ptr, "%s: NULL pointer", who);
    const size_t need = wu_nn_radius_workspace_bytes(nq, nb, col_splits);
    WU_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int S = nr_splits(nq, nb, col_splits);
    double* qnorms = (double*)ws;
    double* bnorms = qnorms + nq;
    long long* offs = (long long*)(bnorms + nb);
    unsigned char* flags = (unsigned char*)(offs + nr_slots(nq, nb, col_splits) + 1);
    nr_launch_norms(q, ldq, nq, b, ldb, nb, D, qnorms, bnorms, s);
    WU_LAUNCH_CHECK("nr_norms_kernel");
    hipLaunchKernelGGL(nr_count_kernel, dim3((unsigned)nr_tiles(nq), (unsigned)S), dim3(256), 0, s, q, ldq, nq, b, ldb, nb, D, radius2,
                       self_offset, upper_only ? 1 : 0, (const double*)qnorms, (const double*)bnorms, offs, flags);
    WU_LAUNCH_CHECK("nr_count_kernel");
    hipLaunchKernelGGL(nr_scan_kernel, dim3(1), dim3(kNrScanThreads), 0, s, offs, (long long)nr_slots(nq, nb, col_splits), S, row_ptr, nq);
    WU_LAUNCH_CHECK("nr_scan_kernel");
    return 0;
}

extern "C" int wu_nn_radius_fill(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, double radius2, int self_offset,
                                 int upper_only, int col_splits, void* ws, size_t ws_bytes, const long long* row_ptr, long long capacity,
                                 int* col, double* dist2, void* stream) {
    const char* who = "wu_nn_radius_fill";
    if (int rc = nr_check(who, q, ldq, nq, b, ldb, nb, D, self_offset, col_splits, ws)) return rc;
    if (int rc = nr_check_join(who, radius2, self_offset, upper_only)) return rc;
    WU_REQUIRE(row_ptr, "%s: NULL pointer", who);
    WU_REQUIRE(capacity >= 0, "%s: capacity %lld is negative", who, capacity);
    const size_t need = wu_nn_radius_workspace_bytes(nq, nb, col_splits);
    WU_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, ws_bytes, need);
    if (capacity == 0) return 0;                   // an empty result: nothing to write, nothing launched
    WU_REQUIRE(col && dist2, "%s: NULL output with capacity %lld", who, capacity);
    hipStream_t s = (hipStream_t)stream;
    const int S = nr_splits(nq, nb, col_splits);
    const double* qnorms = (const double*)ws;
    const double* bnorms = qnorms + nq;
    const long long* offs = (const long long*)(bnorms + nb);
    const unsigned char* flags = (const unsigned char*)(offs + nr_slots(nq, nb, col_splits) + 1);
    hipLaunchKernelGGL(nr_fill_kernel, dim3((unsigned)nr_tiles(nq), (unsigned)S), dim3(256), 0, s, q, ldq, nq, b, ldb, nb, D, radius2,
                       self_offset, upper_only ? 1 : 0, qnorms, bnorms, offs, flags, row_ptr, capacity, col, dist2);
    WU_LAUNCH_CHECK("nr_fill_kernel");
    return 0;
}

// the scores' workspace: both sides' norms and three doubles per (row, split) slot, then three ints per slot
extern "C" size_t wu_nn_ball_workspace_bytes(int nq, int nb, int col_splits) {
    if (!nr_sizes_ok(nq, nb, col_splits)) return 0;
    const size_t e = 3 * nr_slots(nq, nb, col_splits);
    return ((size_t)nq + (size_t)nb + e) * sizeof(double) + e * sizeof(int);
}

extern "C" int wu_nn_ball_scores(const float* q, int ldq, int nq, const float* b, int ldb, int nb, int D, const double* r2, int self_offset,
                                 int col_splits, void* ws, size_t ws_bytes, unsigned* count, double* rarity_r2, int* rarity_index,
                                 double* realism_r2, double* realism_d2, int* realism_index, void* stream) {
    const char* who = "wu_nn_ball_scores";
    if (int rc = nr_check(who, q, ldq, nq, b, ldb, nb, D, self_offset, col_splits, ws)) return rc;
    WU_REQUIRE(self_offset < 0 || nb >= 2, "%s: nb %d bank rows, need at least 2 with the row itself excluded", who, nb);
    WU_REQUIRE(r2 && count && rarity_r2 && rarity_index && realism_r2 && realism_d2 && realism_index, "%s: NULL pointer", who);
    const size_t need = wu_nn_ball_workspace_bytes(nq, nb, col_splits);
    WU_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, need %zu", who, ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int S = nr_splits(nq, nb, col_splits);
    const size_t e = 3 * nr_slots(nq, nb, col_splits);
    double* qnorms = (double*)ws;
    double* bnorms = qnorms + nq;
    double* pd = bnorms + nb;
    int* pi = (int*)(pd + e);
    nr_launch_norms(q, ldq, nq, b, ldb, nb, D, qnorms, bnorms, s);
    WU_LAUNCH_CHECK("nr_norms_kernel");
    hipLaunchKernelGGL(nr_ball_kernel, dim3((unsigned)nr_tiles(nq), (unsigned)S), dim3(256), 0, s, q, ldq, nq, b, ldb, nb, D, r2, self_offset,
                       (const double*)qnorms, (const double*)bnorms, pd, pi);
    WU_LAUNCH_CHECK("nr_ball_kernel");
    hipLaunchKernelGGL(nr_ball_finish, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const double*)pd, (const int*)pi, nq, S, count,
                       rarity_r2, rarity_index, realism_r2, realism_d2, realism_index);
    WU_LAUNCH_CHECK("nr_ball_finish");
    return 0;
}
