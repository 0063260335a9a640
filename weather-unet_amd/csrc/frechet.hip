// Rank-aware Frechet distance on two banks of float32 feature rows, without a covariance and without a matrix square root:
//     Tr sqrt(Sigma1 Sigma2) = || A B^T ||_* / sqrt((n1 - 1)(n2 - 1)),      A, B the centred rows,
// and A B^T is the double-centred cross-Gram matrix of the raw rows.  Its singular values come from a one-sided (Hestenes) Jacobi
// iteration: plane rotations of row pairs until every pair is orthogonal, then the row norms.
//   * fd_gram_kernel       one 64 x 64 tile of V[i][j] = <p_i, q_j> per workgroup on the fp64 matrix cores (gram_f64.h); the "vectors" p are
//                          the rows of the bank with fewer rows (ns <= nl), so V is ns x nl with row stride ld;
//   * fd_row_sums / fd_col_sums / fd_block_total / fd_centre_kernel
//                          V[i][j] = ((V[i][j] - r_i / nl) - c_j / ns) + t / (ns nl), in place;
//   * fd_mean / fd_dev2 / fd_block_total
//                          per bank mu and s = sum_i |x_i - mu|^2, two passes;
//   * fd_jacobi_kernel     one round-robin step: a workgroup per row pair, alpha = |p|^2, beta = |q|^2, gamma = <p, q>, and the rotation
//                          that makes them orthogonal unless they already are; one launch per step, every launch ends on its own;
//   * fd_sigma / fd_sigma_sum
//                          sigma_i = sqrt(|v_i|^2) and their sum in index order.
// Every floating-point reduction runs in one fixed order (block_sum_f64: a thread's elements t, t + 256, .. in order, wave_sum_f64, the four
// waves in wave order; the column sums and the means row by row), the only atomic is the integer rotation counter: the same inputs give the
// same bits.  tests/_frechet_ref.py restates every stage in numpy in the same order.
#include "gram_f64.h"

// every product and sum rounds on its own, as the numpy restatement does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kFdMaxVectors = 4096;   // ns: one workgroup per pair and step, ns - 1 launches per sweep
constexpr int kFdMaxRows = 1 << 21;   // rows per bank, and the length of a vector
constexpr int kFdRegLen = 2048;       // vectors up to this length stay in registers between the dot products and the update (8 per thread)
// A squared norm below DBL_MIN / eps has lost its relative precision to underflow: neither the threshold nor the rotation can be trusted,
// so the vector counts as zero and is stored as zero.  Without it a matrix with more vectors than length never settles: the surplus
// vectors shrink to about 1e-155 and then rotate among themselves on subnormal sums.
constexpr double kFdNorm2Floor = 0x1p-969;

__host__ __device__ inline int fd_tiles(int n) { return (n + kGramTile - 1) / kGramTile; }
inline int fd_ld(int nl) { return (nl + 7) & ~7; }
inline bool fd_counts_ok(int n1, int n2) { return n1 >= 2 && n2 >= 2 && n1 <= kFdMaxRows && n2 <= kFdMaxRows && (n1 < n2 ? n1 : n2) <= kFdMaxVectors; }

// The sum of one value per thread over the 256 threads of a workgroup, returned to every thread.  sRed: 4 doubles, free again after the call's
// first barrier; all 256 threads must make the call.
__device__ __forceinline__ double block_sum_f64(double v, double* sRed) {
    v = wave_sum_f64(v);
    __syncthreads();                               // an earlier call's readers are done with sRed
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// ---- stage 1: the cross-Gram matrix ----------------------------------------------------------------------------------------------------------
// grid (column tiles of nl, row tiles of ns).  Rows past the end read the bank's last row; their entries are not stored.
__global__ __launch_bounds__(256) void fd_gram_kernel(const float* __restrict__ p, int pld, int ns, const float* __restrict__ q, int qld, int nl,
                                                      int D, double* __restrict__ V, int ld) {
    __shared__ double sP[kGramTile * kGramLd];
    __shared__ double sQ[kGramTile * kGramLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = blockIdx.y, tj = blockIdx.x;
    f64x4_t acc[2][2];
    gram_tile_f64([&](int r) { return p + (size_t)min(ti * kGramTile + r, ns - 1) * pld; },
                  [&](int r) { return q + (size_t)min(tj * kGramTile + r, nl - 1) * qld; }, D, sP, sQ, acc);
    // gram_f64.h's C/D map
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = ti * kGramTile + wr + 16 * a + g + 4 * r;
                const int gj = tj * kGramTile + wc + 16 * b + l15;
                if (gi < ns && gj < nl) V[(size_t)gi * ld + gj] = acc[a][b][r];
            }
}

// ---- stage 2: double centring ----------------------------------------------------------------------------------------------------------------
// one workgroup per row
__global__ __launch_bounds__(256) void fd_row_sums_kernel(const double* __restrict__ V, int ld, int nl, double* __restrict__ r) {
    __shared__ double sRed[4];
    const double* v = V + (size_t)blockIdx.x * ld;
    double s = 0.0;
    for (int j = threadIdx.x; j < nl; j += 256) s += v[j];
    s = block_sum_f64(s, sRed);
    if (threadIdx.x == 0) r[blockIdx.x] = s;
}

// one thread per column: rows 0, 1, .. in order
__global__ __launch_bounds__(256) void fd_col_sums_kernel(const double* __restrict__ V, int ld, int ns, int nl, double* __restrict__ c) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nl) return;
    double s = 0.0;
    for (int i = 0; i < ns; ++i) s += V[(size_t)i * ld + j];
    c[j] = s;
}

// one workgroup: out[0] = the sum of a[0 .. n)
__global__ __launch_bounds__(256) void fd_block_total_kernel(const double* __restrict__ a, int n, double* __restrict__ out) {
    __shared__ double sRed[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += a[i];
    s = block_sum_f64(s, sRed);
    if (threadIdx.x == 0) out[0] = s;
}

// grid (column blocks, rows).  The four terms in this order, one rounding per operation.
__global__ __launch_bounds__(256) void fd_centre_kernel(double* __restrict__ V, int ld, int ns, int nl, const double* __restrict__ r,
                                                        const double* __restrict__ c, const double* __restrict__ t) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= nl) return;
    const double ri = r[i] / (double)nl;
    const double cj = c[j] / (double)ns;
    const double tt = t[0] / ((double)ns * (double)nl);
    double* v = V + (size_t)i * ld + j;
    *v = ((*v - ri) - cj) + tt;
}

// ---- stage 3: moments --------------------------------------------------------------------------------------------------------------------------
// grid ceil(D / 64): lane = column, wave w adds rows w, w + 4, .. in order; then the four waves in wave order, over n
__global__ __launch_bounds__(256) void fd_mean_kernel(const float* __restrict__ x, int ldx, int n, int D, double* __restrict__ mu) {
    __shared__ double sPart[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (d < D)
        for (int i = wave; i < n; i += 4) s += (double)x[(size_t)i * ldx + d];
    sPart[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && d < D) mu[d] = (((sPart[0][lane] + sPart[1][lane]) + sPart[2][lane]) + sPart[3][lane]) / (double)n;
}

// one workgroup per row: dev2[i] = sum_d (x_id - mu_d)^2
__global__ __launch_bounds__(256) void fd_dev2_kernel(const float* __restrict__ x, int ldx, int D, const double* __restrict__ mu,
                                                      double* __restrict__ dev2) {
    __shared__ double sRed[4];
    const float* p = x + (size_t)blockIdx.x * ldx;
    double s = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double v = (double)p[d] - mu[d];
        s += v * v;
    }
    s = block_sum_f64(s, sRed);
    if (threadIdx.x == 0) dev2[blockIdx.x] = s;
}

// ---- stage 4: one round-robin step of the one-sided Jacobi iteration ---------------------------------------------------------------------------
// grid ceil(ns / 2).  With N = 2 ceil(ns / 2) - 1, step s pairs (N, s) (workgroup 0) and ((s + k) mod N, (s - k + N) mod N) (workgroup k >= 1):
// over s = 0 .. N - 1 every unordered pair once, no index twice in a step.  p is the smaller index.  kRegs: nl <= kFdRegLen, the pair is
// read once; otherwise it is read again for the update.  Both forms add a thread's elements in the same order.
template <bool kRegs>
__global__ __launch_bounds__(256) void fd_jacobi_kernel(double* __restrict__ V, int ld, int ns, int nl, int step, double tol,
                                                        unsigned* __restrict__ rotations) {
    __shared__ double sRed[12];
    const int N = 2 * ((ns + 1) / 2) - 1;
    const int k = blockIdx.x;
    const int a = k == 0 ? N : (step + k) % N;
    const int b = k == 0 ? step : (step - k + N) % N;
    const int pi = min(a, b), qi = max(a, b);
    if (qi >= ns) return;                          // the phantom of an odd ns: uniform over the workgroup
    double* __restrict__ p = V + (size_t)pi * ld;
    double* __restrict__ q = V + (size_t)qi * ld;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    double pv[8], qv[8];
    double sa = 0.0, sb = 0.0, sg = 0.0;
    if (kRegs) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = tid + 256 * e;
            const bool ok = j < nl;
            pv[e] = ok ? p[j] : 0.0;               // a 0.0 past the end changes no partial sum
            qv[e] = ok ? q[j] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sa += pv[e] * pv[e];
            sb += qv[e] * qv[e];
            sg += pv[e] * qv[e];
        }
    } else {
        for (int j = tid; j < nl; j += 256) {
            const double x = p[j], y = q[j];
            sa += x * x;
            sb += y * y;
            sg += x * y;
        }
    }
    sa = wave_sum_f64(sa);
    sb = wave_sum_f64(sb);
    sg = wave_sum_f64(sg);
    if (lane == 0) {
        sRed[wave] = sa;
        sRed[4 + wave] = sb;
        sRed[8 + wave] = sg;
    }
    __syncthreads();
    const double alpha = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
    const double beta = ((sRed[4] + sRed[5]) + sRed[6]) + sRed[7];
    const double gamma = ((sRed[8] + sRed[9]) + sRed[10]) + sRed[11];

    // all of this is uniform over the workgroup: every thread holds the same three sums
    const bool dead_p = alpha < kFdNorm2Floor, dead_q = beta < kFdNorm2Floor;
    if (dead_p || dead_q) {
        if (dead_p && alpha != 0.0)
            for (int j = tid; j < nl; j += 256) p[j] = 0.0;
        if (dead_q && beta != 0.0)
            for (int j = tid; j < nl; j += 256) q[j] = 0.0;
        return;
    }
    if (fabs(gamma) <= (tol * sqrt(alpha)) * sqrt(beta)) return;       // LAPACK dgesvj's criterion: orthogonal already, nothing is written

    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));      // zeta = 0: t = 1
    const double c = 1.0 / sqrt(1.0 + t * t);
    const double s = c * t;
    if (kRegs) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = tid + 256 * e;
            if (j < nl) {
                p[j] = c * pv[e] - s * qv[e];
                q[j] = s * pv[e] + c * qv[e];
            }
        }
    } else {
        for (int j = tid; j < nl; j += 256) {
            const double x = p[j], y = q[j];
            p[j] = c * x - s * y;
            q[j] = s * x + c * y;
        }
    }
    if (tid == 0) atomicAdd(rotations, 1u);
}

// ---- stage 5: singular values ------------------------------------------------------------------------------------------------------------------
// one workgroup per vector
__global__ __launch_bounds__(256) void fd_sigma_kernel(const double* __restrict__ V, int ld, int nl, double* __restrict__ sigma) {
    __shared__ double sRed[4];
    const double* v = V + (size_t)blockIdx.x * ld;
    double s = 0.0;
    for (int j = threadIdx.x; j < nl; j += 256) {
        const double x = v[j];
        s += x * x;
    }
    s = block_sum_f64(s, sRed);
    if (threadIdx.x == 0) sigma[blockIdx.x] = sqrt(s);
}

// one workgroup: sigma_0 + sigma_1 + .. in index order
__global__ __launch_bounds__(256) void fd_sigma_sum_kernel(const double* __restrict__ sigma, int ns, double* __restrict__ total) {
    __shared__ double sSig[kFdMaxVectors];
    for (int i = threadIdx.x; i < ns; i += 256) sSig[i] = sigma[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < ns; ++i) s += sSig[i];
        total[0] = s;
    }
}

}  // namespace

extern "C" int wu_fd_ld(int n1, int n2) {
    if (!fd_counts_ok(n1, n2)) return 0;
    return fd_ld(n1 <= n2 ? n2 : n1);
}

// V (ns x ld), then the row sums (ns), the column sums (nl) and the total (1)
extern "C" size_t wu_fd_workspace_bytes(int n1, int n2, int D) {
    if (!fd_counts_ok(n1, n2) || D < 1) return 0;
    const size_t ns = (size_t)(n1 <= n2 ? n1 : n2), nl = (size_t)(n1 <= n2 ? n2 : n1);
    return (ns * (size_t)fd_ld((int)nl) + ns + nl + 1) * sizeof(double);
}

extern "C" int wu_fd_cross_gram(const float* x1, int ld1, int n1, const float* x2, int ld2, int n2, int D, void* workspace, void* stream) {
    WU_REQUIRE(n1 >= 2 && n2 >= 2 && n1 <= kFdMaxRows && n2 <= kFdMaxRows, "wu_fd_cross_gram: n1 %d / n2 %d outside 2..%d", n1, n2, kFdMaxRows);
    WU_REQUIRE((n1 < n2 ? n1 : n2) <= kFdMaxVectors, "wu_fd_cross_gram: min(n1 %d, n2 %d) over %d vectors", n1, n2, kFdMaxVectors);
    WU_REQUIRE(D >= 1 && ld1 >= D && ld2 >= D, "wu_fd_cross_gram: D %d / ld1 %d / ld2 %d (ld >= D >= 1)", D, ld1, ld2);
    WU_REQUIRE(x1 && x2 && workspace, "wu_fd_cross_gram: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const bool first = n1 <= n2;                   // a tie goes to set 1
    const float* p = first ? x1 : x2;
    const float* q = first ? x2 : x1;
    const int pld = first ? ld1 : ld2, qld = first ? ld2 : ld1;
    const int ns = first ? n1 : n2, nl = first ? n2 : n1;
    const int ld = fd_ld(nl);
    double* V = (double*)workspace;
    double* r = V + (size_t)ns * ld;
    double* c = r + ns;
    double* t = c + nl;
    hipLaunchKernelGGL(fd_gram_kernel, dim3((unsigned)fd_tiles(nl), (unsigned)fd_tiles(ns)), dim3(256), 0, s, p, pld, ns, q, qld, nl, D, V, ld);
    WU_LAUNCH_CHECK("fd_gram_kernel");
    hipLaunchKernelGGL(fd_row_sums_kernel, dim3((unsigned)ns), dim3(256), 0, s, (const double*)V, ld, nl, r);
    WU_LAUNCH_CHECK("fd_row_sums_kernel");
    hipLaunchKernelGGL(fd_col_sums_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, (const double*)V, ld, ns, nl, c);
    WU_LAUNCH_CHECK("fd_col_sums_kernel");
    hipLaunchKernelGGL(fd_block_total_kernel, dim3(1), dim3(256), 0, s, (const double*)r, ns, t);
    WU_LAUNCH_CHECK("fd_block_total_kernel");
    hipLaunchKernelGGL(fd_centre_kernel, dim3((unsigned)((nl + 255) / 256), (unsigned)ns), dim3(256), 0, s, V, ld, ns, nl, (const double*)r,
                       (const double*)c, (const double*)t);
    WU_LAUNCH_CHECK("fd_centre_kernel");
    return 0;
}

extern "C" int wu_fd_moments(const float* x, int ldx, int n, int D, double* mu, double* dev2, double* s, void* stream) {
    WU_REQUIRE(n >= 2 && n <= kFdMaxRows, "wu_fd_moments: n %d outside 2..%d", n, kFdMaxRows);
    WU_REQUIRE(D >= 1 && ldx >= D, "wu_fd_moments: D %d / ldx %d (ld >= D >= 1)", D, ldx);
    WU_REQUIRE(x && mu && dev2 && s, "wu_fd_moments: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fd_mean_kernel, dim3((unsigned)((D + 63) / 64)), dim3(256), 0, st, x, ldx, n, D, mu);
    WU_LAUNCH_CHECK("fd_mean_kernel");
    hipLaunchKernelGGL(fd_dev2_kernel, dim3((unsigned)n), dim3(256), 0, st, x, ldx, D, (const double*)mu, dev2);
    WU_LAUNCH_CHECK("fd_dev2_kernel");
    hipLaunchKernelGGL(fd_block_total_kernel, dim3(1), dim3(256), 0, st, (const double*)dev2, n, s);
    WU_LAUNCH_CHECK("fd_block_total_kernel");
    return 0;
}

extern "C" int wu_fd_jacobi_sweep(double* V, int ld, int ns, int nl, unsigned* rotations, void* stream) {
    WU_REQUIRE(ns >= 1 && ns <= kFdMaxVectors, "wu_fd_jacobi_sweep: ns %d vectors outside 1..%d", ns, kFdMaxVectors);
    WU_REQUIRE(nl >= 1 && nl <= kFdMaxRows && ld >= nl, "wu_fd_jacobi_sweep: nl %d / ld %d (1 <= nl <= %d, ld >= nl)", nl, ld, kFdMaxRows);
    WU_REQUIRE(V && rotations, "wu_fd_jacobi_sweep: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(rotations, 0, sizeof(unsigned), s);
    if (e != hipSuccess) WU_FAIL((int)e, "wu_fd_jacobi_sweep: hipMemsetAsync: %s", hipGetErrorString(e));
    const int half = (ns + 1) / 2, N = 2 * half - 1;
    const double tol = sqrt((double)nl) * 0x1p-53;
    for (int step = 0; step < N; ++step) {
        if (nl <= kFdRegLen)
            hipLaunchKernelGGL(fd_jacobi_kernel<true>, dim3((unsigned)half), dim3(256), 0, s, V, ld, ns, nl, step, tol, rotations);
        else
            hipLaunchKernelGGL(fd_jacobi_kernel<false>, dim3((unsigned)half), dim3(256), 0, s, V, ld, ns, nl, step, tol, rotations);
        WU_LAUNCH_CHECK("fd_jacobi_kernel");
    }
    return 0;
}

extern "C" int wu_fd_finish(const double* V, int ld, int ns, int nl, double* sigma, double* total, void* stream) {
    WU_REQUIRE(ns >= 1 && ns <= kFdMaxVectors, "wu_fd_finish: ns %d vectors outside 1..%d", ns, kFdMaxVectors);
    WU_REQUIRE(nl >= 1 && nl <= kFdMaxRows && ld >= nl, "wu_fd_finish: nl %d / ld %d (1 <= nl <= %d, ld >= nl)", nl, ld, kFdMaxRows);
    WU_REQUIRE(V && sigma && total, "wu_fd_finish: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fd_sigma_kernel, dim3((unsigned)ns), dim3(256), 0, s, V, ld, nl, sigma);
    WU_LAUNCH_CHECK("fd_sigma_kernel");
    hipLaunchKernelGGL(fd_sigma_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)sigma, ns, total);
    WU_LAUNCH_CHECK("fd_sigma_sum_kernel");
    return 0;
}
