// Colour baselines beyond the iterated transfer (wu/colour.py; tests/_regrain_ref.py states the arithmetic):
//
// REGRAINING (Pitie, Kokaram, Dahyot, CVIU 2007, section 5): the transferred colours IT are kept and the result is given the gradient
// field of the original I0, by a multigrid Jacobi solve.  State (nimg, 3, h w) fp64, as colour_ot.hip keeps it.
//   * regrain_down_kernel     one thread per coarse pixel of an image: the 2 x 2 mean (rows first, then columns) of the original and of
//                             the transfer, all three channels; the coarse transfer is written twice, as c0 and as the level's first iterate;
//   * regrain_weights_kernel  one thread per pixel of a level: dI from the clamped central differences of the original, psi, phi here and at
//                             the four neighbours, the four edge weights phi_j, den and the constant term b of the three channels -- once per
//                             level, so that an iteration is four products, one quotient and a blend per channel;
//   * regrain_solve_kernel    the hot path.  A workgroup of 512 threads holds a region (tile + halo, clipped to the image) of all three
//                             channels in LDS (96 KiB) and runs T Jacobi iterations on it; thread t owns cells t, t + 512, .. of the
//                             region, whose weights and constant terms stay in registers.  Region cells are numbered row-major with the
//                             region's own width as pitch, so the 32 lanes of a ds_read_b64 group read 256 contiguous bytes for the centre and
//                             for every neighbour: no bank conflicts at any width.  Neighbour reads clamp to the region: at an image edge
//                             that is the rule, elsewhere the error moves inwards one cell per iteration and stops short of the owned tile,
//                             T cells in.  Halo cells run the same operations as their owners, hence give the same bits: tiling cannot
//                             show.  A level of at most 4096 pixels (28 x 28, 56 x 56, 64 x 64) is one region and runs ALL its iterations
//                             in one launch; a larger one takes 8 per launch on 48 x 48 tiles (4 on 56 x 56 for the finest default level):
//                             5 solve launches for 224 x 224 with the default counts (1 + 2 + 1 + 1), against 116 at one per iteration;
//   * regrain_up_kernel       IR + up(c1 - c0): the coarse-grid correction, rows first, then columns.
//
// LINEAR MAPS (mean / sigma transfer, Reinhard et al. 2001; the Monge-Kantorovich map, Pitie & Kokaram 2007):
//   * colour_moments_*        mean and population covariance of point sets read through strides, in two passes, each a two-stage sum in an
//                             order fixed by n alone (include/wu_kernels.h);
//   * colour_linear_kernel    thread 0 of every workgroup forms the 3 x 3 map of its image from the two sets of moments (cyclic Jacobi, 8
//                             sweeps, no trigonometry) and the workgroup applies it to 4096 pixels.
// No atomics, no sum whose order depends on the grid: the same inputs give the same bits.
#include <math.h>

#include "colour_regrain_idx.h"
#include "wu_common.h"

// every product, sum and quotient is rounded on its own, as the numpy restatement does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kMomChunk = 4096;                // points of one partial sum: 16 per lane of a 256-thread workgroup
constexpr int kLinPer = 16;                    // pixels per thread of colour_linear_kernel

unsigned rg_grid(long long total) { return (unsigned)((total + 255) / 256); }

// ---------------------------------------------------------------------------------------------------------------------------------------
// regraining
// ---------------------------------------------------------------------------------------------------------------------------------------
struct RgDownArgs {
    const double* i0;            // (nimg, 3, h w): the original of the fine level
    const double* it;            // (nimg, 3, h w): the transfer of the fine level
    double* i0c;                 // (nimg, 3, hc wc)
    double* c0;
    double* irc;
    int h, w, hc, wc;
    long long total;             // nimg hc wc
};

__device__ __forceinline__ double rg_down_at(const double* a, int w, int y0, int y1, int x0, int x1) {
    const double r0 = (a[(long long)y0 * w + x0] + a[(long long)y1 * w + x0]) * 0.5;
    const double r1 = (a[(long long)y0 * w + x1] + a[(long long)y1 * w + x1]) * 0.5;
    return (r0 + r1) * 0.5;
}

__global__ __launch_bounds__(256) void regrain_down_kernel(const RgDownArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const int nc = a.hc * a.wc;
    const long long v = idx / nc;
    const int p = (int)(idx % nc);
    const int dy = p / a.wc, dx = p % a.wc;
    const int y0 = 2 * dy, y1 = rg_down_second(dy, a.h), x0 = 2 * dx, x1 = rg_down_second(dx, a.w);
    const long long n = (long long)a.h * a.w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long fine = (v * 3 + c) * n, coarse = (v * 3 + c) * nc + p;
        a.i0c[coarse] = rg_down_at(a.i0 + fine, a.w, y0, y1, x0, x1);
        const double t = rg_down_at(a.it + fine, a.w, y0, y1, x0, x1);
        a.c0[coarse] = t;
        a.irc[coarse] = t;
    }
}

struct RgWeightArgs {
    const double* i0;            // (nimg, 3, n)
    const double* it;            // (nimg, 3, n)
    double* wts;                 // (nimg, 5, n): phi_up, phi_down, phi_left, phi_right, den
    double* b;                   // (nimg, 3, n)
    int h, w;
    long long total;             // nimg n
    double num;                  // 30 * 2^-level
    double smooth;
};

// dI of pixel (y, x), both already inside the image: sqrt((q_0 + q_1) + q_2), q_c = gx gx + gy gy of the clamped central differences
__device__ __forceinline__ double rg_grad(const double* i0, int h, int w, int y, int x) {
    const int xl = rg_clamp(x - 1, w - 1), xr = rg_clamp(x + 1, w - 1), yu = rg_clamp(y - 1, h - 1), yd = rg_clamp(y + 1, h - 1);
    const long long n = (long long)h * w;
    double q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double* ch = i0 + c * n;
        const double gx = ch[(long long)y * w + xr] - ch[(long long)y * w + xl];
        const double gy = ch[(long long)yd * w + x] - ch[(long long)yu * w + x];
        q[c] = gx * gx + gy * gy;
    }
    return sqrt((q[0] + q[1]) + q[2]);
}

__device__ __forceinline__ double rg_phi(double dI, double num, double smooth) { return num / (1.0 + (10.0 * dI) / smooth); }

__global__ __launch_bounds__(256) void regrain_weights_kernel(const RgWeightArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const long long n = (long long)a.h * a.w;
    const long long v = idx / n;
    const int p = (int)(idx % n);
    const int y = p / a.w, x = p % a.w;
    const double* i0 = a.i0 + v * 3 * n;
    const double* it = a.it + v * 3 * n;
    const int ny[4] = {rg_clamp(y - 1, a.h - 1), rg_clamp(y + 1, a.h - 1), y, y};
    const int nx[4] = {x, x, rg_clamp(x - 1, a.w - 1), rg_clamp(x + 1, a.w - 1)};
    const double dI = rg_grad(i0, a.h, a.w, y, x);
    const double psi = fmin((256.0 * dI) / 5.0, 1.0);
    const double phi = rg_phi(dI, a.num, a.smooth);
    double pj[4];
    double den = psi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pj[j] = (rg_phi(rg_grad(i0, a.h, a.w, ny[j], nx[j]), a.num, a.smooth) + phi) * 0.5;
        den = den + pj[j];
        a.wts[(v * 5 + j) * n + p] = pj[j];
    }
    a.wts[(v * 5 + 4) * n + p] = den + 0x1p-52;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double* ch = i0 + c * n;
        const double s = ch[p];
        double b = psi * it[c * n + p];
#pragma unroll
        for (int j = 0; j < 4; ++j) b = b + pj[j] * (s - ch[(long long)ny[j] * a.w + nx[j]]);
        a.b[(v * 3 + c) * n + p] = b;
    }
}

struct RgSolveArgs {
    const double* src;           // (nimg, 3, n): the iterate before this launch
    double* dst;                 // the iterate after T iterations; src itself only where one workgroup holds the whole image
    const double* wts;           // (nimg, 5, n)
    const double* b;             // (nimg, 3, n)
    int h, w, T, tiles_x, tiles;
};

__global__ __launch_bounds__(kRgThreads) void regrain_solve_kernel(const RgSolveArgs a) {
    __shared__ double ir[3][kRgRegion];
    const int tid = threadIdx.x;
    const long long v = blockIdx.x / a.tiles;
    const RgTile tl = rg_tile(a.h, a.w, a.T, a.tiles_x, blockIdx.x % a.tiles);
    const int rw = tl.x1 - tl.x0, rh = tl.y1 - tl.y0, cells = rw * rh;      // cells <= kRgRegion: rg_tile
    const long long n = (long long)a.h * a.w;
    const double* src = a.src + v * 3 * n;
    const double* wts = a.wts + v * 5 * n;
    const double* bb = a.b + v * 3 * n;
    double pj[kRgCells][4], den[kRgCells], b[kRgCells][3];
    int g[kRgCells];
    unsigned has = 0;            // 4 bits per cell: the neighbour j lies inside the region (rg_nbr_mask)
#pragma unroll
    for (int k = 0; k < kRgCells; ++k) {
        const int e = tid + k * kRgThreads;
        g[k] = -1;
        if (e < cells) {
            g[k] = (tl.y0 + e / rw) * a.w + tl.x0 + e % rw;
            has |= (unsigned)rg_nbr_mask(e, rw, rh) << (4 * k);
#pragma unroll
            for (int j = 0; j < 4; ++j) pj[k][j] = wts[j * n + g[k]];
            den[k] = wts[4 * n + g[k]];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                b[k][c] = bb[c * n + g[k]];
                ir[c][e] = src[c * n + g[k]];
            }
        }
    }
    __syncthreads();
    for (int it = 0; it < a.T; ++it) {
        double nv[kRgCells][3];
#pragma unroll
        for (int k = 0; k < kRgCells; ++k) {
            const int e = tid + k * kRgThreads;
            if (e < cells) {
                const unsigned m = has >> (4 * k);
                const int e0 = rg_nbr_at(e, rw, m, 0), e1 = rg_nbr_at(e, rw, m, 1), e2 = rg_nbr_at(e, rw, m, 2), e3 = rg_nbr_at(e, rw, m, 3);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double s = b[k][c] + pj[k][0] * ir[c][e0];
                    s = s + pj[k][1] * ir[c][e1];
                    s = s + pj[k][2] * ir[c][e2];
                    s = s + pj[k][3] * ir[c][e3];
                    nv[k][c] = (s / den[k]) * 0.8 + 0.2 * ir[c][e];
                }
            }
            // one cell's reads and quotients at a time: hoisting the LDS reads of all cells costs more registers than there are
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kRgCells; ++k) {
            const int e = tid + k * kRgThreads;
            if (e < cells) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ir[c][e] = nv[k][c];
            }
        }
        __syncthreads();
    }
    double* dst = a.dst + v * 3 * n;
#pragma unroll
    for (int k = 0; k < kRgCells; ++k) {
        const int e = tid + k * kRgThreads;
        if (e < cells) {
            const int y = tl.y0 + e / rw, x = tl.x0 + e % rw;
            if (y >= tl.oy0 && y < tl.oy1 && x >= tl.ox0 && x < tl.ox1) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[c * n + g[k]] = ir[c][e];
            }
        }
    }
}

struct RgUpArgs {
    const double* in;            // (nimg, 3, h w): the fine iterate
    double* out;                 // in + up(c1 - c0)
    const double* c1;            // (nimg, 3, hc wc): the coarse solution
    const double* c0;            // (nimg, 3, hc wc): the coarse level's first iterate
    int h, w, hc, wc;
    long long total;             // nimg h w
};

__global__ __launch_bounds__(256) void regrain_up_kernel(const RgUpArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const int n = a.h * a.w, nc = a.hc * a.wc;
    const long long v = idx / n;
    const int p = (int)(idx % n);
    const int y = p / a.w, x = p % a.w;
    const int yn = y / 2, yf = rg_up_far(y, a.hc), xn = x / 2, xf = rg_up_far(x, a.wc);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double* c1 = a.c1 + (v * 3 + c) * nc;
        const double* c0 = a.c0 + (v * 3 + c) * nc;
        const double dnn = c1[yn * a.wc + xn] - c0[yn * a.wc + xn], dfn = c1[yf * a.wc + xn] - c0[yf * a.wc + xn];
        const double dnf = c1[yn * a.wc + xf] - c0[yn * a.wc + xf], dff = c1[yf * a.wc + xf] - c0[yf * a.wc + xf];
        const double rn = dnn * 0.75 + dfn * 0.25;           // rows first: column xn, then column xf, of fine row y
        const double rf = dnf * 0.75 + dff * 0.25;
        const double u = rn * 0.75 + rf * 0.25;
        const long long at = (v * 3 + c) * n + p;
        a.out[at] = a.in[at] + u;
    }
}

bool rg_range(int nimg, int H, int W, int levels) {
    return nimg >= 1 && nimg <= (1 << 24) && H >= 1 && W >= 1 && (long long)H * W <= kRgMaxN && levels >= 1 && levels <= kRgMaxLevels;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// moments and linear maps
// ---------------------------------------------------------------------------------------------------------------------------------------
// sh[q][t] += sh[q][t + s], s = 128, 64, .., 1: the fixed tree of every sum here
template <int NQ> __device__ __forceinline__ void mom_tree(double (*sh)[256], int tid) {
    for (int s = 128; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) sh[q][tid] = sh[q][tid] + sh[q][tid + s];
        }
    }
    __syncthreads();
}

// PASS 1: the sums of the three channels; PASS 2: the six sums of (s_a - mu_a) (s_b - mu_b), (a, b) = 00 01 02 11 12 22
template <int PASS> __global__ __launch_bounds__(256) void colour_moments_partial_kernel(const double* points, long long sp, long long sc, int n,
                                                                                         const double* moments, double* partial) {
    constexpr int NQ = PASS == 1 ? 3 : 6;
    __shared__ double sh[NQ][256];
    const int tid = threadIdx.x, set = blockIdx.y, chunk = blockIdx.x;
    const double* pts = points + (long long)set * 3 * n;
    double mu[3] = {0.0, 0.0, 0.0};
    if constexpr (PASS == 2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = moments[(long long)set * 12 + c];
    }
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    for (int j = 0; j < kMomChunk / 256; ++j) {
        const long long i = (long long)chunk * kMomChunk + j * 256 + tid;
        if (i < n) {
            const double s0 = pts[i * sp], s1 = pts[i * sp + sc], s2 = pts[i * sp + 2 * sc];
            if constexpr (PASS == 1) {
                acc[0] = acc[0] + s0, acc[1] = acc[1] + s1, acc[2] = acc[2] + s2;
            } else {
                const double d0 = s0 - mu[0], d1 = s1 - mu[1], d2 = s2 - mu[2];
                acc[0] = acc[0] + d0 * d0, acc[1] = acc[1] + d0 * d1, acc[2] = acc[2] + d0 * d2;
                acc[3] = acc[3] + d1 * d1, acc[4] = acc[4] + d1 * d2, acc[5] = acc[5] + d2 * d2;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) sh[q][tid] = acc[q];
    mom_tree<NQ>(sh, tid);
    if (tid < NQ) partial[((long long)set * gridDim.x + chunk) * 6 + tid] = sh[tid][0];
}

template <int PASS> __global__ __launch_bounds__(256) void colour_moments_final_kernel(const double* partial, int nchunk, int n, double* moments) {
    constexpr int NQ = PASS == 1 ? 3 : 6;
    __shared__ double sh[NQ][256];
    const int tid = threadIdx.x, set = blockIdx.x;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    for (int i = tid; i < nchunk; i += 256) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = acc[q] + partial[((long long)set * nchunk + i) * 6 + q];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) sh[q][tid] = acc[q];
    mom_tree<NQ>(sh, tid);
    double* m = moments + (long long)set * 12;
    const double dn = (double)n;
    if constexpr (PASS == 1) {
        if (tid < 3) m[tid] = sh[tid][0] / dn;
    } else if (tid == 0) {
        const int at[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double cv = sh[q][0] / dn;
            m[3 + at[q][0] * 3 + at[q][1]] = cv;
            m[3 + at[q][1] * 3 + at[q][0]] = cv;
        }
    }
}

// Cyclic Jacobi on the UPPER triangle of a 3 x 3 symmetric matrix: exactly 8 sweeps over (0,1), (0,2), (1,2), no convergence test, a
// rotation skipped when a_pq == 0.  lam = the diagonal left, V = the product of the rotations (columns = eigenvectors).
__device__ void lin_jacobi(const double* in, double* lam, double* V) {
    double a[3][3], v[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            a[i][j] = i <= j ? in[i * 3 + j] : in[j * 3 + i];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2}, Rr[3] = {2, 1, 0};
    for (int sweep = 0; sweep < 8; ++sweep)
        for (int k = 0; k < 3; ++k) {
            const int p = P[k], q = Q[k], r = Rr[k];
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0);
            const double s = t * c;
            a[p][p] = a[p][p] - t * apq;
            a[q][q] = a[q][q] + t * apq;
            a[p][q] = a[q][p] = 0.0;
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
            for (int i = 0; i < 3; ++i) {
                const double vip = v[i][p], viq = v[i][q];
                v[i][p] = c * vip - s * viq;
                v[i][q] = s * vip + c * viq;
            }
        }
    for (int i = 0; i < 3; ++i) {
        lam[i] = a[i][i];
        for (int j = 0; j < 3; ++j) V[i * 3 + j] = v[i][j];
    }
}

// V diag(f) V^T: entry (i, j), i <= j, is ((V_i0 f_0) V_j0 + (V_i1 f_1) V_j1) + (V_i2 f_2) V_j2, mirrored below the diagonal
__device__ void lin_fsym(const double* V, const double* f, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double e = ((V[i * 3] * f[0]) * V[j * 3] + (V[i * 3 + 1] * f[1]) * V[j * 3 + 1]) + (V[i * 3 + 2] * f[2]) * V[j * 3 + 2];
            out[i * 3 + j] = e;
            out[j * 3 + i] = e;
        }
}

__device__ void lin_matmul(const double* X, const double* Y, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = (X[i * 3] * Y[j] + X[i * 3 + 1] * Y[3 + j]) + X[i * 3 + 2] * Y[6 + j];
}

// the 3 x 3 map from the covariance of the image (cs) to that of the palette (ct)
__device__ void lin_map(const double* cs, const double* ct, int mode, double eps, double* A) {
    if (mode == WU_COLOUR_MEANSTD) {
        for (int i = 0; i < 9; ++i) A[i] = 0.0;
        for (int c = 0; c < 3; ++c) A[c * 4] = sqrt(ct[c * 4] / fmax(cs[c * 4], eps));
        return;
    }
    double lam[3], V[9], f[3], g[3], S[9], Si[9], T[9], M[9], Mr[9];
    lin_jacobi(cs, lam, V);
    for (int k = 0; k < 3; ++k) {
        f[k] = sqrt(fmax(lam[k], eps));
        g[k] = 1.0 / f[k];
    }
    lin_fsym(V, f, S);
    lin_fsym(V, g, Si);
    lin_matmul(S, ct, T);
    lin_matmul(T, S, M);
    lin_jacobi(M, lam, V);
    for (int k = 0; k < 3; ++k) f[k] = sqrt(fmax(lam[k], 0.0));
    lin_fsym(V, f, Mr);
    lin_matmul(Si, Mr, T);
    lin_matmul(T, Si, A);
}

struct LinArgs {
    double* state;               // (nimg, 3, n)
    const double* ms;            // (nimg, 12): the moments of every state
    const double* mt;            // (npal, 12): the moments of every palette
    const int* cls;              // (nimg)
    int n, npal, mode;
    double eps;
};

__global__ __launch_bounds__(256) void colour_linear_kernel(const LinArgs a) {
    __shared__ double map[15];                   // A (9), mu_s (3), mu_t (3)
    const int tid = threadIdx.x;
    const long long v = blockIdx.y;
    const int cl = a.cls[v];
    if (cl < 0 || cl >= a.npal) return;          // uniform over the workgroup: an image with no palette is left as it is
    if (tid == 0) {
        const double* ms = a.ms + v * 12;
        const double* mt = a.mt + (long long)cl * 12;
        lin_map(ms + 3, mt + 3, a.mode, a.eps, map);
        for (int c = 0; c < 3; ++c) map[9 + c] = ms[c], map[12 + c] = mt[c];
    }
    __syncthreads();
    double* st = a.state + v * 3 * a.n;
    for (int u = 0; u < kLinPer; ++u) {
        const long long p = ((long long)blockIdx.x * kLinPer + u) * 256 + tid;
        if (p >= a.n) break;
        const double d0 = st[p] - map[9], d1 = st[a.n + p] - map[10], d2 = st[2ll * a.n + p] - map[11];
#pragma unroll
        for (int c = 0; c < 3; ++c) st[(long long)c * a.n + p] = ((map[c * 3] * d0 + map[c * 3 + 1] * d1) + map[c * 3 + 2] * d2) + map[12 + c];
    }
}

}  // namespace

extern "C" int wu_colour_regrain_levels(int H, int W, int n_iters, int min_side) {
    if (H < 1 || W < 1 || n_iters < 1 || n_iters > kRgMaxLevels || min_side < 0) return 0;
    return rg_level_count(H, W, n_iters, min_side);
}

extern "C" size_t wu_colour_regrain_workspace_bytes(int nimg, int H, int W, int levels) {
    if (!rg_range(nimg, H, W, levels)) return 0;
    return (size_t)nimg * (size_t)rg_workspace_doubles(H, W, levels) * sizeof(double);
}

extern "C" int wu_colour_regrain(double* state, const double* original, int nimg, int H, int W, int levels, const int* iters_host,
                                 double smoothness, void* workspace, void* stream) {
    WU_REQUIRE(rg_range(nimg, H, W, levels), "wu_colour_regrain: nimg %d, H %d, W %d (H W <= %d) or levels %d (1..%d) out of range", nimg, H, W,
               kRgMaxN, levels, kRgMaxLevels);
    WU_REQUIRE(state && original && iters_host && workspace, "wu_colour_regrain: NULL pointer");
    WU_REQUIRE(smoothness > 0.0 && smoothness <= 1.79e308, "wu_colour_regrain: smoothness must be positive and finite");
    for (int l = 0; l < levels; ++l)
        WU_REQUIRE(iters_host[l] >= 1 && iters_host[l] <= (1 << 20), "wu_colour_regrain: iters[%d] = %d out of 1..2^20", l, iters_host[l]);
    hipStream_t s = (hipStream_t)stream;
    // the workspace, in planes of (nimg, k, n_l)
    int hs[kRgMaxLevels], ws[kRgMaxLevels];
    double *wts[kRgMaxLevels], *bt[kRgMaxLevels], *i0[kRgMaxLevels], *c0[kRgMaxLevels], *ir[kRgMaxLevels];
    double* at = (double*)workspace;
    double* tmp = at;
    at += (size_t)nimg * 3 * H * W;
    for (int l = 0; l < levels; ++l) {
        rg_level_size(H, W, l, &hs[l], &ws[l]);
        const size_t n = (size_t)nimg * hs[l] * ws[l];
        wts[l] = at, at += 5 * n;
        bt[l] = at, at += 3 * n;
        if (l == 0) {
            i0[0] = const_cast<double*>(original), c0[0] = nullptr, ir[0] = state;
        } else {
            i0[l] = at, at += 3 * n;
            c0[l] = at, at += 3 * n;
            ir[l] = at, at += 3 * n;
        }
    }
    // down the pyramid: the weights and constant terms of every level, from its original and its transfer (the level's first iterate)
    for (int l = 0; l < levels; ++l) {
        RgWeightArgs w;
        w.i0 = i0[l], w.it = ir[l], w.wts = wts[l], w.b = bt[l], w.h = hs[l], w.w = ws[l];
        w.total = (long long)nimg * hs[l] * ws[l];
        w.num = ldexp(30.0, -l), w.smooth = smoothness;
        hipLaunchKernelGGL(regrain_weights_kernel, dim3(rg_grid(w.total)), dim3(256), 0, s, w);
        WU_LAUNCH_CHECK("regrain_weights_kernel");
        if (l + 1 < levels) {
            RgDownArgs d;
            d.i0 = i0[l], d.it = ir[l], d.i0c = i0[l + 1], d.c0 = c0[l + 1], d.irc = ir[l + 1];
            d.h = hs[l], d.w = ws[l], d.hc = hs[l + 1], d.wc = ws[l + 1];
            d.total = (long long)nimg * d.hc * d.wc;
            hipLaunchKernelGGL(regrain_down_kernel, dim3(rg_grid(d.total)), dim3(256), 0, s, d);
            WU_LAUNCH_CHECK("regrain_down_kernel");
        }
    }
    // and up again: solve, then correct the finer level by the change of the coarser one
    const double* coarse = nullptr;                 // where the solution of level l + 1 lies
    for (int l = levels - 1; l >= 0; --l) {
        const int h = hs[l], w = ws[l];
        const bool whole = rg_whole(h, w);
        int launches = 0;
        for (int left = iters_host[l]; left > 0; left -= rg_launch_iters(h, w, left)) ++launches;
        // a tiled launch reads its halo from cells that other workgroups own, so it writes another buffer; with an odd number of such
        // launches the first reads from tmp, so that the last writes the level's own buffer
        double* cur = !whole && (launches & 1) ? tmp : ir[l];
        if (l + 1 < levels) {
            RgUpArgs u;
            u.in = ir[l], u.out = cur, u.c1 = coarse, u.c0 = c0[l + 1], u.h = h, u.w = w, u.hc = hs[l + 1], u.wc = ws[l + 1];
            u.total = (long long)nimg * h * w;
            hipLaunchKernelGGL(regrain_up_kernel, dim3(rg_grid(u.total)), dim3(256), 0, s, u);
            WU_LAUNCH_CHECK("regrain_up_kernel");
        } else if (cur != ir[l]) {
            const hipError_t e = hipMemcpyAsync(cur, ir[l], (size_t)nimg * 3 * h * w * sizeof(double), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) WU_FAIL((int)e, "wu_colour_regrain: hipMemcpyAsync: %s", hipGetErrorString(e));
        }
        for (int left = iters_host[l]; left > 0;) {
            RgSolveArgs a;
            a.T = rg_launch_iters(h, w, left);
            a.src = cur, a.dst = whole ? cur : (cur == tmp ? ir[l] : tmp);
            a.wts = wts[l], a.b = bt[l], a.h = h, a.w = w;
            a.tiles = rg_tiles(h, w, a.T, &a.tiles_x);
            hipLaunchKernelGGL(regrain_solve_kernel, dim3((unsigned)((long long)nimg * a.tiles)), dim3(kRgThreads), 0, s, a);
            WU_LAUNCH_CHECK("regrain_solve_kernel");
            cur = a.dst;
            left -= a.T;
        }
        coarse = cur;                               // == ir[l]
    }
    return 0;
}

extern "C" size_t wu_colour_moments_workspace_bytes(int nsets, int n) {
    if (nsets < 1 || nsets > 65535 || n < 1 || n > kRgMaxN) return 0;
    return (size_t)nsets * cdiv(n, kMomChunk) * 6 * sizeof(double);
}

extern "C" int wu_colour_moments(const double* points, long long stride_point, long long stride_channel, int nsets, int n, double* moments_out,
                                 void* workspace, void* stream) {
    WU_REQUIRE(nsets >= 1 && nsets <= 65535 && n >= 1 && n <= kRgMaxN, "wu_colour_moments: nsets %d (1..65535) or n %d (1..%d) out of range",
               nsets, n, kRgMaxN);
    WU_REQUIRE((stride_point == 1 && stride_channel == n) || (stride_point == 3 && stride_channel == 1),
               "wu_colour_moments: strides (%lld, %lld) are neither planar (1, n) nor interleaved (3, 1)", stride_point, stride_channel);
    WU_REQUIRE(points && moments_out && workspace, "wu_colour_moments: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = cdiv(n, kMomChunk);
    double* partial = (double*)workspace;
    const dim3 grid((unsigned)nchunk, (unsigned)nsets);
    hipLaunchKernelGGL(colour_moments_partial_kernel<1>, grid, dim3(256), 0, s, points, stride_point, stride_channel, n,
                       (const double*)moments_out, partial);
    WU_LAUNCH_CHECK("colour_moments_partial_kernel<1>");
    hipLaunchKernelGGL(colour_moments_final_kernel<1>, dim3((unsigned)nsets), dim3(256), 0, s, (const double*)partial, nchunk, n, moments_out);
    WU_LAUNCH_CHECK("colour_moments_final_kernel<1>");
    hipLaunchKernelGGL(colour_moments_partial_kernel<2>, grid, dim3(256), 0, s, points, stride_point, stride_channel, n,
                       (const double*)moments_out, partial);
    WU_LAUNCH_CHECK("colour_moments_partial_kernel<2>");
    hipLaunchKernelGGL(colour_moments_final_kernel<2>, dim3((unsigned)nsets), dim3(256), 0, s, (const double*)partial, nchunk, n, moments_out);
    WU_LAUNCH_CHECK("colour_moments_final_kernel<2>");
    return 0;
}

extern "C" int wu_colour_linear_apply(double* state, int nimg, int n, const double* state_moments, const double* palette_moments, int npal,
                                      const int* classes, int mode, double eps_var, void* stream) {
    WU_REQUIRE(nimg >= 1 && nimg <= 65535 && n >= 1 && n <= kRgMaxN && npal >= 1 && npal <= (1 << 16),
               "wu_colour_linear_apply: nimg %d (1..65535), n %d (1..%d) or npal %d out of range", nimg, n, kRgMaxN, npal);
    WU_REQUIRE(mode == WU_COLOUR_MEANSTD || mode == WU_COLOUR_MKL, "wu_colour_linear_apply: unknown mode %d", mode);
    WU_REQUIRE(eps_var > 0.0 && eps_var <= 1.79e308, "wu_colour_linear_apply: eps_var must be positive and finite");
    WU_REQUIRE(state && state_moments && palette_moments && classes, "wu_colour_linear_apply: NULL pointer");
    LinArgs a;
    a.state = state, a.ms = state_moments, a.mt = palette_moments, a.cls = classes, a.n = n, a.npal = npal, a.mode = mode, a.eps = eps_var;
    hipLaunchKernelGGL(colour_linear_kernel, dim3((unsigned)cdiv(n, 256 * kLinPer), (unsigned)nimg), dim3(256), 0, (hipStream_t)stream, a);
    WU_LAUNCH_CHECK("colour_linear_kernel");
    return 0;
}
