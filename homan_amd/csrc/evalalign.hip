// evalalign.hip -- the hand protocol's evaluation arithmetic (FreiHAND / HO-3D): a batched similarity alignment with a 3x3
// SVD per frame (k_procrustes), exact threshold curves for PCK / AUC (k_thr_hist, k_thr_scan) and F-scores off the
// nearest-neighbour distances of hm_cloud_metrics (k_fscore).
//
// The protocol's script is not part of the reference tree: the formulas are the ones written in include/homan_amd.h and
// DESIGN.md section 7, pinned by a float64 NumPy restatement (tests/handmetrics_ref.py).  Every floating-point sum is a
// double formed in a fixed order by the workgroup of its own frame (per thread i = t, t + blockDim, ... in order, the DPP
// tree of hm_wave_sum_f64 over a wave, the waves in order): two calls return the same bits and a frame's result does not
// depend on the other frames of the call.  Counters are integers (LDS and global integer atomics only).
#include "hm_common.h"

#define EA_THREADS 256
#define EA_SMALL_N 64            // up to this many points one wave per frame, above it four
#define EA_MAX_GRID 65535        // frames per launch
#define EA_SWEEPS 30             // cap of the Jacobi sweeps (a 3x3 converges in 4-6)
#define EA_TOL2 6.2230152778611417e-31        // 2^-100: a pair of columns is orthogonal when (p.q)^2 <= 2^-100 |p|^2 |q|^2
#define EA_TINY 1e-150           // a column shorter than this has no direction: its left vector is completed
#define EA_XFORM 13
#define EA_MAX_T 8
#define EA_MAX_STEPS 1024
#define EA_HIST_BLOCKS 1024

// One rotation of the one-sided (Hestenes) Jacobi SVD: columns P and Q of A (and of V) are rotated so that the new columns of
// A are orthogonal.  Returns false when they already are, to the tolerance above.
template <int P, int Q>
__host__ __device__ __forceinline__ bool ea_jacobi_pair(double (&A)[3][3], double (&V)[3][3])
{
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) { alpha += A[r][P] * A[r][P]; beta += A[r][Q] * A[r][Q]; gamma += A[r][P] * A[r][Q]; }
    if (gamma * gamma <= EA_TOL2 * (alpha * beta)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double ap = A[r][P], aq = A[r][Q], vp = V[r][P], vq = V[r][Q];
        A[r][P] = c * ap - s * aq;
        A[r][Q] = s * ap + c * aq;
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
    return true;
}

template <int P, int Q>
__host__ __device__ __forceinline__ void ea_sort_pair(double (&A)[3][3], double (&V)[3][3], double (&sg)[3])
{
    if (sg[P] >= sg[Q]) return;
    double t = sg[P]; sg[P] = sg[Q]; sg[Q] = t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        t = A[r][P]; A[r][P] = A[r][Q]; A[r][Q] = t;
        t = V[r][P]; V[r][P] = V[r][Q]; V[r][Q] = t;
    }
}

__host__ __device__ __forceinline__ double ea_det3(const double (&Q)[3][3])
{
    return Q[0][0] * (Q[1][1] * Q[2][2] - Q[1][2] * Q[2][1]) - Q[0][1] * (Q[1][0] * Q[2][2] - Q[1][2] * Q[2][0]) +
           Q[0][2] * (Q[1][0] * Q[2][1] - Q[1][1] * Q[2][0]);
}

// M = U S V^T by one-sided Jacobi in double: sweeps over the column pairs (0,1), (0,2), (1,2) of A = M V until a whole sweep
// rotates nothing (or EA_SWEEPS).  The columns are then sorted by length, longest first: S = their lengths, U = the columns
// over their lengths.  A column without a direction (rank-deficient M: one point, collinear or coplanar sets, zero) is
// replaced by a unit vector orthogonal to the others, so U is orthogonal for every M.  Returns Q = U V^T, the orthogonal
// matrix that maximises trace(Q^T M), and *sigma = trace S; with `proper`, det Q < 0 flips the last column of U and the
// smallest singular value (Kabsch / Umeyama), so Q is the best proper rotation.
__host__ __device__ __forceinline__ void ea_procrustes_q(const double (&M)[3][3], bool proper, double (&Q)[3][3], double* sigma)
{
    double A[3][3], V[3][3], sg[3], U[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { A[r][c] = M[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
    }
    for (int sweep = 0; sweep < EA_SWEEPS; ++sweep) {
        bool moved = ea_jacobi_pair<0, 1>(A, V);
        moved |= ea_jacobi_pair<0, 2>(A, V);
        moved |= ea_jacobi_pair<1, 2>(A, V);
        if (!moved) break;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) sg[c] = sqrt((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
    ea_sort_pair<0, 1>(A, V, sg);
    ea_sort_pair<1, 2>(A, V, sg);
    ea_sort_pair<0, 1>(A, V, sg);
    if (!(sg[0] > EA_TINY)) {                 // M = 0: any orthogonal Q is a minimiser
#pragma unroll
        for (int r = 0; r < 3; ++r) { U[r][0] = r == 0; U[r][1] = r == 1; U[r][2] = r == 2; }
        sg[0] = sg[1] = sg[2] = 0.0;
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) U[r][0] = A[r][0] / sg[0];
        if (!(sg[1] > EA_TINY)) {             // rank 1: the axis least along u0, made orthogonal to it
            const double ax = fabs(U[0][0]), ay = fabs(U[1][0]), az = fabs(U[2][0]);
            const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
            const double d = k == 0 ? U[0][0] : k == 1 ? U[1][0] : U[2][0];
            double w[3], n2 = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) { w[r] = (r == k ? 1.0 : 0.0) - d * U[r][0]; n2 += w[r] * w[r]; }
            const double n = sqrt(n2);
#pragma unroll
            for (int r = 0; r < 3; ++r) U[r][1] = w[r] / n;
            sg[1] = sg[2] = 0.0;
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) U[r][1] = A[r][1] / sg[1];
        }
        if (!(sg[2] > EA_TINY)) {             // rank 2 (or completed rank 1): u2 = u0 x u1
            U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
            U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
            U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
            sg[2] = 0.0;
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) U[r][2] = A[r][2] / sg[2];
        }
    }
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Q[r][c] = (U[r][0] * V[c][0] + U[r][1] * V[c][1]) + U[r][2] * V[c][2];
        }
        if (pass == 1 || !proper || !(ea_det3(Q) < 0.0)) break;
#pragma unroll
        for (int r = 0; r < 3; ++r) U[r][2] = -U[r][2];
        sg[2] = -sg[2];
    }
    *sigma = (sg[0] + sg[1]) + sg[2];
}

// grid (frames of this launch), 64 or 256 threads; frame = b0 + blockIdx.x.  Modes 0 / 1: pass 1 sums the points (means),
// pass 2 the centred norms and M = sum_i pc_i^T gc_i (11 sums), every thread then runs the same SVD on the same M, pass 3
// maps the points.  Mode 2 reads the two anchors and maps the points.  All modes end in
//   y = scale * ((p - cp) Q) + cg     (double),     aligned = (float)y,     err = |y - g|,
// mode 2 with Q = I (its products by 0 and 1 are exact), cp = pred[a], cg = gt[a], scale = k.
__global__ __launch_bounds__(EA_THREADS) void k_procrustes(const float* __restrict__ pred, const float* __restrict__ gt, int N,
                                                            int mode, int anchor_a, int anchor_b, float* __restrict__ aligned,
                                                            double* __restrict__ err, double* __restrict__ xform, int b0)
{
    __shared__ double red[16 * 11];
    const long b = (long)b0 + blockIdx.x;
    const float* p0 = pred + b * N * 3;
    const float* g0 = gt + b * N * 3;
    double Q[3][3], cp[3], cg[3], scale;
    if (mode == 2) {
        double dp2 = 0.0, dg2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            cp[k] = (double)p0[3 * anchor_a + k];
            cg[k] = (double)g0[3 * anchor_a + k];
            const double dp = (double)p0[3 * anchor_b + k] - cp[k], dg = (double)g0[3 * anchor_b + k] - cg[k];
            dp2 += dp * dp;
            dg2 += dg * dg;
        }
        const double den = sqrt(dp2);
        scale = den == 0.0 ? 1.0 : sqrt(dg2) / den;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Q[r][c] = r == c ? 1.0 : 0.0;
        }
    } else {
        double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { m[k] += (double)g0[3 * i + k]; m[3 + k] += (double)p0[3 * i + k]; }
        }
        hm_block_sum_n_f64<6>(m, red);
#pragma unroll
        for (int k = 0; k < 3; ++k) { cg[k] = m[k] / (double)N; cp[k] = m[3 + k] / (double)N; }
        double v[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // |gc|^2, |pc|^2, M row-major
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            double gc[3], pc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { gc[k] = (double)g0[3 * i + k] - cg[k]; pc[k] = (double)p0[3 * i + k] - cp[k]; }
            v[0] += (gc[0] * gc[0] + gc[1] * gc[1]) + gc[2] * gc[2];
            v[1] += (pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[2 + 3 * r + c] += pc[r] * gc[c];
            }
        }
        hm_block_sum_n_f64<11>(v, red);
        const double s1 = sqrt(v[0]) + 1e-8, s2 = sqrt(v[1]) + 1e-8, s12 = s1 * s2;
        double M[3][3], sigma;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) M[r][c] = v[2 + 3 * r + c] / s12;
        }
        ea_procrustes_q(M, mode == 1, Q, &sigma);
        scale = (sigma * s1) / s2;
    }
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        double pc[3], e2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) pc[k] = (double)p0[3 * i + k] - cp[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double y = scale * ((pc[0] * Q[0][c] + pc[1] * Q[1][c]) + pc[2] * Q[2][c]) + cg[c];
            const double d = y - (double)g0[3 * i + c];
            e2 += d * d;
            if (aligned) aligned[(b * N + i) * 3 + c] = (float)y;
        }
        if (err) err[b * N + i] = sqrt(e2);
    }
    if (xform && threadIdx.x == 0) {          // aligned = s * pred * R^T + t (row vectors): R = Q^T, t = cg - s * (cp Q)
        double* x = xform + b * EA_XFORM;
        x[0] = scale;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[1 + 3 * r + c] = Q[c][r];
            x[10 + r] = cg[r] - scale * ((cp[0] * Q[0][r] + cp[1] * Q[1][r]) + cp[2] * Q[2][r]);
        }
    }
}

// t_k of np.linspace(0, val_max, steps): k * step with step = val_max / (steps - 1), the last one val_max itself
__device__ __forceinline__ double ea_threshold(int k, int steps, double val_max, double step)
{
    return k == steps - 1 ? val_max : (double)k * step;
}

// Histogram of "first threshold at or above the distance" into counts (zeroed by the entry point).  The bin is guessed by a
// division and corrected against t_k itself, both ways, so the count is exact.  NaN and distances above val_max count nowhere.
template <typename T>
__global__ __launch_bounds__(EA_THREADS) void k_thr_hist(const T* __restrict__ dist, long n, double val_max, double step,
                                                          int steps, unsigned long long* __restrict__ counts)
{
    __shared__ unsigned int h[EA_MAX_STEPS];
    for (int k = threadIdx.x; k < steps; k += EA_THREADS) h[k] = 0u;
    __syncthreads();
    for (long i = (long)blockIdx.x * EA_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * EA_THREADS) {
        const double d = (double)dist[i];
        if (!(d <= val_max)) continue;
        int k = 0;
        if (d > 0.0) {
            const double g = ceil(d / step);
            k = g >= (double)(steps - 1) ? steps - 1 : (int)g;
        }
        while (k > 0 && d <= ea_threshold(k - 1, steps, val_max, step)) --k;
        while (d > ea_threshold(k, steps, val_max, step)) ++k;          // (ends at steps - 1 at the latest: d <= val_max)
        atomicAdd(&h[k], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < steps; k += EA_THREADS) {
        if (h[k]) atomicAdd(&counts[k], (unsigned long long)h[k]);
    }
}

// one workgroup: counts[k] <- counts[0] + ... + counts[k] (integers)
__global__ __launch_bounds__(EA_MAX_STEPS) void k_thr_scan(unsigned long long* __restrict__ counts, int steps)
{
    __shared__ unsigned long long s[EA_MAX_STEPS];
    const int k = threadIdx.x;
    s[k] = k < steps ? counts[k] : 0ull;
    __syncthreads();
    if (k >= steps) return;
    unsigned long long a = 0ull;
    for (int j = 0; j <= k; ++j) a += s[j];
    counts[k] = a;
}

struct EaThresholds { float th[EA_MAX_T]; };

// grid (frames of this launch): one workgroup per frame counts the points of x and of y under each threshold
__global__ __launch_bounds__(EA_THREADS) void k_fscore(const float* __restrict__ x_d2, const float* __restrict__ y_d2, int N, int M,
                                                        EaThresholds th, int T, double* __restrict__ out, int b0)
{
    __shared__ unsigned int cnt[2 * EA_MAX_T];
    const long b = (long)b0 + blockIdx.x;
    if (threadIdx.x < 2 * EA_MAX_T) cnt[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const float* d2 = side ? y_d2 + b * M : x_d2 + b * N;
        const int n = side ? M : N;
        unsigned int c[EA_MAX_T] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (int i = threadIdx.x; i < n; i += EA_THREADS) {
            const double d = sqrt((double)d2[i]);
#pragma unroll
            for (int t = 0; t < EA_MAX_T; ++t) c[t] += (t < T && d < (double)th.th[t]) ? 1u : 0u;
        }
#pragma unroll
        for (int t = 0; t < EA_MAX_T; ++t) {
            if (c[t]) atomicAdd(&cnt[side * EA_MAX_T + t], c[t]);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < T) {
        const int t = threadIdx.x;
        const double p = (double)cnt[t] / (double)N, r = (double)cnt[EA_MAX_T + t] / (double)M;
        double* o = out + (b * T + t) * 3;
        o[0] = p;
        o[1] = r;
        o[2] = p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0;
    }
}

extern "C" {
int hm_procrustes_align(const float* pred, const float* gt, int B, int N, int mode, int anchor_a, int anchor_b, float* aligned,
                        double* err, double* xform, hipStream_t stream)
{
    HM_CHECK_ARG(pred && gt && B > 0 && N > 0 && N <= 0x7fffffff / 3 && mode >= 0 && mode <= 2);
    HM_CHECK_ARG(mode != 2 || (anchor_a >= 0 && anchor_a < N && anchor_b >= 0 && anchor_b < N));
    const int threads = N <= EA_SMALL_N ? HM_WAVE : EA_THREADS;
    for (int b0 = 0; b0 < B; b0 += EA_MAX_GRID)
        hipLaunchKernelGGL(k_procrustes, dim3(min(B - b0, EA_MAX_GRID)), dim3(threads), 0, stream, pred, gt, N, mode, anchor_a,
                           anchor_b, aligned, err, xform, b0);
    return hm_launch_status();
}

int hm_threshold_counts(const void* dist, long n, int is_f64, const double* val_max, int steps, void* counts, hipStream_t stream)
{
    HM_CHECK_ARG(val_max && counts && n >= 0 && n <= (1L << 40) && (dist || n == 0) && steps >= 2 && steps <= EA_MAX_STEPS);
    // the void pointers: counts are 64-bit words (atomic targets), dist is fp32 or double
    HM_CHECK_ARG(HM_ALIGNED(counts, 8) && HM_ALIGNED(dist, is_f64 ? 8 : 4));
    const double vmax = *val_max;
    HM_CHECK_ARG(vmax > 0.0 && vmax <= 1.7976931348623157e308);
    const double step = vmax / (double)(steps - 1);
    HM_CHECK_ARG(step > 0.0);
    if (hipMemsetAsync(counts, 0, (size_t)steps * sizeof(unsigned long long), stream) != hipSuccess) return HM_ERR_LAUNCH;
    if (n == 0) return HM_OK;
    const long want = (n + EA_THREADS - 1) / EA_THREADS;
    const int blocks = want < EA_HIST_BLOCKS ? (int)want : EA_HIST_BLOCKS;
    if (is_f64)
        hipLaunchKernelGGL(k_thr_hist<double>, dim3(blocks), dim3(EA_THREADS), 0, stream, (const double*)dist, n, vmax, step,
                           steps, (unsigned long long*)counts);
    else
        hipLaunchKernelGGL(k_thr_hist<float>, dim3(blocks), dim3(EA_THREADS), 0, stream, (const float*)dist, n, vmax, step, steps,
                           (unsigned long long*)counts);
    hipLaunchKernelGGL(k_thr_scan, dim3(1), dim3(EA_MAX_STEPS), 0, stream, (unsigned long long*)counts, steps);
    return hm_launch_status();
}

int hm_fscore(const float* x_d2, const float* y_d2, int B, int N, int M, const float* thresholds, int T, double* out,
              hipStream_t stream)
{
    HM_CHECK_ARG(x_d2 && y_d2 && thresholds && out && B > 0 && N > 0 && M > 0 && T >= 1 && T <= EA_MAX_T);
    EaThresholds th;
    for (int t = 0; t < EA_MAX_T; ++t) th.th[t] = t < T ? thresholds[t] : 0.f;
    for (int b0 = 0; b0 < B; b0 += EA_MAX_GRID)
        hipLaunchKernelGGL(k_fscore, dim3(min(B - b0, EA_MAX_GRID)), dim3(EA_THREADS), 0, stream, x_d2, y_d2, N, M, th, T, out,
                           b0);
    return hm_launch_status();
}
}  // extern "C"
