// pointmetrics.hip -- evaluation metrics between two point clouds of unrelated sizes: chamfer, ADD-S, paired vertex error
// and the hand-aligned variants.
//
// Replaces the pytorch3d `chamfer_distance` and scipy `cKDTree` calls of reference homan/eval/pointmetrics.py:17-99 by an
// exact brute-force nearest-neighbour search in both directions (k_cloud_nn), a per-frame fold of its partial sums
// (k_cloud_fold) and the centroid / scale statistics of the hand alignment (k_align_stats).  Every sum is formed in a
// fixed order by the workgroups of its own frame: a frame's result does not depend on the other frames of the launch.
#include "hm_common.h"
#include "pair_bodies.h"     // rl_f, NN_HV (128 queries per workgroup), NN_WAVES (waves splitting the targets)

#define PM_AFF 5             // per-frame affine row (cx, cy, cz, div, mul): p' = ((p - c) / div) * mul
#define PM_PART 3            // per-workgroup partials: sum d2, sum sqrt(d2), sum of the paired distances
#define PM_FOLD_THREADS 256
#define PM_ALIGN_THREADS 256
#define PM_MAX_GRID_Y 65535

__device__ __forceinline__ void pm_load(const float* __restrict__ p, const float* __restrict__ aff, float& x, float& y,
                                        float& z)
{
    x = p[0]; y = p[1]; z = p[2];
    if (aff) {
        x = ((x - aff[0]) / aff[3]) * aff[4];
        y = ((y - aff[1]) / aff[3]) * aff[4];
        z = ((z - aff[2]) / aff[3]) * aff[4];
    }
}

__device__ __forceinline__ float pm_d2(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }

// grid (ceil(N/128) + ceil(M/128), frames of this launch); frame = b0 + blockIdx.y.  The first ceil(N/128) workgroups of a
// frame take 128 queries of X and search Y, the others take 128 queries of Y and search X.  Layout of nn_full_body
// (pair_bodies.h): two queries per lane, wave q scans an equal contiguous share of the targets 64 at a time (coalesced load,
// v_readlane broadcast), minima merged on (d2, index) so that ties keep the lowest index.  Each workgroup stores its sums
// of d2 and of sqrt(d2) (double) and, X side with N == M, of |x_i - y_i| to its own slot of `partials`.
__global__ __launch_bounds__(64 * NN_WAVES) void k_cloud_nn(const float* __restrict__ x, const float* __restrict__ y, int N,
                                                             int M, const float* __restrict__ aff_x,
                                                             const float* __restrict__ aff_y, float* __restrict__ x_d2,
                                                             int* __restrict__ x_idx, float* __restrict__ y_d2,
                                                             int* __restrict__ y_idx, double* __restrict__ partials, int b0)
{
    __shared__ float s_d[NN_WAVES][NN_HV];
    __shared__ int s_i[NN_WAVES][NN_HV];
    __shared__ double s_v[PM_PART][NN_HV];
    __shared__ double s_q[PM_PART][4];
    const long b = (long)b0 + blockIdx.y;
    const int nbx = (N + NN_HV - 1) / NN_HV;
    const bool fwd = (int)blockIdx.x < nbx;
    const bool paired = fwd && N == M;
    const int bx = fwd ? blockIdx.x : blockIdx.x - nbx;
    const int Nq = fwd ? N : M, Nt = fwd ? M : N;
    const float* qp = (fwd ? x : y) + b * Nq * 3;
    const float* tp = (fwd ? y : x) + b * Nt * 3;
    const float* qa = fwd ? aff_x : aff_y;
    const float* ta = fwd ? aff_y : aff_x;
    qa = qa ? qa + b * PM_AFF : nullptr;
    ta = ta ? ta + b * PM_AFF : nullptr;
    float* o_d2 = fwd ? x_d2 : y_d2;
    int* o_idx = fwd ? x_idx : y_idx;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    float hx[2], hy[2], hz[2], best[2];
    int besti[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = bx * NN_HV + lane + 64 * u;
        hx[u] = hy[u] = hz[u] = 0.f;
        if (i < Nq) pm_load(qp + (long)i * 3, qa, hx[u], hy[u], hz[u]);
        best[u] = __builtin_inff();
        besti[u] = 0;
    }
    const int share = (Nt + NN_WAVES - 1) / NN_WAVES, jend = min(Nt, (q + 1) * share);
    for (int j0 = q * share; j0 < jend; j0 += 64) {
        const int n = min(64, jend - j0);
        float ox = 0.f, oy = 0.f, oz = 0.f;
        if (lane < n) pm_load(tp + (long)(j0 + lane) * 3, ta, ox, oy, oz);
        int k = 0;
#define PM_STEP(K)                                                                                   \
    {                                                                                                \
        const float sx = rl_f(ox, (K)), sy = rl_f(oy, (K)), sz = rl_f(oz, (K));                      \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                              \
            const float d = pm_d2(sx - hx[u], sy - hy[u], sz - hz[u]);                               \
            const bool lt = d < best[u];                                                             \
            best[u] = lt ? d : best[u];                                                              \
            besti[u] = lt ? j0 + (K) : besti[u];                                                     \
        }                                                                                            \
    }
        for (; k + 4 <= n; k += 4) { PM_STEP(k) PM_STEP(k + 1) PM_STEP(k + 2) PM_STEP(k + 3) }
        for (; k < n; ++k) PM_STEP(k)
#undef PM_STEP
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) { s_d[q][lane + 64 * u] = best[u]; s_i[q][lane + 64 * u] = besti[u]; }
    if (q == 0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = bx * NN_HV + lane + 64 * u;
            double pv = 0.0;
            if (paired && i < N) {
                float px, py, pz;
                pm_load(y + (b * N + i) * 3, aff_y ? aff_y + b * PM_AFF : nullptr, px, py, pz);
                pv = sqrt((double)pm_d2(hx[u] - px, hy[u] - py, hz[u] - pz));
            }
            s_v[2][lane + 64 * u] = pv;
        }
    }
    __syncthreads();
    if (threadIdx.x < NN_HV) {
        const int t = threadIdx.x, i = bx * NN_HV + t;
        float bd = s_d[0][t];
        int bi = s_i[0][t];
#pragma unroll
        for (int w = 1; w < NN_WAVES; ++w) {
            const float d = s_d[w][t];
            const int id = s_i[w][t];
            if (d < bd || (d == bd && id < bi)) { bd = d; bi = id; }
        }
        double dv = 0.0, sv = 0.0;
        if (i < Nq) {
            if (o_d2) o_d2[b * Nq + i] = bd;
            if (o_idx) o_idx[b * Nq + i] = bi;
            dv = (double)bd;
            sv = sqrt(dv);
        }
        s_v[0][t] = dv;
        s_v[1][t] = sv;
    }
    __syncthreads();
    // fixed-order sums of the 128 values: four serial quarters per quantity, then the quarters in order
    if (threadIdx.x < PM_PART * 4) {
        const int k = threadIdx.x >> 2, r = threadIdx.x & 3;
        double a = 0.0;
        for (int t = r * (NN_HV / 4); t < (r + 1) * (NN_HV / 4); ++t) a += s_v[k][t];
        s_q[k][r] = a;
    }
    __syncthreads();
    if (threadIdx.x < PM_PART) {
        const int k = threadIdx.x;
        partials[(b * gridDim.x + blockIdx.x) * PM_PART + k] = ((s_q[k][0] + s_q[k][1]) + s_q[k][2]) + s_q[k][3];
    }
}

// one thread per frame: the frame's workgroup partials in block order -> out4 (B,4) double
// {mean d2 X->Y, mean d2 Y->X, mean distance X->Y, mean paired distance (NaN when N != M)}
__global__ __launch_bounds__(PM_FOLD_THREADS) void k_cloud_fold(const double* __restrict__ partials, int B, int N, int M,
                                                                 double* __restrict__ out4)
{
    const long b = (long)blockIdx.x * PM_FOLD_THREADS + threadIdx.x;
    if (b >= B) return;
    const int nbx = (N + NN_HV - 1) / NN_HV, nby = (M + NN_HV - 1) / NN_HV;
    const double* p = partials + b * (nbx + nby) * PM_PART;
    double d2x = 0.0, dx = 0.0, pr = 0.0, d2y = 0.0;
    for (int k = 0; k < nbx; ++k) { d2x += p[k * PM_PART]; dx += p[k * PM_PART + 1]; pr += p[k * PM_PART + 2]; }
    for (int k = nbx; k < nbx + nby; ++k) d2y += p[k * PM_PART];
    out4[b * 4 + 0] = d2x / N;
    out4[b * 4 + 1] = d2y / M;
    out4[b * 4 + 2] = dx / N;
    out4[b * 4 + 3] = N == M ? pr / N : __builtin_nan("");
}

// fixed-order block sum of K doubles per thread (tree over the 256 threads); every thread gets the totals
template <int K>
__device__ __forceinline__ void pm_block_sum(double (&v)[K], double (*s)[PM_ALIGN_THREADS])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k][t] = v[k];
    __syncthreads();
    for (int w = PM_ALIGN_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k][t] += s[k][t + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = s[k][0];
    __syncthreads();
}

// grid (B): one workgroup per frame.  Hands are rows b*hands + k (frame-major, hand-minor); the first hand of the frame
// gives the centroids c_gt, c_pred (c_pred = c_gt when pred_centroid_from_gt) and the scales s = sqrt(sum |v - c|^2 / V),
// all in double and rounded to fp32.  aff_gt = (c_gt, 1, 1), aff_pred = (c_pred, s_pred, s_gt) for the object search;
// hand_mean[b*hands + k] = mean_i |(g_i - c_gt) - ((p_i - c_pred) / s_pred) * s_gt| (fp32 vectors, double norm and mean).
__global__ __launch_bounds__(PM_ALIGN_THREADS) void k_align_stats(const float* __restrict__ gt, const float* __restrict__ pred,
                                                                   int hands, int V, int pred_centroid_from_gt,
                                                                   float* __restrict__ aff_gt, float* __restrict__ aff_pred,
                                                                   double* __restrict__ hand_mean)
{
    __shared__ double s[6][PM_ALIGN_THREADS];
    const long b = blockIdx.x;
    const float* g0 = gt + b * hands * V * 3;
    const float* p0 = pred + b * hands * V * 3;
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < V; i += PM_ALIGN_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { c[k] += (double)g0[3 * i + k]; c[3 + k] += (double)p0[3 * i + k]; }
    }
    pm_block_sum<6>(c, s);
    float cg[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cg[k] = (float)(c[k] / V);
        cp[k] = pred_centroid_from_gt ? cg[k] : (float)(c[3 + k] / V);
    }
    double r[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < V; i += PM_ALIGN_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dg = (double)(g0[3 * i + k] - cg[k]), dp = (double)(p0[3 * i + k] - cp[k]);
            r[0] += dg * dg;
            r[1] += dp * dp;
        }
    }
    pm_block_sum<2>(r, s);
    const float sg = (float)sqrt(r[0] / V), sp = (float)sqrt(r[1] / V);
    if (threadIdx.x == 0) {
        float* ag = aff_gt + b * PM_AFF;
        float* ap = aff_pred + b * PM_AFF;
        ag[0] = cg[0]; ag[1] = cg[1]; ag[2] = cg[2]; ag[3] = 1.f; ag[4] = 1.f;
        ap[0] = cp[0]; ap[1] = cp[1]; ap[2] = cp[2]; ap[3] = sp; ap[4] = sg;
    }
    for (int h = 0; h < hands; ++h) {
        const float* gh = g0 + (long)h * V * 3;
        const float* ph = p0 + (long)h * V * 3;
        double a[1] = {0.0};
        for (int i = threadIdx.x; i < V; i += PM_ALIGN_THREADS) {
            float d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = (gh[3 * i + k] - cg[k]) - ((ph[3 * i + k] - cp[k]) / sp) * sg;
            a[0] += sqrt((double)pm_d2(d[0], d[1], d[2]));
        }
        pm_block_sum<1>(a, s);
        if (threadIdx.x == 0) hand_mean[b * hands + h] = a[0] / V;
    }
}

extern "C" {
size_t hm_cloud_metrics_workspace_bytes(int B, int N, int M)
{
    if (B <= 0 || N <= 0 || M <= 0) return 0;
    return (size_t)B * (size_t)(hm_cdiv(N, NN_HV) + hm_cdiv(M, NN_HV)) * PM_PART * sizeof(double);
}

int hm_cloud_metrics(const float* x, const float* y, int B, int N, int M, const float* aff_x, const float* aff_y, float* x_d2,
                     int* x_idx, float* y_d2, int* y_idx, double* out4, void* workspace, hipStream_t stream)
{
    HM_CHECK_ARG(x && y && out4 && workspace && B > 0 && N > 0 && M > 0);
    HM_CHECK_ARG(HM_ALIGNED(workspace, 8));          // double partial sums
    const int nblk = hm_cdiv(N, NN_HV) + hm_cdiv(M, NN_HV);
    for (int b0 = 0; b0 < B; b0 += PM_MAX_GRID_Y) {      // the frame axis in launches of at most 65535 frames
        const int nb = min(B - b0, PM_MAX_GRID_Y);
        hipLaunchKernelGGL(k_cloud_nn, dim3(nblk, nb), dim3(64 * NN_WAVES), 0, stream, x, y, N, M, aff_x, aff_y, x_d2, x_idx,
                           y_d2, y_idx, (double*)workspace, b0);
    }
    hipLaunchKernelGGL(k_cloud_fold, dim3(hm_cdiv(B, PM_FOLD_THREADS)), dim3(PM_FOLD_THREADS), 0, stream,
                       (const double*)workspace, B, N, M, out4);
    return hm_launch_status();
}

int hm_align_stats(const float* gt_hand, const float* pred_hand, int B, int hands, int V, int pred_centroid_from_gt,
                   float* aff_gt, float* aff_pred, double* hand_mean, hipStream_t stream)
{
    HM_CHECK_ARG(gt_hand && pred_hand && aff_gt && aff_pred && hand_mean && B > 0 && hands > 0 && V > 0);
    hipLaunchKernelGGL(k_align_stats, dim3(B), dim3(PM_ALIGN_THREADS), 0, stream, gt_hand, pred_hand, hands, V,
                       pred_centroid_from_gt, aff_gt, aff_pred, hand_mean);
    return hm_launch_status();
}
}  // extern "C"
