// handinit.hip -- hand initialisation from 21 keypoints (homan_amd/handinit.py; DESIGN.md section 7, "Hand initialisation
// from keypoints").  No reference counterpart: the reference receives its hand start from a pose network (homan/mocap.py:34-113).
//
//   hm_keypoint_terms_clips    keypoint regression off the camera-space MANO vertices, robust 2-D term, root-relative 3-D term,
//                              their per-clip values and the gradient w.r.t. the vertices, in one launch
//   hm_handinit_finish_clips   betas prior (value + gradient), each clip's weighted total, the step's log row
//
// The rules and the order of every sum are stated in include/homan_amd.h; tests/handinit_ref.py restates them in NumPy and the
// kernel is held to that restatement bit for bit.  Compiled with -ffp-contract=off: every product and sum below rounds once.
#include "hm_common.h"

#define HI_THREADS 256
#define HI_V 778
#define HI_K 21

// TREE64: 64 values, one per lane, s[l] += s[l ^ o] for o = 32, 16, ... 1 (every lane ends with the same bits: the addends of
// each level commute)
__device__ __forceinline__ float hi_tree64(float v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// BLOCKSUM: one value per thread of the 256 -> TREE64 per wave, then ((w0 + w1) + w2) + w3; valid in every thread
__device__ __forceinline__ float hi_block_sum(float v, float* red)
{
    v = hi_tree64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (N): one workgroup per row.  The row's vertices sit in LDS (9.3 KB) for the 63 dot products; W is read twice per
// workgroup (regression, gather), both times along v with consecutive lanes on consecutive floats, and stays in L2 (65 KB).
__global__ __launch_bounds__(HI_THREADS) void k_keypoint_terms(
    const float* __restrict__ verts, const float* __restrict__ W, const float* __restrict__ camintr,
    const float* __restrict__ kp2d, const float* __restrict__ c2, const float* __restrict__ s, const float* __restrict__ kp3d,
    const float* __restrict__ c3, float sigma, float znear, float lw2, float lw3, int clip_len, float* __restrict__ keypoints,
    float* __restrict__ unit_grad, float* __restrict__ row_parts, unsigned int* tickets, float* __restrict__ out, int out_stride)
{
    __shared__ float s_x[HI_V * 3];
    __shared__ float s_kp[HI_K * 3], s_g[HI_K * 3], s_h[HI_K * 3];
    __shared__ float red[4];
    __shared__ int s_flag;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int n = blockIdx.x, clip = n / clip_len;
    const long row0 = (long)clip * clip_len;
    const bool has3 = kp3d != nullptr;

    for (int i = t; i < HI_V * 3; i += HI_THREADS) s_x[i] = verts[(long)n * (HI_V * 3) + i];
    // the clip's confidence sums (inputs only: every row of the clip forms the same two floats)
    const int cnt = clip_len * HI_K;
    float a2 = 0.f, a3 = 0.f;
    for (int i = t; i < cnt; i += HI_THREADS) {
        a2 = a2 + c2[row0 * HI_K + i];
        if (has3) a3 = a3 + c3[row0 * HI_K + i];
    }
    const float csum2 = hi_block_sum(a2, red);          // (its barriers also publish s_x)
    const float csum3 = hi_block_sum(a3, red);
    const float coef2 = csum2 > 0.f ? lw2 / csum2 : 0.f;
    const float coef3 = csum3 > 0.f ? lw3 / csum3 : 0.f;

    // regression: wave wv takes keypoints wv, wv + 4, ...; lane l adds vertices l, l + 64, ... in ascending order, then TREE64
    for (int k = wv; k < HI_K; k += 4) {
        float x = 0.f, y = 0.f, z = 0.f;
        for (int v = lane; v < HI_V; v += 64) {
            const float w = W[k * HI_V + v];
            x = x + w * s_x[3 * v];
            y = y + w * s_x[3 * v + 1];
            z = z + w * s_x[3 * v + 2];
        }
        x = hi_tree64(x); y = hi_tree64(y); z = hi_tree64(z);
        if (lane == 0) { s_kp[3 * k] = x; s_kp[3 * k + 1] = y; s_kp[3 * k + 2] = z; }
    }
    __syncthreads();
    if (t < HI_K * 3) keypoints[(long)n * (HI_K * 3) + t] = s_kp[t];

    // per keypoint: thread k
    float cost2 = 0.f, cost3 = 0.f;
    if (t < HI_K) {
        const int k = t;
        const float x = s_kp[3 * k], y = s_kp[3 * k + 1], z = s_kp[3 * k + 2];
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, h0 = 0.f, h1 = 0.f, h2 = 0.f;
        const float conf = c2[(long)n * HI_K + k];
        const float s2 = sigma * sigma;
        if (conf > 0.f) {
            if (z > znear) {
                const float* K = camintr + (long)n * 9;
                const float fx = K[0], cx = K[2], fy = K[4], cy = K[5], sc = s[n];
                const float fxx = fx * x, fyy = fy * y;
                const float px = fxx / z + cx, py = fyy / z + cy;
                const float rx = (px - kp2d[((long)n * HI_K + k) * 2]) / sc;
                const float ry = (py - kp2d[((long)n * HI_K + k) * 2 + 1]) / sc;
                const float u = rx * rx + ry * ry;
                const float den = s2 + u;
                cost2 = conf * ((s2 * u) / den);
                const float q = s2 / den;
                const float g = (conf * (q * q)) * coef2;            // d (lw2 L2d) / d u
                const float gpx = g * ((2.0f * rx) / sc), gpy = g * ((2.0f * ry) / sc);
                g0 = gpx * (fx / z);
                g1 = gpy * (fy / z);
                g2 = -((gpx * fxx + gpy * fyy) / (z * z));
            } else {
                cost2 = conf * s2;
            }
        }
        if (has3) {
            const float conf3 = c3[(long)n * HI_K + k];
            if (conf3 > 0.f) {
                const float* tg = kp3d + ((long)n * HI_K + k) * 3;
                const float d0 = (x - s_kp[0]) - tg[0], d1 = (y - s_kp[1]) - tg[1], d2 = (z - s_kp[2]) - tg[2];
                cost3 = conf3 * ((d0 * d0 + d1 * d1) + d2 * d2);
                const float g = (2.0f * conf3) * coef3;
                h0 = g * d0; h1 = g * d1; h2 = g * d2;
            }
        }
        s_g[3 * k] = g0 + h0; s_g[3 * k + 1] = g1 + h1; s_g[3 * k + 2] = g2 + h2;
        s_h[3 * k] = h0; s_h[3 * k + 1] = h1; s_h[3 * k + 2] = h2;
    }
    __syncthreads();
    if (t < 3 && has3) {               // the 3-D term is relative to keypoint 0: it receives minus the sum, k ascending
        float acc = 0.f;
        for (int k = 0; k < HI_K; ++k) acc = acc + s_h[3 * k + t];
        s_g[t] = s_g[t] - acc;
    }
    __syncthreads();
    // gather: one thread per vertex, k ascending
    for (int v = t; v < HI_V; v += HI_THREADS) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int k = 0; k < HI_K; ++k) {
            const float w = W[k * HI_V + v];
            gx = gx + w * s_g[3 * k];
            gy = gy + w * s_g[3 * k + 1];
            gz = gz + w * s_g[3 * k + 2];
        }
        float* o = unit_grad + ((long)n * HI_V + v) * 3;
        o[0] = gx; o[1] = gy; o[2] = gz;
    }
    // the row's two sums (TREE64 over the keypoints, lanes 21.. hold 0), then the clip's last row adds the rows
    if (wv == 0) {
        const float r2 = hi_tree64(cost2), r3 = hi_tree64(cost3);
        if (t == 0) { hm_partial_store(row_parts + 2 * (long)n, r2); hm_partial_store(row_parts + 2 * (long)n + 1, r3); }
    }
    if (hm_last_block(tickets + clip, (unsigned int)clip_len, &s_flag)) {
        float b2 = 0.f, b3 = 0.f;
        for (int r = t; r < clip_len; r += HI_THREADS) {
            b2 = b2 + hm_partial_load(row_parts + 2 * (row0 + r));
            b3 = b3 + hm_partial_load(row_parts + 2 * (row0 + r) + 1);
        }
        b2 = hi_block_sum(b2, red);
        b3 = hi_block_sum(b3, red);
        if (t == 0) {
            float* o = out + (long)clip * out_stride;
            o[0] = csum2 > 0.f ? b2 / csum2 : 0.f;
            o[1] = csum3 > 0.f ? b3 / csum3 : 0.f;
        }
    }
}

// grid (clips).  vals row of a clip: {L2d, L3d, Lpca, -, -, Lsmooth, Lbeta, total} (slots 2..4 are what hm_priors_fwd_clips
// writes, slot 5 what hm_smooth_fwd_clips writes).
__global__ __launch_bounds__(HI_THREADS) void k_handinit_finish(const float* __restrict__ betas, float* __restrict__ g_betas,
                                                                int clip_len, float* __restrict__ vals, int vals_stride,
                                                                float lw2, float lw3, float lw_pca, float lw_beta,
                                                                float lw_smooth, const int* __restrict__ step, int max_steps,
                                                                float* __restrict__ log)
{
    __shared__ float red[4];
    const int t = threadIdx.x, clip = blockIdx.x;
    const int nb = clip_len * 10;
    const float inv = 1.0f / (float)nb;
    betas += (long)clip * nb;
    float a = 0.f;
    for (int i = t; i < nb; i += HI_THREADS) {
        const float b = betas[i];
        a = a + b * b;
        if (g_betas) g_betas[(long)clip * nb + i] = g_betas[(long)clip * nb + i] + lw_beta * ((2.0f * b) * inv);
    }
    a = hi_block_sum(a, red);
    float* row = vals + (long)clip * vals_stride;
    if (t == 0) {
        const float lb = a * inv;
        row[6] = lb;
        row[7] = (((lw2 * row[0] + lw3 * row[1]) + lw_pca * row[2]) + lw_beta * lb) + lw_smooth * row[5];
    }
    __syncthreads();
    if (log && t < 8) {
        const int r = min(max(step[0], 0), max_steps - 1);
        log[((long)r * gridDim.x + clip) * 8 + t] = row[t];
    }
}

extern "C" {
int hm_keypoint_terms_clips(const float* verts_world, const float* W, const float* camintr, const float* kp2d, const float* c2,
                            const float* s, const float* kp3d, const float* c3, float sigma, float znear, float lw_kp2d,
                            float lw_kp3d, int N, int clip_len, float* keypoints, float* unit_grad, float* row_parts,
                            int* clip_tickets, float* out2, int out_stride, hipStream_t stream)
{
    HM_CHECK_ARG(verts_world && W && camintr && kp2d && c2 && s && keypoints && unit_grad && row_parts && clip_tickets && out2);
    HM_CHECK_ARG((kp3d == nullptr) == (c3 == nullptr));
    HM_CHECK_ARG(N > 0 && clip_len > 0 && N % clip_len == 0 && out_stride >= 0);
    HM_CHECK_ARG(sigma > 0.f);                   // (false for a NaN as well)
    hipLaunchKernelGGL(k_keypoint_terms, dim3(N), dim3(HI_THREADS), 0, stream, verts_world, W, camintr, kp2d, c2, s, kp3d, c3,
                       sigma, znear, lw_kp2d, lw_kp3d, clip_len, keypoints, unit_grad, row_parts, (unsigned int*)clip_tickets,
                       out2, out_stride);
    return hm_launch_status();
}

int hm_handinit_finish_clips(const float* betas, float* g_betas, int N, int clip_len, float* vals, int vals_stride,
                             float lw_kp2d, float lw_kp3d, float lw_pca, float lw_beta, float lw_smooth, const int* step,
                             int max_steps, float* log, hipStream_t stream)
{
    HM_CHECK_ARG(betas && vals && N > 0 && clip_len > 0 && N % clip_len == 0 && vals_stride >= 8);
    HM_CHECK_ARG(!log || (step && max_steps > 0));
    hipLaunchKernelGGL(k_handinit_finish, dim3(N / clip_len), dim3(HI_THREADS), 0, stream, betas, g_betas, clip_len, vals,
                       vals_stride, lw_kp2d, lw_kp3d, lw_pca, lw_beta, lw_smooth, step, max_steps, log);
    return hm_launch_status();
}
}  // extern "C"
