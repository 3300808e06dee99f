// softpose.hip -- the soft silhouette mode of the object-pose initialisation (homan_amd/pose_optimization.py, sil_mode="soft").
//
//   hm_softsil_pose_terms  per candidate the masked L2 and the IoU of the soft image of hm_softsil_fwd against ONE shared mask,
//                          and the per-sample gradient image of the L2 for hm_softsil_bwd, in one pass over the image;
//   hm_sigma_anneal        the blur schedule's update, sigma <- max(sigma * decay, floor), on the stream.
//
// Every sum is formed in one fixed order and there is no floating-point atomic: a candidate's results are the same bits whatever
// the number of candidates in the launch and from call to call.
#include "hm_common.h"

#define SP_THREADS 256
#define SP_INFLIGHT 4                                   // independent 16-byte loads per lane and image
#define SP_CHUNK_QUADS (SP_THREADS * SP_INFLIGHT)       // a workgroup's pass: 1024 quads = 4096 samples
#define SP_MAX_PARTS 256                                // workgroups per candidate (<= SP_THREADS: one partial per lane at the end)
#define SP_MAX_SIZE 4096

// A candidate's image is a flat array of npix = S * S floats, cut into quads of 4 consecutive samples.  Lane t of the workgroup
// that walks chunk c takes the quads c * 1024 + j * 256 + t, j = 0..3, and adds their samples in ascending order: the
// assignment of samples to lanes, and with it every sum, is the same on the vector path (whole quads as one 16-byte access;
// npix a multiple of 4 and the four images 16-byte aligned) and on the scalar path (any npix, any alignment).  Samples past the
// end are read as alpha = keep = ref = 0: they add +0 to every sum.
template <bool VEC>
__device__ __forceinline__ void sp_load(const float* __restrict__ p, int quad, long npix, float (&v)[4])
{
    const long at = 4l * quad;
    if (VEC) {
        if (at < npix) {
            const float4 q = *reinterpret_cast<const float4*>(p + at);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = v[1] = v[2] = v[3] = 0.f;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = at + e < npix ? p[at + e] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void sp_store(float* __restrict__ p, int quad, long npix, const float (&v)[4])
{
    const long at = 4l * quad;
    if (VEC) {
        if (at < npix) *reinterpret_cast<float4*>(p + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (at + e < npix) p[at + e] = v[e];
    }
}

// grid (workgroups per candidate, candidates).  Workgroup b of a candidate walks the chunks b, b + gridDim.x, ...; its three
// partial sums {sum of squares, intersection, union} go to the workspace, and the candidate's last-arriving workgroup adds the
// partials in ascending workgroup index.
template <bool VEC>
__global__ __launch_bounds__(SP_THREADS) void k_softsil_pose_terms(const float* __restrict__ alpha, const float* __restrict__ keep,
                                                                    const float* __restrict__ ref, long npix,
                                                                    float* __restrict__ terms, float* __restrict__ grad,
                                                                    unsigned int* __restrict__ tickets, float* __restrict__ partials)
{
    __shared__ float red[48];
    __shared__ float s_part[3][SP_MAX_PARTS];
    __shared__ int s_flag;
    const int cand = blockIdx.y, nparts = gridDim.x;
    const int nquads = (int)((npix + 3) >> 2), nchunks = (nquads + SP_CHUNK_QUADS - 1) / SP_CHUNK_QUADS;
    const float* a_img = alpha + (long)cand * npix;
    float* g_img = grad + (long)cand * npix;
    float sums[3] = {0.f, 0.f, 0.f};

    for (int chunk = blockIdx.x; chunk < nchunks; chunk += nparts) {
        const int q0 = chunk * SP_CHUNK_QUADS + threadIdx.x;
        float a[SP_INFLIGHT][4], kp[SP_INFLIGHT][4], rf[SP_INFLIGHT][4];
#pragma unroll
        for (int j = 0; j < SP_INFLIGHT; ++j) sp_load<VEC>(a_img, q0 + j * SP_THREADS, npix, a[j]);
#pragma unroll
        for (int j = 0; j < SP_INFLIGHT; ++j) sp_load<VEC>(keep, q0 + j * SP_THREADS, npix, kp[j]);
#pragma unroll
        for (int j = 0; j < SP_INFLIGHT; ++j) sp_load<VEC>(ref, q0 + j * SP_THREADS, npix, rf[j]);
#pragma unroll
        for (int j = 0; j < SP_INFLIGHT; ++j) {
            float g[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float img = kp[j][e] * a[j][e], d = img - rf[j][e];
                sums[0] += d * d;
                sums[1] += img * rf[j][e];
                sums[2] += fminf(fmaxf(img + rf[j][e], 0.f), 1.f);
                g[e] = 2.f * kp[j][e] * d;
            }
            sp_store<VEC>(g_img, q0 + j * SP_THREADS, npix, g);
        }
    }

    hm_block_sum_n<3>(sums, red);
    float* mine = partials + ((long)cand * nparts + blockIdx.x) * 3;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) hm_partial_store(mine + k, sums[k]);
    }
    if (hm_last_block(tickets + cand, nparts, &s_flag)) {
        const float* all = partials + (long)cand * nparts * 3;
        if ((int)threadIdx.x < nparts) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s_part[k][threadIdx.x] = hm_partial_load(all + 3 * threadIdx.x + k);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float sq = 0.f, in = 0.f, un = 0.f;
            for (int b = 0; b < nparts; ++b) { sq += s_part[0][b]; in += s_part[1][b]; un += s_part[2][b]; }
            terms[2 * cand] = sq;                              // loss_dict["mask"]
            terms[2 * cand + 1] = in / (un + 1e-6f);           // batch_mask_iou
        }
    }
}

// workgroups per candidate: a function of S alone (a candidate's sums do not depend on N)
static inline int sp_parts(int S)
{
    const long nquads = ((long)S * S + 3) / 4;
    const long nchunks = (nquads + SP_CHUNK_QUADS - 1) / SP_CHUNK_QUADS;
    return (int)(nchunks < SP_MAX_PARTS ? nchunks : SP_MAX_PARTS);
}

__global__ void k_sigma_anneal(float* __restrict__ sigma, float decay, float sigma_min)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) sigma[0] = fmaxf(sigma[0] * decay, sigma_min);
}

extern "C" {
size_t hm_softsil_pose_workspace_bytes(int N, int S)
{
    if (N < 1 || N > 65535 || S < 1 || S > SP_MAX_SIZE) return 0;
    return (size_t)N * sizeof(unsigned int) + (size_t)N * sp_parts(S) * 3 * sizeof(float);
}

int hm_softsil_pose_terms(const float* alpha, const float* keep, const float* ref, int N, int S, float* terms, float* grad,
                          void* workspace, hipStream_t stream)
{
    HM_CHECK_ARG(alpha && keep && ref && terms && grad && workspace);
    HM_CHECK_ARG(HM_ALIGNED(workspace, 4));          // 32-bit tickets (atomic targets), then fp32 partial sums
    HM_CHECK_ARG(N >= 1 && N <= 65535 && S >= 1 && S <= SP_MAX_SIZE);
    const long npix = (long)S * S;
    unsigned int* tickets = static_cast<unsigned int*>(workspace);
    float* partials = reinterpret_cast<float*>(tickets + N);
    const bool vec = npix % 4 == 0 && (((uintptr_t)alpha | (uintptr_t)keep | (uintptr_t)ref | (uintptr_t)grad) & 15) == 0;
    const dim3 grid(sp_parts(S), N);
    if (vec)
        k_softsil_pose_terms<true><<<grid, SP_THREADS, 0, stream>>>(alpha, keep, ref, npix, terms, grad, tickets, partials);
    else
        k_softsil_pose_terms<false><<<grid, SP_THREADS, 0, stream>>>(alpha, keep, ref, npix, terms, grad, tickets, partials);
    return hm_launch_status();
}

int hm_sigma_anneal(float* sigma, float decay, float sigma_min, hipStream_t stream)
{
    HM_CHECK_ARG(sigma && decay > 0.f && decay <= 1.f && sigma_min >= 0.f && sigma_min < __builtin_inff());
    k_sigma_anneal<<<1, 64, 0, stream>>>(sigma, decay, sigma_min);
    return hm_launch_status();
}
}
