// surfcontact.hip -- the surface contact loss: attraction of the points outside a mesh and repulsion of those inside it, each a
// tanh-saturated EXACT distance to the surface, with the gradients to the points and to the mesh's vertices.  Beyond the
// reference (its contact term as executed is degenerate); the rules are in include/homan_amd.h and DESIGN.md
// section 7, pinned bit for bit by the fp32 NumPy restatement of tests/surfcontact_ref.py: every fp32 operation is IEEE without
// contraction, in the order written here.
//
//   the search          hm_point_mesh_distance (csrc/surfdist.hip), unchanged: (D, face, inside) per point.
//   k_surface_terms     grid (ceil(N/256), frames of this launch), a lane per point.  The lane reloads its winning face and walks
//                       it again with sd_closest_w<true> (surfdist_walk.h: the function that gave D, so q and D are the search's
//                       bits), which also yields the barycentric weights and p - q; forms u, phi and g; writes g / (B N); and
//                       adds -w_k g into the three vertices of the face and u into its frame's loss word - of the attraction
//                       accumulators when the point is outside, of the repulsion accumulators when it is inside.
//   accumulation        each fp32 addend is rounded to the grid 2^L (hm_quant) and added as a 64-bit INTEGER count of quanta
//                       (atomicAdd on unsigned 64-bit words, two's complement): integer sums are exact and do not depend on the
//                       order of the lanes, so the result is a function of the set of addends - the same bits from run to run,
//                       and for a frame alone or in a batch.  The loss words are summed per workgroup in LDS first (one global
//                       atomic per workgroup and term).  No floating-point atomics.
//   k_surface_finish    vertex accumulators -> fp32: (double)count * 2^L / (B N), rounded to fp32 once.
//   k_surface_loss      one workgroup adds the B per-frame loss words of each term - as sum(word >> 32) and sum(word & 2^32 - 1),
//                       which cannot overflow - and forms (double)hi * 2^32 + (double)lo (one rounding, and none below 2^53
//                       quanta), * 2^L, / (B N), rounded to fp32.
//   k_surface_bwd       the autograd backward: the saved unit gradients scaled by the two upstreams.
// The workspace is zeroed on the stream by every call (hipMemsetAsync: a memset node under capture); no host synchronisation.
#include "hm_common.h"
#include "surfdist_walk.h"

#define SC_THREADS 256
#define SC_MAX_GRID_Y 65535

typedef unsigned long long sc_word;

// x rounded to the grid, as a count of quanta (|x| < 2^51 quanta: the host's choice of L guarantees it)
__device__ __forceinline__ sc_word sc_quanta(float x, double magic, double inv_q)
{
    return (sc_word)(long long)(hm_quant(x, magic) * inv_q);
}

__global__ __launch_bounds__(SC_THREADS) void k_surface_terms(
    const float* __restrict__ points, const float* __restrict__ verts, const int* __restrict__ faces,
    const float* __restrict__ weights, const int* __restrict__ face_idx, const int* __restrict__ inside, int N, int V, int F,
    float c_a, float c_r, double magic, double inv_q, double bn, int b0, sc_word* __restrict__ acc_attr,
    sc_word* __restrict__ acc_rep, sc_word* __restrict__ acc_loss, float* __restrict__ grad_points, float* __restrict__ value,
    float* __restrict__ bary)
{
    __shared__ sc_word s_loss[2];
    if (threadIdx.x < 2) s_loss[threadIdx.x] = 0ull;
    __syncthreads();
    const long b = (long)b0 + blockIdx.y;
    const int i = blockIdx.x * SC_THREADS + threadIdx.x;
    if (i < N) {
        const long at = b * N + i;
        const int face = face_idx[at];
        const int in = inside[at] != 0;
        float u = 0.f, g[3] = {0.f, 0.f, 0.f}, w[3] = {0.f, 0.f, 0.f};
        int iv[3] = {0, 0, 0};
        bool valid = false;
        if (face >= 0 && face < F) {
            const float* vb = verts + b * V * 3;
            const float p[3] = {points[3 * at], points[3 * at + 1], points[3 * at + 2]};
            SdFace r;
            sd_load_face(vb, faces, face, V, r);
            if (r.kind != SD_SKIPPED) {                            // (the search never returns a skipped face)
                float q[3], dv[3];
                const float D = sd_closest_w<true>(p, r, q, w, dv);
                valid = D != 0.f;
                if (valid) {
                    const float d = sqrtf(D);
                    const float c = in ? c_r : c_a;
                    const float t = hm_tanh(d / c);
                    const float om = (in || !weights) ? 1.f : weights[i];       // the weights are the attraction's
                    u = om * (c * t);
                    const float phi = om * (1.f - t * t);
#pragma unroll
                    for (int a = 0; a < 3; ++a) g[a] = (phi * dv[a]) / d;
                    iv[0] = faces[3L * face]; iv[1] = faces[3L * face + 1]; iv[2] = faces[3L * face + 2];
                }
            }
        }
        if (grad_points) {
#pragma unroll
            for (int a = 0; a < 3; ++a) grad_points[3 * at + a] = (float)((double)g[a] / bn);
        }
        if (value) value[at] = u;
        if (bary) { bary[3 * at] = w[0]; bary[3 * at + 1] = w[1]; bary[3 * at + 2] = w[2]; }
        if (valid) {
            sc_word* acc = (in ? acc_rep : acc_attr) + b * V * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (w[k] == 0.f) continue;                         // (adds nothing)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const sc_word n = sc_quanta(-(w[k] * g[a]), magic, inv_q);
                    if (n) atomicAdd(&acc[3L * iv[k] + a], n);
                }
            }
            const sc_word n = sc_quanta(u, magic, inv_q);
            if (n) atomicAdd(&s_loss[in], n);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_loss[threadIdx.x]) atomicAdd(&acc_loss[2 * b + threadIdx.x], s_loss[threadIdx.x]);
}

__global__ __launch_bounds__(SC_THREADS) void k_surface_finish(const sc_word* __restrict__ acc, long total, double q, double bn,
                                                                float* __restrict__ out_attr, float* __restrict__ out_rep)
{
    for (long t = (long)blockIdx.x * SC_THREADS + threadIdx.x; t < 2 * total; t += (long)gridDim.x * SC_THREADS) {
        const float v = (float)(((double)(long long)acc[t] * q) / bn);
        if (t < total) out_attr[t] = v;
        else out_rep[t - total] = v;
    }
}

__global__ __launch_bounds__(SC_THREADS) void k_surface_loss(const sc_word* __restrict__ acc_loss, int B, double q, double bn,
                                                              float* __restrict__ out)
{
    __shared__ sc_word s_hi[2], s_lo[2];
    if (threadIdx.x < 2) { s_hi[threadIdx.x] = 0ull; s_lo[threadIdx.x] = 0ull; }
    __syncthreads();
    long long hi[2] = {0, 0}, lo[2] = {0, 0};
    for (long b = threadIdx.x; b < B; b += SC_THREADS) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long s = (long long)acc_loss[2 * b + k];
            hi[k] += s >> 32;                                      // (arithmetic: floor(s / 2^32))
            lo[k] += s & 0xffffffffll;
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (hi[k]) atomicAdd(&s_hi[k], (sc_word)hi[k]);
        if (lo[k]) atomicAdd(&s_lo[k], (sc_word)lo[k]);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double sum = (double)(long long)s_hi[threadIdx.x] * 4294967296.0 + (double)(long long)s_lo[threadIdx.x];
        out[threadIdx.x] = (float)((sum * q) / bn);
    }
}

__global__ __launch_bounds__(SC_THREADS) void k_surface_bwd(const float* __restrict__ unit_points, const int* __restrict__ inside,
                                                             const float* __restrict__ unit_attr, const float* __restrict__ unit_rep,
                                                             const float* __restrict__ upstream, long n_points, long n_verts,
                                                             float* __restrict__ grad_points, float* __restrict__ grad_verts)
{
    const float ga = upstream[0], gr = upstream[1];
    const long np3 = grad_points ? 3 * n_points : 0, nv3 = grad_verts ? 3 * n_verts : 0;
    for (long t = (long)blockIdx.x * SC_THREADS + threadIdx.x; t < np3 + nv3; t += (long)gridDim.x * SC_THREADS) {
        if (t < np3) grad_points[t] = (inside[t / 3] ? gr : ga) * unit_points[t];
        else grad_verts[t - np3] = ga * unit_attr[t - np3] + gr * unit_rep[t - np3];
    }
}

// the workspace: accumulators (64-bit words: attraction (B,V,3), repulsion (B,V,3), loss (B,2)), then the search's own workspace
// (64-bit aligned), then the face index (B,N) for callers that do not ask for it
static inline size_t sc_acc_words(int B, int V) { return (size_t)B * (size_t)V * 6 + (size_t)B * 2; }
static inline size_t sc_search_bytes(int B, int N, int F) { return (hm_point_mesh_workspace_bytes(B, N, F) + 7) / 8 * 8; }

extern "C" {
size_t hm_surface_contact_workspace_bytes(int B, int N, int V, int F)
{
    if (B <= 0 || N <= 0 || V <= 0 || F <= 0) return 0;
    return sc_acc_words(B, V) * sizeof(sc_word) + sc_search_bytes(B, N, F) + (size_t)B * (size_t)N * sizeof(int);
}

int hm_surface_contact_fwd(const float* points, const float* verts, const int* faces, const float* weights, int B, int N, int V,
                           int F, float contact_thresh, float collision_thresh, int log2q, float* out, float* grad_points,
                           int* inside, float* grad_verts_attr, float* grad_verts_rep, float* value, float* bary, float* d2,
                           int* face_idx, void* workspace, hipStream_t stream)
{
    HM_CHECK_ARG(points && verts && faces && B > 0 && N > 0 && V > 0 && F > 0);
    HM_CHECK_ARG(out && grad_points && inside && grad_verts_attr && grad_verts_rep && workspace);
    HM_CHECK_ARG(contact_thresh > 0.f && collision_thresh > 0.f && contact_thresh <= 3.4028234e38f &&
                 collision_thresh <= 3.4028234e38f);         // (a NaN fails)
    HM_CHECK_ARG(log2q >= -100 && log2q <= 100);
    HM_CHECK_ARG(HM_ALIGNED(workspace, 8));          // 64-bit accumulator words, the targets of integer atomics, at its base
    const size_t acc_bytes = sc_acc_words(B, V) * sizeof(sc_word);
    sc_word* acc = (sc_word*)workspace;
    sc_word* acc_attr = acc;
    sc_word* acc_rep = acc + (size_t)B * V * 3;
    sc_word* acc_loss = acc + (size_t)B * V * 6;
    char* search_ws = (char*)workspace + acc_bytes;
    int* face_ws = face_idx ? face_idx : (int*)(search_ws + sc_search_bytes(B, N, F));
    if (hipMemsetAsync(acc, 0, acc_bytes, stream) != hipSuccess) return HM_ERR_LAUNCH;
    const int rc = hm_point_mesh_distance(points, verts, faces, B, N, V, F, d2, face_ws, inside, nullptr, search_ws, stream);
    if (rc != HM_OK) return rc;
    const double q = __builtin_ldexp(1.0, log2q), inv_q = __builtin_ldexp(1.0, -log2q);
    const double magic = 6755399441055744.0 /* 1.5 * 2^52 */ * q;
    const double bn = (double)((long)B * N);
    for (int b0 = 0; b0 < B; b0 += SC_MAX_GRID_Y) {          // the frame axis in launches of at most 65535 frames
        const int nb = min(B - b0, SC_MAX_GRID_Y);
        hipLaunchKernelGGL(k_surface_terms, dim3(hm_cdiv(N, SC_THREADS), nb), dim3(SC_THREADS), 0, stream, points, verts, faces,
                           weights, (const int*)face_ws, (const int*)inside, N, V, F, contact_thresh, collision_thresh, magic,
                           inv_q, bn, b0, acc_attr, acc_rep, acc_loss, grad_points, value, bary);
    }
    const long total = (long)B * V * 3;
    const long want = (2 * total + SC_THREADS - 1) / SC_THREADS;
    hipLaunchKernelGGL(k_surface_finish, dim3(want < 4096 ? (int)want : 4096), dim3(SC_THREADS), 0, stream, (const sc_word*)acc,
                       total, q, bn, grad_verts_attr, grad_verts_rep);
    hipLaunchKernelGGL(k_surface_loss, dim3(1), dim3(SC_THREADS), 0, stream, (const sc_word*)acc_loss, B, q, bn, out);
    return hm_launch_status();
}

int hm_surface_contact_bwd(const float* unit_points, const int* inside, const float* unit_verts_attr,
                           const float* unit_verts_rep, const float* upstream, long n_points, long n_verts, float* grad_points,
                           float* grad_verts, hipStream_t stream)
{
    HM_CHECK_ARG(upstream && n_points >= 0 && n_verts >= 0 && (grad_points || grad_verts));
    HM_CHECK_ARG(!grad_points || (unit_points && inside));
    HM_CHECK_ARG(!grad_verts || (unit_verts_attr && unit_verts_rep));
    const long n = 3 * ((grad_points ? n_points : 0) + (grad_verts ? n_verts : 0));
    if (n == 0) return HM_OK;
    const long want = (n + SC_THREADS - 1) / SC_THREADS;
    hipLaunchKernelGGL(k_surface_bwd, dim3(want < 4096 ? (int)want : 4096), dim3(SC_THREADS), 0, stream, unit_points, inside,
                       unit_verts_attr, unit_verts_rep, upstream, n_points, n_verts, grad_points, grad_verts);
    return hm_launch_status();
}
}  // extern "C"
