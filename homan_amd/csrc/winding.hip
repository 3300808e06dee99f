// winding.hip -- the generalised winding number (Jacobson et al. 2013) of points against a triangle mesh: the inside-outside sign
// for meshes that are NOT closed, behind ops.point_mesh_winding and the sign="winding" mode of the surface metrics.  Beyond the
// reference; the rules are in include/homan_amd.h and DESIGN.md section 7, pinned bit for bit by the NumPy restatement of
// tests/winding_ref.py: every operation is IEEE double from the fp32 inputs, without contraction, in the order written here.
//
//   k_point_mesh_winding  the shape of k_point_mesh (csrc/surfdist.hip): grid (ceil(N/256), splits, frames of this launch).  A lane
//                         owns a point (three doubles); the 256 threads stage the workgroup's faces through LDS 256 at a time as
//                         the search's records, one per thread, and every lane walks the same record (LDS broadcast reads): the
//                         signed solid angle of the face by Van Oosterom and Strackee, 2 hm_atan2(num, den), rounded to the grid
//                         2^log2q by the magic-number add and counted in quanta as a signed 64-bit integer.
//   splits == 1           the lane stores its count and its flag itself.
//   splits > 1            the faces of a frame are dealt to `splits` workgroups by sd_splits; the entry point clears the counts
//                         (hipMemsetAsync), every lane merges with ONE 64-bit integer atomicAdd on its output word (consecutive
//                         lanes, consecutive words), and k_winding_sign forms the flags after; all ordered on the stream.
// A sum of integers depends neither on the order of the faces, nor on the split, nor on the batch.  No floating-point atomics;
// no workgroup waits for another.
#include "hm_common.h"
#include "surfdist_walk.h"   // SdFace, sd_load_face, sd_finite; SD_THREADS, SD_CHUNK, SD_MAX_GRID_Z, sd_splits

#define WN_LOG2Q_MIN (-47)               // below it |omega| < 8 leaves the exact range 2^51 quanta of the magic-number add

__device__ __forceinline__ double wn_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// signed solid angle of the face (a, b, c) seen from p
__device__ __forceinline__ double wn_omega(const double* p, const SdFace& r)
{
    const double A[3] = {(double)r.a[0] - p[0], (double)r.a[1] - p[1], (double)r.a[2] - p[2]};
    const double B[3] = {(double)r.b[0] - p[0], (double)r.b[1] - p[1], (double)r.b[2] - p[2]};
    const double C[3] = {(double)r.c[0] - p[0], (double)r.c[1] - p[1], (double)r.c[2] - p[2]};
    const double la = __builtin_sqrt(wn_dot(A, A)), lb = __builtin_sqrt(wn_dot(B, B)), lc = __builtin_sqrt(wn_dot(C, C));
    const double cx = B[1] * C[2] - B[2] * C[1], cy = B[2] * C[0] - B[0] * C[2], cz = B[0] * C[1] - B[1] * C[0];
    const double num = (A[0] * cx + A[1] * cy) + A[2] * cz;
    if (num == 0.0) return 0.0;                // in the face's plane, at a vertex
    const double den = (((la * lb) * lc + wn_dot(A, B) * lc) + wn_dot(B, C) * la) + wn_dot(C, A) * lb;
    return 2.0 * hm_atan2(num, den);
}

__device__ __forceinline__ int wn_flag(long long count, long long thresh) { return (count < 0 ? -count : count) > thresh ? 1 : 0; }

__global__ __launch_bounds__(SD_THREADS) void k_point_mesh_winding(const float* __restrict__ points,
                                                                    const float* __restrict__ verts,
                                                                    const int* __restrict__ faces, int N, int V, int F,
                                                                    int chunks_per_split, double magic, double per_quantum,
                                                                    long long thresh, long long* __restrict__ count,
                                                                    int* __restrict__ inside, int b0)
{
    __shared__ __attribute__((aligned(16))) SdFace s_face[SD_CHUNK];
    const long b = (long)b0 + blockIdx.z;
    const int i = blockIdx.x * SD_THREADS + threadIdx.x;
    const float* vb = verts + b * V * 3;
    const long at = b * N + i;
    float pf[3] = {0.f, 0.f, 0.f};
    const bool live = i < N;
    if (live) {
        pf[0] = points[3 * at]; pf[1] = points[3 * at + 1]; pf[2] = points[3 * at + 2];
    }
    const bool ok = live && sd_finite(pf[0]) && sd_finite(pf[1]) && sd_finite(pf[2]);
    const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
    long long sum = 0;
    const long f_begin = (long)blockIdx.y * chunks_per_split * SD_CHUNK;
    const long f_stop = f_begin + (long)chunks_per_split * SD_CHUNK, f_end = f_stop < F ? f_stop : (long)F;
    for (long f0 = f_begin; f0 < f_end; f0 += SD_CHUNK) {
        const int n = f_end - f0 < SD_CHUNK ? (int)(f_end - f0) : SD_CHUNK;
        __syncthreads();                                           // the previous chunk has been walked by every wave
        if ((int)threadIdx.x < n) sd_load_face(vb, faces, f0 + threadIdx.x, V, s_face[threadIdx.x]);
        __syncthreads();
        if (!ok) continue;
        for (int k = 0; k < n; ++k) {
            const SdFace& r = s_face[k];
            if (r.kind != SD_TRIANGLE) continue;                   // skipped, or of zero area (the same for every lane)
            const double q = (wn_omega(p, r) + magic) - magic;     // to the grid, ties to even
            sum += (long long)(q * per_quantum);                   // (exact: a whole number of quanta below 2^51)
        }
    }
    if (!live) return;
    if (gridDim.y == 1) {
        count[at] = sum;
        if (inside) inside[at] = wn_flag(sum, thresh);
        return;
    }
    if (sum != 0) atomicAdd((unsigned long long*)&count[at], (unsigned long long)sum);
}

__global__ __launch_bounds__(SD_THREADS) void k_winding_sign(const long long* __restrict__ count, long total, long long thresh,
                                                              int* __restrict__ inside)
{
    for (long t = (long)blockIdx.x * SD_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * SD_THREADS)
        inside[t] = wn_flag(count[t], thresh);
}

extern "C" {
int hm_point_mesh_winding(const float* points, const float* verts, const int* faces, int B, int N, int V, int F, int log2q,
                          void* count, int* inside, hipStream_t stream)
{
    HM_CHECK_ARG(points && verts && faces && count && B > 0 && N > 0 && V > 0 && F > 0);
    HM_CHECK_ARG(HM_ALIGNED(count, 8));              // signed 64-bit words, the targets of atomicAdd
    int bits = 0;                                    // ceil(log2(F))
    while (((long)1 << bits) < (long)F) ++bits;
    // |omega| < 8 = 2^3: F addends stay below 2^(bits + 3 - log2q) <= 2^62 quanta
    HM_CHECK_ARG(log2q >= WN_LOG2Q_MIN && log2q >= bits - 59 && log2q <= 0);
    const double magic = 6755399441055744.0 /* 1.5 * 2^52 */ * __builtin_ldexp(1.0, log2q);
    const double per_quantum = __builtin_ldexp(1.0, -log2q);
    const long long thresh = (long long)__builtin_rint(__builtin_ldexp(6.283185307179586, -log2q));     // |w| > 0.5
    int per;
    const int splits = sd_splits(B, N, F, &per);
    const long total = (long)B * N;                  // every index of the kernels is a 64-bit product of the int sizes
    if (splits > 1 && hipMemsetAsync(count, 0, (size_t)total * sizeof(long long), stream) != hipSuccess) return HM_ERR_LAUNCH;
    for (int b0 = 0; b0 < B; b0 += SD_MAX_GRID_Z) {     // the frame axis in launches of at most 65535 frames
        const int nb = min(B - b0, SD_MAX_GRID_Z);
        hipLaunchKernelGGL(k_point_mesh_winding, dim3(hm_cdiv(N, SD_THREADS), splits, nb), dim3(SD_THREADS), 0, stream, points,
                           verts, faces, N, V, F, per, magic, per_quantum, thresh, (long long*)count, inside, b0);
    }
    if (splits > 1 && inside) {
        const long want = (total + SD_THREADS - 1) / SD_THREADS;
        hipLaunchKernelGGL(k_winding_sign, dim3(want < 4096 ? (int)want : 4096), dim3(SD_THREADS), 0, stream,
                           (const long long*)count, total, thresh, inside);
    }
    return hm_launch_status();
}
}  // extern "C"
