// surfdist.hip -- exact point-to-mesh distance with the inside-outside sign: the kernel behind the surface metrics of
// homan_amd/pointmetrics.py get_surface_metrics (penetration depth to the SURFACE, contact by a distance threshold).  Beyond
// the reference; the rules are in include/homan_amd.h and DESIGN.md section 7, pinned bit for bit by the fp32 NumPy restatement
// of tests/surfmetrics_ref.py: every operation is fp32 IEEE without contraction, in the order written here.
//
//   k_point_mesh        grid (ceil(N/256), splits, frames of this launch).  A lane owns a point; the 256 threads stage the
//                       workgroup's faces through LDS 256 at a time as records (a, b, c, ab, ac, kind), one record per thread,
//                       and every lane then walks the same record (LDS broadcast reads): Ericson's region walk or the three
//                       segments of a degenerate face for the distance, ray_x_crosses (inside_test.h) for the sign.  A lane
//                       keeps (best D, lowest face) under a strict <, faces ascending, and the parity of its crossings.
//   splits == 1         the lane writes its outputs itself.
//   splits > 1          the faces of a frame are dealt to `splits` workgroups in contiguous runs of whole chunks (small
//                       batches would otherwise leave most of the chip idle); the lanes merge through integers only: an
//                       unsigned 64-bit atomicMin on (bits(D) << 32) | face - D >= 0, so its bits are monotone, and the low
//                       word breaks ties towards the lowest face - and an atomicXor of the parity.  k_point_mesh_init sets the
//                       merge words before, k_point_mesh_finish unpacks them after; both are ordered on the stream.
// The closest point is recomputed from the winning face by the same function that gave D: the same bits on either path.
// The minimum and the parity do not depend on the order of the faces, so a frame's values depend neither on the split nor on
// the batch.  No floating-point atomics.
#include "hm_common.h"
#include "inside_test.h"     // orient2, ray_x_crosses
#include "surfdist_walk.h"   // SdFace, sd_load_face, sd_closest: the per-face walk, shared with csrc/surfcontact.hip; SD_*, sd_splits

#define SD_EMPTY 0x7f800000ffffffffull   // (bits(+inf) << 32) | (unsigned)-1: no face yet

// the outputs of point `at` (= b * N + i) from its merged values; face < 0: no face counted
__device__ __forceinline__ void sd_write(const float* __restrict__ points, const float* __restrict__ vb,
                                         const int* __restrict__ faces, int V, long at, float best, int face, int parity,
                                         float* __restrict__ d2, int* __restrict__ face_idx, int* __restrict__ inside,
                                         float* __restrict__ closest)
{
    if (d2) d2[at] = best;
    if (face_idx) face_idx[at] = face;
    if (inside) inside[at] = parity;
    if (closest) {
        float q[3] = {0.f, 0.f, 0.f};
        if (face >= 0) {
            const float p[3] = {points[3 * at], points[3 * at + 1], points[3 * at + 2]};
            SdFace r;
            sd_load_face(vb, faces, face, V, r);
            sd_closest(p, r, q);
        }
        closest[3 * at] = q[0]; closest[3 * at + 1] = q[1]; closest[3 * at + 2] = q[2];
    }
}

__global__ __launch_bounds__(SD_THREADS) void k_point_mesh(const float* __restrict__ points, const float* __restrict__ verts,
                                                            const int* __restrict__ faces, int N, int V, int F,
                                                            int chunks_per_split, float* __restrict__ d2,
                                                            int* __restrict__ face_idx, int* __restrict__ inside,
                                                            float* __restrict__ closest, unsigned long long* __restrict__ ws_min,
                                                            unsigned int* __restrict__ ws_par, int b0)
{
    __shared__ __attribute__((aligned(16))) SdFace s_face[SD_CHUNK];
    const long b = (long)b0 + blockIdx.z;
    const int i = blockIdx.x * SD_THREADS + threadIdx.x;
    const float* vb = verts + b * V * 3;
    const long at = b * N + i;
    float p[3] = {0.f, 0.f, 0.f};
    bool live = i < N;
    if (live) {
        p[0] = points[3 * at]; p[1] = points[3 * at + 1]; p[2] = points[3 * at + 2];
    }
    const bool ok = live && sd_finite(p[0]) && sd_finite(p[1]) && sd_finite(p[2]);
    float best = __builtin_inff();
    int besti = -1, parity = 0;
    const long f_begin = (long)blockIdx.y * chunks_per_split * SD_CHUNK;
    const long f_stop = f_begin + (long)chunks_per_split * SD_CHUNK, f_end = f_stop < F ? f_stop : (long)F;
    for (long f0 = f_begin; f0 < f_end; f0 += SD_CHUNK) {
        const int n = f_end - f0 < SD_CHUNK ? (int)(f_end - f0) : SD_CHUNK;
        __syncthreads();                                           // the previous chunk has been walked by every wave
        if ((int)threadIdx.x < n) sd_load_face(vb, faces, f0 + threadIdx.x, V, s_face[threadIdx.x]);
        __syncthreads();
        if (!ok) continue;
        for (int k = 0; k < n; ++k) {
            const SdFace r = s_face[k];
            if (r.kind == SD_SKIPPED) continue;                    // (the same for every lane)
            float q[3];
            const float D = sd_closest(p, r, q);
            if (D < best) { best = D; besti = (int)(f0 + k); }
            float xhit;
            if (ray_x_crosses(p[1], p[2], r.a, r.b, r.c, &xhit) && xhit > p[0]) parity ^= 1;
        }
    }
    if (gridDim.y == 1) {
        if (live) sd_write(points, vb, faces, V, at, best, besti, parity, d2, face_idx, inside, closest);
        return;
    }
    if (besti >= 0)
        atomicMin(&ws_min[at], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned int)besti);
    if (parity) atomicXor(&ws_par[at], 1u);
}

__global__ __launch_bounds__(SD_THREADS) void k_point_mesh_init(unsigned long long* __restrict__ ws_min,
                                                                 unsigned int* __restrict__ ws_par, long total)
{
    for (long t = (long)blockIdx.x * SD_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * SD_THREADS) {
        ws_min[t] = SD_EMPTY;
        ws_par[t] = 0u;
    }
}

__global__ __launch_bounds__(SD_THREADS) void k_point_mesh_finish(const float* __restrict__ points,
                                                                   const float* __restrict__ verts,
                                                                   const int* __restrict__ faces, int N, int V,
                                                                   const unsigned long long* __restrict__ ws_min,
                                                                   const unsigned int* __restrict__ ws_par, long total,
                                                                   float* __restrict__ d2, int* __restrict__ face_idx,
                                                                   int* __restrict__ inside, float* __restrict__ closest)
{
    for (long t = (long)blockIdx.x * SD_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * SD_THREADS) {
        const unsigned long long m = ws_min[t];
        const long b = t / N;
        sd_write(points, verts + b * V * 3, faces, V, t, __uint_as_float((unsigned int)(m >> 32)), (int)(unsigned int)m,
                 (int)(ws_par[t] & 1u), d2, face_idx, inside, closest);
    }
}

extern "C" {
size_t hm_point_mesh_workspace_bytes(int B, int N, int F)
{
    if (B <= 0 || N <= 0 || F <= 0) return 0;
    int per;
    if (sd_splits(B, N, F, &per) == 1) return 0;
    return (size_t)B * (size_t)N * (sizeof(unsigned long long) + sizeof(unsigned int));
}

int hm_point_mesh_distance(const float* points, const float* verts, const int* faces, int B, int N, int V, int F, float* d2,
                           int* face_idx, int* inside, float* closest, void* workspace, hipStream_t stream)
{
    HM_CHECK_ARG(points && verts && faces && B > 0 && N > 0 && V > 0 && F > 0);
    HM_CHECK_ARG(d2 || face_idx || inside || closest);
    int per;
    const int splits = sd_splits(B, N, F, &per);
    HM_CHECK_ARG(splits == 1 || workspace);
    HM_CHECK_ARG(HM_ALIGNED(workspace, 8));          // 64-bit (distance, face) words, the targets of atomicMin, at its base
    const long total = (long)B * N;                 // every index of the kernels is a 64-bit product of the int sizes
    unsigned long long* ws_min = (unsigned long long*)workspace;
    unsigned int* ws_par = splits > 1 ? (unsigned int*)(ws_min + total) : nullptr;
    const long aux_want = (total + SD_THREADS - 1) / SD_THREADS;
    const int aux_blocks = aux_want < 4096 ? (int)aux_want : 4096;
    if (splits > 1)
        hipLaunchKernelGGL(k_point_mesh_init, dim3(aux_blocks), dim3(SD_THREADS), 0, stream, ws_min, ws_par, total);
    for (int b0 = 0; b0 < B; b0 += SD_MAX_GRID_Z) {     // the frame axis in launches of at most 65535 frames
        const int nb = min(B - b0, SD_MAX_GRID_Z);
        hipLaunchKernelGGL(k_point_mesh, dim3(hm_cdiv(N, SD_THREADS), splits, nb), dim3(SD_THREADS), 0, stream, points, verts,
                           faces, N, V, F, per, d2, face_idx, inside, closest, ws_min, ws_par, b0);
    }
    if (splits > 1)
        hipLaunchKernelGGL(k_point_mesh_finish, dim3(aux_blocks), dim3(SD_THREADS), 0, stream, points, verts, faces, N, V,
                           (const unsigned long long*)ws_min, (const unsigned int*)ws_par, total, d2, face_idx, inside, closest);
    return hm_launch_status();
}
}  // extern "C"
