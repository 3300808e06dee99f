// solidvox.hip -- solid voxelisation of closed meshes on one world-anchored lattice, overlap counts of two voxelisations and
// the exact volume of a mesh: the hand-object intersection volume of the ObMan protocol (homan_amd/pointmetrics.py
// get_volume_metrics).  Beyond the reference; the definitions are in include/homan_amd.h and DESIGN.md section 7, pinned by
// the fp32 NumPy restatement of tests/volmetrics_ref.py (occupancy bit for bit).
//
//   k_solid_marks   one thread per triangle, as k_sdf_tris (sdf.hip): the triangle visits only the (y,z) voxel rows whose
//                   centre lies in its closed (y,z) box, casts the row's +x ray with the shared crossing rule
//                   (inside_test.h) and, per crossing, toggles ONE mark bit: that of the last voxel of the row whose centre
//                   lies in front of the hit.  Integer XOR: order-independent, hence deterministic.
//   k_solid_scan    one thread per row: occupancy = suffix XOR of the marks (voxel i is inside iff an odd number of marks
//                   sit at or after it): shift-XOR ladder within a word, parity carried from the higher words of the row.
//   k_voxel_overlap one workgroup per frame: popcounts of (a & b), a, b; a may be the OR of several arrays (two hands).
//   k_mesh_volume   one workgroup per frame: signed tetrahedra against the frame's vertex 0, in double, fixed order.
// The two passes of the voxeliser are separate launches: no workgroup waits for another inside a kernel.
#include "hm_common.h"
#include "inside_test.h"     // orient2, ray_x_crosses

#define SV_THREADS 256
#define SV_MAX_GRID_Y 65535
#define SV_MAX_INDEX (1 << 22)      // beyond it (i + 0.5) * h is no longer a clean fp32 lattice
#define SV_SCAN_MAX_BLOCKS 4096

__device__ __forceinline__ float sv_centre(int i, float h) { return ((float)i + 0.5f) * h; }

// x / h - 0.5 rounded down (up) and moved one index outwards, kept inside [lo_i - 1, hi_i + 1] before the conversion: the
// fp32 centre of an index differs from (i + 0.5) h by less than a quarter of a pitch for |i| <= 2^22, so the one index of
// slack covers it; the exact test against the centre itself follows at the caller.
__device__ __forceinline__ int sv_index_guess(float x, double h, double outwards, int lo_i, int hi_i)
{
    const double q = (double)x / h - 0.5;
    const double g = (outwards < 0.0 ? floor(q) : ceil(q)) + outwards;
    return (int)fmin(fmax(g, (double)(lo_i - 1)), (double)(hi_i + 1));
}

// grid (ceil(F/256), frames of this launch); frame = b0 + blockIdx.y.  words must be zero on entry.
__global__ __launch_bounds__(SV_THREADS) void k_solid_marks(const float* __restrict__ verts, const int* __restrict__ faces,
                                                             int V, int F, float h, const int* __restrict__ boxes, int NWX,
                                                             int NY, int NZ, unsigned int* __restrict__ words, int b0)
{
    const long b = (long)b0 + blockIdx.y;
    const int fi = blockIdx.x * SV_THREADS + threadIdx.x;
    if (fi >= F) return;
    const int* bx = boxes + b * 6;
    const int i0 = bx[0], j0 = bx[1], k0 = bx[2], nx = bx[3], ny = bx[4], nz = bx[5];
    if (nx <= 0 || ny <= 0 || nz <= 0) return;
    const int* t = faces + 3 * fi;
    if ((unsigned)t[0] >= (unsigned)V || (unsigned)t[1] >= (unsigned)V || (unsigned)t[2] >= (unsigned)V) return;
    const float* v = verts + b * V * 3;
    float p[9];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float* src = v + 3 * t[q];
        p[3 * q] = src[0]; p[3 * q + 1] = src[1]; p[3 * q + 2] = src[2];
    }
    const float lo_y = fminf(p[1], fminf(p[4], p[7])), hi_y = fmaxf(p[1], fmaxf(p[4], p[7]));
    const float lo_z = fminf(p[2], fminf(p[5], p[8])), hi_z = fmaxf(p[2], fmaxf(p[5], p[8]));
    const double hd = (double)h;
    const int ja = max(j0, sv_index_guess(lo_y, hd, -1.0, j0, j0 + ny - 1));
    const int jb = min(j0 + ny - 1, sv_index_guess(hi_y, hd, 1.0, j0, j0 + ny - 1));
    const int ka = max(k0, sv_index_guess(lo_z, hd, -1.0, k0, k0 + nz - 1));
    const int kb = min(k0 + nz - 1, sv_index_guess(hi_z, hd, 1.0, k0, k0 + nz - 1));
    unsigned int* frame = words + b * NZ * NY * NWX;
    for (int kz = ka; kz <= kb; ++kz) {
        const float cz = sv_centre(kz, h);
        if (cz < lo_z || cz > hi_z) continue;
        for (int jy = ja; jy <= jb; ++jy) {
            const float cy = sv_centre(jy, h);
            // exact reject on the closed (y,z) box of the triangle, as k_sdf_tris applies it
            if (cy < lo_y || cy > hi_y) continue;
            float xh;
            if (!ray_x_crosses(cy, cz, p, p + 3, p + 6, &xh)) continue;
            // m = number of voxels i0 .. i0 + nx - 1 of the row with xh > centre (centres increase with the index): a guess
            // by division, corrected against the centres themselves, so that the strict > holds exactly (NaN: m = 0)
            const double g = floor((double)xh / hd - 0.5) + 1.0 - (double)i0;
            int m = (int)fmin(fmax(g, 0.0), (double)nx);
            while (m > 0 && !(xh > sv_centre(i0 + m - 1, h))) --m;
            while (m < nx && xh > sv_centre(i0 + m, h)) ++m;
            if (m > 0)
                atomicXor(&frame[((long)(kz - k0) * NY + (jy - j0)) * NWX + ((m - 1) >> 5)], 1u << ((m - 1) & 31));
        }
    }
}

// grid-stride over the rows of every frame.  Marks sit below the frame's nx only, so every bit past it stays 0.
__global__ __launch_bounds__(SV_THREADS) void k_solid_scan(unsigned int* __restrict__ words, long rows, int NWX)
{
    for (long r = (long)blockIdx.x * SV_THREADS + threadIdx.x; r < rows; r += (long)gridDim.x * SV_THREADS) {
        unsigned int* row = words + r * NWX;
        unsigned int carry = 0u;                    // all ones when the marks of the higher words are odd in number
        for (int w = NWX - 1; w >= 0; --w) {
            unsigned int x = row[w];
            if (!(x | carry)) continue;
            x ^= x >> 1; x ^= x >> 2; x ^= x >> 4; x ^= x >> 8; x ^= x >> 16;
            x ^= carry;
            row[w] = x;
            carry = (x & 1u) ? 0xffffffffu : 0u;
        }
    }
}

// grid (B).  a (sets, B, W), b (B, W) -> counts (B,3) {popcount((a_0 | a_1 | ...) & b), popcount(a_0 | ...), popcount(b)}
__global__ __launch_bounds__(SV_THREADS) void k_voxel_overlap(const unsigned int* __restrict__ a, int sets,
                                                               const unsigned int* __restrict__ bw, long B, long W,
                                                               unsigned long long* __restrict__ counts)
{
    __shared__ unsigned long long s[3][SV_THREADS];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    unsigned long long c[3] = {0ull, 0ull, 0ull};
    for (long i = t; i < W; i += SV_THREADS) {
        unsigned int ua = 0u;
        for (int k = 0; k < sets; ++k) ua |= a[((long)k * B + b) * W + i];
        const unsigned int ub = bw[b * W + i];
        c[0] += (unsigned)__popc(ua & ub);
        c[1] += (unsigned)__popc(ua);
        c[2] += (unsigned)__popc(ub);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k][t] = c[k];
    __syncthreads();
    for (int w = SV_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k][t] += s[k][t + w];
        }
        __syncthreads();
    }
    if (t < 3) counts[b * 3 + t] = s[t][0];
}

// grid (B).  Thread t sums the faces t, t + 256, ... in that order; the 256 sums are folded by a halving tree (t += t + w,
// w = 128, 64, ... 1): one fixed order, whatever the batch.  A face that names a vertex outside [0, V) counts nothing.
__global__ __launch_bounds__(SV_THREADS) void k_mesh_volume(const float* __restrict__ verts, const int* __restrict__ faces,
                                                             int V, int F, double* __restrict__ out)
{
    __shared__ double s[SV_THREADS];
    const long b = blockIdx.x;
    const int t = threadIdx.x;
    const float* v = verts + b * V * 3;
    const double r[3] = {(double)v[0], (double)v[1], (double)v[2]};
    double acc = 0.0;
    for (int f = t; f < F; f += SV_THREADS) {
        const int* tr = faces + 3 * f;
        if ((unsigned)tr[0] >= (unsigned)V || (unsigned)tr[1] >= (unsigned)V || (unsigned)tr[2] >= (unsigned)V) continue;
        double e[3][3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) e[q][c] = (double)v[3 * tr[q] + c] - r[c];
        acc += (e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]))
               + e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
    }
    s[t] = acc;
    __syncthreads();
    for (int w = SV_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    if (t == 0) out[b] = fabs(s[0]) / 6.0;
}

extern "C" {
int hm_mesh_volume(const float* verts, const int* faces, int B, int V, int F, double* out, hipStream_t stream)
{
    HM_CHECK_ARG(verts && faces && out && B > 0 && V > 0 && F > 0);
    hipLaunchKernelGGL(k_mesh_volume, dim3(B), dim3(SV_THREADS), 0, stream, verts, faces, V, F, out);
    return hm_launch_status();
}

int hm_solid_voxels(const float* verts, const int* faces, int B, int V, int F, float pitch, const int* boxes, int NWX, int NY,
                    int NZ, int* boxes_dev, void* words, hipStream_t stream)
{
    HM_CHECK_ARG(verts && faces && boxes && boxes_dev && B > 0 && V > 0 && F > 0);
    HM_CHECK_ARG(pitch > 0.0f && pitch <= 3.4028234e38f);          // (a NaN fails the first comparison)
    HM_CHECK_ARG(NWX >= 0 && NY >= 0 && NZ >= 0);
    HM_CHECK_ARG(HM_ALIGNED(words, 4));              // the void pointer: 32-bit words (atomic targets)
    for (long b = 0; b < B; ++b) {
        const int* bx = boxes + b * 6;
        HM_CHECK_ARG(bx[3] >= 0 && bx[4] >= 0 && bx[5] >= 0);
        HM_CHECK_ARG((long)bx[3] <= 32L * NWX && bx[4] <= NY && bx[5] <= NZ);
        for (int c = 0; c < 3; ++c)
            HM_CHECK_ARG(bx[c] >= -SV_MAX_INDEX && (long)bx[c] + bx[3 + c] <= SV_MAX_INDEX);
    }
    const size_t rows = (size_t)B * (size_t)NZ * (size_t)NY, total = rows * (size_t)NWX;
    if (total == 0) return HM_OK;                                   // nothing to clear, nothing to mark
    HM_CHECK_ARG(words);
    // the kernel reads the boxes that were checked: this call's own copy, ordered on the stream before the launches
    if (hipMemcpyAsync(boxes_dev, boxes, (size_t)B * 6 * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess)
        return HM_ERR_LAUNCH;
    if (hipMemsetAsync(words, 0, total * sizeof(unsigned int), stream) != hipSuccess) return HM_ERR_LAUNCH;
    for (int b0 = 0; b0 < B; b0 += SV_MAX_GRID_Y) {                 // the frame axis in launches of at most 65535 frames
        const int nb = min(B - b0, SV_MAX_GRID_Y);
        hipLaunchKernelGGL(k_solid_marks, dim3(hm_cdiv(F, SV_THREADS), nb), dim3(SV_THREADS), 0, stream, verts, faces, V, F,
                           pitch, boxes_dev, NWX, NY, NZ, (unsigned int*)words, b0);
    }
    const long blocks = ((long)rows + SV_THREADS - 1) / SV_THREADS;
    hipLaunchKernelGGL(k_solid_scan, dim3((unsigned)(blocks < SV_SCAN_MAX_BLOCKS ? blocks : SV_SCAN_MAX_BLOCKS)),
                       dim3(SV_THREADS), 0, stream, (unsigned int*)words, (long)rows, NWX);
    return hm_launch_status();
}

int hm_voxel_overlap(const void* a, int a_sets, const void* b, int B, long words_per_frame, void* counts, hipStream_t stream)
{
    HM_CHECK_ARG(counts && a_sets > 0 && B > 0 && words_per_frame >= 0 && (words_per_frame == 0 || (a && b)));
    HM_CHECK_ARG(HM_ALIGNED(counts, 8) && HM_ALIGNED(a, 4) && HM_ALIGNED(b, 4));      // the void pointers: 64-bit counts, 32-bit words
    hipLaunchKernelGGL(k_voxel_overlap, dim3(B), dim3(SV_THREADS), 0, stream, (const unsigned int*)a, a_sets,
                       (const unsigned int*)b, (long)B, words_per_frame, (unsigned long long*)counts);
    return hm_launch_status();
}
}  // extern "C"
