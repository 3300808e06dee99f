// remesh.hip -- mesh preparation: a closed, oriented triangle mesh off a lattice of inside-outside signs (surface nets), behind
// ops.lattice_signs / ops.surface_nets and homan_amd/meshprep.py (make_watertight, simplify_mesh).  Stands in for the reference's
// external ManifoldPlus + ACVD stage (meshprocess/simplifymesh.py); the rules are in include/homan_amd.h and DESIGN.md section 7,
// pinned bit for bit by the NumPy restatement of tests/meshprep_ref.py.  The topology is integer work on a packed bit field; the
// only floating point is the corner and vertex positions, fp32 IEEE without contraction.
//
// The field: corner (i, j, k) of an (nx, ny, nz) lattice is bit (i & 63) of word i >> 6 of row k * ny + j; a row is W =
// ceil(nx / 64) 64-bit words, bits at and beyond nx are 0, and so is the outermost corner layer.  With those zeros no kernel
// needs a mask along x: a shifted word (bit i + 1 brought to position i) reads 0 where the lattice ends.
//
//   k_lattice_corners   a thread per corner: origin + (float)index * h.
//   k_lattice_pack      a wave per (row, word): one __ballot of "flag set and not on the outer layer" is the word.
//   k_repair_pass       a thread per word, Jacobi: new = old | marks(old), where marks are the four corners of every unit face
//                       whose corners are a checkerboard.  Reads one buffer, writes the other; pass p returns at once when pass
//                       p - 1 changed nothing (both buffers are then equal).  The only atomics: one integer atomicAdd per word
//                       that changed, into the pass's counter.
//   k_repair_report     one thread folds the 65 counters into {passes, corners, status}.
//   k_nets_count        a thread per row: popcounts of the active cells and of the sign-changing x-, y-, z-edges that the row
//                       bases, and the words of the active-cell field.
//   k_nets_scan         one workgroup per count array: exclusive scan over the rows in tiles of 2048 with a running carry.
//   k_nets_vertices     a wave per (row, word) of the cell field: index = row offset + popcount below; the position.
//   k_nets_faces        a wave per (row, word) and axis: two triangles per sign-changing edge at 2 * (axis base + row offset +
//                       popcount below), naming the four cells around the edge through the same offsets.
//   k_lattice_snap      a thread per vertex: the closest surface point where it is within the limit, else the lattice position.
// Every hand-off between kernels is a kernel boundary on the stream; no workgroup waits for another; nothing is allocated.
#include "hm_common.h"

#define RM_THREADS 256
#define RM_WAVES (RM_THREADS / HM_WAVE)
#define RM_MAX_PASSES 64                 // passes that may change something; pass 65 only detects
#define RM_REPORT_PASS0 8                // report[8 + p]: corners set by pass p
#define RM_REPORT_INTS (RM_REPORT_PASS0 + RM_MAX_PASSES + 1)
#define RM_SCAN_ITEMS 8
#define RM_SCAN_TILE (RM_THREADS * RM_SCAN_ITEMS)
#define RM_MAX_AXIS 512                  // 6 * 512^3 triangles at the most: every count and index fits an int

typedef unsigned long long rm_word;

static inline int rm_words(int nx) { return (nx + 63) >> 6; }

// word w of row (j, k); 0 outside the lattice
__device__ __forceinline__ rm_word rm_load(const rm_word* __restrict__ f, int j, int k, int w, int ny, int nz, int W)
{
    if (j < 0 || j >= ny || k < 0 || k >= nz || w < 0 || w >= W) return 0;
    return f[((long)k * ny + j) * W + w];
}
// bit i + 1 at position i
__device__ __forceinline__ rm_word rm_up(rm_word x, rm_word next) { return (x >> 1) | (next << 63); }
// s00 == s11 != s10 == s01 for the faces spanned by bits (i, i + 1) of two rows
__device__ __forceinline__ rm_word rm_checker(rm_word p, rm_word p1, rm_word q, rm_word q1) { return ~(p ^ q1) & ~(p1 ^ q) & (p ^ p1); }

__global__ __launch_bounds__(RM_THREADS) void k_lattice_corners(int nx, int ny, long total, float ox, float oy, float oz, float h,
                                                                 float* __restrict__ out)
{
    const long t = (long)blockIdx.x * RM_THREADS + threadIdx.x;
    if (t >= total) return;
    const int i = (int)(t % nx), j = (int)((t / nx) % ny), k = (int)(t / ((long)nx * ny));
    out[3 * t] = ox + (float)i * h;
    out[3 * t + 1] = oy + (float)j * h;
    out[3 * t + 2] = oz + (float)k * h;
}

__global__ __launch_bounds__(RM_THREADS) void k_lattice_pack(const int* __restrict__ flags, int nx, int ny, int nz, int W,
                                                              rm_word* __restrict__ bits)
{
    const long g = (long)blockIdx.x * RM_WAVES + (threadIdx.x >> 6);       // (the same for the whole wave)
    if (g >= (long)ny * nz * W) return;
    const long row = g / W;
    const int w = (int)(g % W), j = (int)(row % ny), k = (int)(row / ny), i = w * 64 + (threadIdx.x & 63);
    const bool interior = i > 0 && i < nx - 1 && j > 0 && j < ny - 1 && k > 0 && k < nz - 1;
    const bool set = interior && flags[row * nx + i] != 0;
    const rm_word word = __ballot(set);
    if ((threadIdx.x & 63) == 0) bits[g] = word;
}

__global__ __launch_bounds__(RM_THREADS) void k_repair_pass(const rm_word* __restrict__ src, rm_word* __restrict__ dst, int ny,
                                                             int nz, int W, int* __restrict__ changed, int p)
{
    if (p > 0 && changed[p - 1] == 0) return;                              // settled: src == dst already
    const long t = (long)blockIdx.x * RM_THREADS + threadIdx.x;
    if (t >= (long)ny * nz * W) return;
    const long row = t / W;
    const int w = (int)(t % W), j = (int)(row % ny), k = (int)(row / ny);
    const rm_word a = src[t], al = rm_load(src, j, k, w - 1, ny, nz, W), ah = rm_load(src, j, k, w + 1, ny, nz, W);
    const rm_word a1 = rm_up(a, ah), al1 = rm_up(al, a);
    rm_word marks = 0;
    const int dj[4] = {-1, 1, 0, 0}, dk[4] = {0, 0, -1, 1};
#pragma unroll
    for (int n = 0; n < 4; ++n) {                                          // faces in the planes that hold the x axis
        const int jj = j + dj[n], kk = k + dk[n];
        const rm_word b = rm_load(src, jj, kk, w, ny, nz, W), bl = rm_load(src, jj, kk, w - 1, ny, nz, W);
        const rm_word bh = rm_load(src, jj, kk, w + 1, ny, nz, W);
        const rm_word m = rm_checker(a, a1, b, rm_up(b, bh)), ml = rm_checker(al, al1, bl, rm_up(bl, b));
        marks |= m | (m << 1) | (ml >> 63);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {                                          // faces across the x axis: the same bit of four rows
        const int sj = (n & 1) ? 1 : -1, sk = (n & 2) ? 1 : -1;
        const rm_word b = rm_load(src, j + sj, k, w, ny, nz, W), c = rm_load(src, j, k + sk, w, ny, nz, W);
        const rm_word d = rm_load(src, j + sj, k + sk, w, ny, nz, W);
        marks |= ~(a ^ d) & ~(b ^ c) & (a ^ b);
    }
    const rm_word now = a | marks;
    dst[t] = now;
    const int c = __popcll(now & ~a);
    if (c) atomicAdd(&changed[p], c);
}

__global__ void k_repair_report(int* __restrict__ report)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int passes = 0, corners = 0;
    for (int p = 0; p <= RM_MAX_PASSES; ++p) {
        const int c = report[RM_REPORT_PASS0 + p];
        passes += c != 0;
        corners += c;
    }
    report[0] = passes;
    report[1] = corners;
    report[2] = report[RM_REPORT_PASS0 + RM_MAX_PASSES] != 0;             // still changing in pass 65
}

// the words of row (j, k) at w that the count and the faces are made of: active cells, and the edges the row bases per axis
struct RmRowWords { rm_word cells, ex, ey, ez, base, corner[2][2][2]; };      // corner[dx][dy][dz]: bit i is corner (i + dx, j + dy, k + dz)
__device__ __forceinline__ RmRowWords rm_row_words(const rm_word* __restrict__ f, int j, int k, int w, int ny, int nz, int W)
{
    const rm_word r00 = rm_load(f, j, k, w, ny, nz, W), r10 = rm_load(f, j + 1, k, w, ny, nz, W);
    const rm_word r01 = rm_load(f, j, k + 1, w, ny, nz, W), r11 = rm_load(f, j + 1, k + 1, w, ny, nz, W);
    const rm_word s00 = rm_up(r00, rm_load(f, j, k, w + 1, ny, nz, W)), s10 = rm_up(r10, rm_load(f, j + 1, k, w + 1, ny, nz, W));
    const rm_word s01 = rm_up(r01, rm_load(f, j, k + 1, w + 1, ny, nz, W));
    const rm_word s11 = rm_up(r11, rm_load(f, j + 1, k + 1, w + 1, ny, nz, W));
    RmRowWords o;
    const rm_word any = r00 | r10 | r01 | r11 | s00 | s10 | s01 | s11, all = r00 & r10 & r01 & r11 & s00 & s10 & s01 & s11;
    o.cells = (j < ny - 1 && k < nz - 1) ? any & ~all : 0;
    o.ex = r00 ^ s00;
    o.ey = j < ny - 1 ? r00 ^ r10 : 0;
    o.ez = k < nz - 1 ? r00 ^ r01 : 0;
    o.base = r00;
    o.corner[0][0][0] = r00; o.corner[0][1][0] = r10; o.corner[0][0][1] = r01; o.corner[0][1][1] = r11;
    o.corner[1][0][0] = s00; o.corner[1][1][0] = s10; o.corner[1][0][1] = s01; o.corner[1][1][1] = s11;
    return o;
}

__global__ __launch_bounds__(RM_THREADS) void k_nets_count(const rm_word* __restrict__ bits, int ny, int nz, int W,
                                                            rm_word* __restrict__ cell_bits, int* __restrict__ counts)
{
    const long row = (long)blockIdx.x * RM_THREADS + threadIdx.x, rows = (long)ny * nz;
    if (row >= rows) return;
    const int j = (int)(row % ny), k = (int)(row / ny);
    int n[4] = {0, 0, 0, 0};
    for (int w = 0; w < W; ++w) {
        const RmRowWords r = rm_row_words(bits, j, k, w, ny, nz, W);
        cell_bits[row * W + w] = r.cells;
        n[0] += __popcll(r.cells); n[1] += __popcll(r.ex); n[2] += __popcll(r.ey); n[3] += __popcll(r.ez);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) counts[a * rows + row] = n[a];
}

// in place: counts -> exclusive offsets; totals[array] = the sum.  One workgroup per array, tiles of RM_SCAN_TILE rows in order.
__global__ __launch_bounds__(RM_THREADS) void k_nets_scan(int* __restrict__ counts, long rows, int* __restrict__ totals)
{
    __shared__ int s_wave[RM_WAVES];
    int* v = counts + blockIdx.x * rows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (long base = 0; base < rows; base += RM_SCAN_TILE) {
        const long at = base + (long)threadIdx.x * RM_SCAN_ITEMS;
        int item[RM_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int q = 0; q < RM_SCAN_ITEMS; ++q) {
            item[q] = at + q < rows ? v[at + q] : 0;
            sum += item[q];
        }
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(incl, d);
            if (lane >= d) incl += u;
        }
        __syncthreads();                                                   // the previous tile's s_wave has been read
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, tile = 0;
#pragma unroll
        for (int u = 0; u < RM_WAVES; ++u) {
            before += u < wave ? s_wave[u] : 0;
            tile += s_wave[u];
        }
        int run = carry + before + (incl - sum);
#pragma unroll
        for (int q = 0; q < RM_SCAN_ITEMS; ++q) {
            if (at + q < rows) v[at + q] = run;
            run += item[q];
        }
        carry += tile;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// index of the active cell (ci, cj, ck): its rank in row-major order, i fastest
__device__ __forceinline__ int rm_cell_index(const rm_word* __restrict__ cell_bits, const int* __restrict__ cell_off, int ci, int cj,
                                             int ck, int ny, int W)
{
    const long row = (long)ck * ny + cj;
    const rm_word* r = cell_bits + row * W;
    int at = cell_off[row];
    for (int w = 0; w < (ci >> 6); ++w) at += __popcll(r[w]);
    return at + __popcll(r[ci >> 6] & (((rm_word)1 << (ci & 63)) - 1));
}

__global__ __launch_bounds__(RM_THREADS) void k_nets_vertices(const rm_word* __restrict__ bits, const rm_word* __restrict__ cell_bits,
                                                               const int* __restrict__ cell_off, int ny, int nz, int W, float ox,
                                                               float oy, float oz, float half_h, int max_vertices,
                                                               float* __restrict__ vertices)
{
    const long g = (long)blockIdx.x * RM_WAVES + (threadIdx.x >> 6);
    if (g >= (long)ny * nz * W) return;
    const rm_word act = cell_bits[g];
    if (act == 0) return;
    const long row = g / W;
    const int w = (int)(g % W), cj = (int)(row % ny), ck = (int)(row / ny), lane = threadIdx.x & 63, ci = w * 64 + lane;
    if (!((act >> lane) & 1)) return;
    int at = cell_off[row];
    for (int u = 0; u < w; ++u) at += __popcll(cell_bits[row * W + u]);
    at += __popcll(act & (((rm_word)1 << lane) - 1));
    if (at >= max_vertices) return;
    const RmRowWords here = rm_row_words(bits, cj, ck, w, ny, nz, W);
    int c[2][2][2];                                                        // [dx][dy][dz]
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dz = 0; dz < 2; ++dz) c[dx][dy][dz] = (int)((here.corner[dx][dy][dz] >> lane) & 1);
    int sx = 0, sy = 0, sz = 0, n = 0;                                     // midpoints of the sign-changing edges, in half cells
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (c[0][u][v] != c[1][u][v]) { sx += 2 * ci + 1; sy += 2 * (cj + u); sz += 2 * (ck + v); ++n; }
            if (c[u][0][v] != c[u][1][v]) { sx += 2 * (ci + u); sy += 2 * cj + 1; sz += 2 * (ck + v); ++n; }
            if (c[u][v][0] != c[u][v][1]) { sx += 2 * (ci + u); sy += 2 * (cj + v); sz += 2 * ck + 1; ++n; }
        }
    const float fn = (float)n;
    vertices[3 * (long)at] = ox + ((float)sx / fn) * half_h;
    vertices[3 * (long)at + 1] = oy + ((float)sy / fn) * half_h;
    vertices[3 * (long)at + 2] = oz + ((float)sz / fn) * half_h;
}

__global__ __launch_bounds__(RM_THREADS) void k_nets_faces(const rm_word* __restrict__ bits, const rm_word* __restrict__ cell_bits,
                                                            const int* __restrict__ offsets, const int* __restrict__ totals, int nx,
                                                            int ny, int nz, int W, int max_triangles, int* __restrict__ triangles)
{
    const long g = (long)blockIdx.x * RM_WAVES + (threadIdx.x >> 6), rows = (long)ny * nz;
    if (g >= rows * W) return;
    const int axis = blockIdx.y;
    const long row = g / W;
    const int w = (int)(g % W), j = (int)(row % ny), k = (int)(row / ny), lane = threadIdx.x & 63, i = w * 64 + lane;
    const RmRowWords here = rm_row_words(bits, j, k, w, ny, nz, W);
    const rm_word e = axis == 0 ? here.ex : axis == 1 ? here.ey : here.ez;
    if (e == 0) return;
    if (!((e >> lane) & 1)) return;
    long at = offsets[(1 + axis) * rows + row];
    for (int a = 0; a < axis; ++a) at += totals[1 + a];                    // all x-edges, then the y-edges, then the z-edges
    for (int u = 0; u < w; ++u) {
        const RmRowWords r = rm_row_words(bits, j, k, u, ny, nz, W);
        at += __popcll(axis == 0 ? r.ex : axis == 1 ? r.ey : r.ez);
    }
    at += __popcll(e & (((rm_word)1 << lane) - 1));
    if (2 * at + 2 > (long)max_triangles) return;
    // the four cells around the edge: the base corner shifted by (-1,-1), (0,-1), (0,0), (-1,0) along axes (a+1)%3, (a+2)%3
    const int du[4] = {-1, 0, 0, -1}, dv[4] = {-1, -1, 0, 0};
    const int p[3] = {i, j, k}, hi[3] = {nx - 2, ny - 2, nz - 2};
    int cell[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int c[3] = {p[0], p[1], p[2]};
        c[(axis + 1) % 3] += du[q];
        c[(axis + 2) % 3] += dv[q];
        const bool ok = c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] <= hi[0] && c[1] <= hi[1] && c[2] <= hi[2];
        cell[q] = ok ? rm_cell_index(cell_bits, offsets, c[0], c[1], c[2], ny, W) : 0;     // (always ok: the outer layer is outside)
    }
    const bool inside = (here.base >> lane) & 1;                           // normals point from inside to outside
    const int c0 = inside ? cell[0] : cell[3], c1 = inside ? cell[1] : cell[2], c2 = inside ? cell[2] : cell[1];
    const int c3 = inside ? cell[3] : cell[0];
    int* t = triangles + 6 * at;
    t[0] = c0; t[1] = c1; t[2] = c2;
    t[3] = c0; t[4] = c2; t[5] = c3;
}

__global__ __launch_bounds__(RM_THREADS) void k_lattice_snap(const float* __restrict__ lattice, const float* __restrict__ closest,
                                                              const float* __restrict__ d2, long n, float limit2,
                                                              float* __restrict__ out, int* __restrict__ snapped)
{
    const long t = (long)blockIdx.x * RM_THREADS + threadIdx.x;
    if (t >= n) return;
    const bool take = d2[t] <= limit2;                                     // (false for a NaN)
    const float* from = take ? closest : lattice;
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * t + a] = from[3 * t + a];
    if (snapped) snapped[t] = take ? 1 : 0;
}

static inline bool rm_dims_ok(int nx, int ny, int nz)
{
    return nx >= 2 && ny >= 2 && nz >= 2 && nx <= RM_MAX_AXIS && ny <= RM_MAX_AXIS && nz <= RM_MAX_AXIS;
}
static inline bool rm_finite(float x) { return x - x == 0.f; }

extern "C" {
long hm_lattice_words(int nx, int ny, int nz)
{
    return rm_dims_ok(nx, ny, nz) ? (long)ny * nz * rm_words(nx) : -1;
}

int hm_lattice_corners(int nx, int ny, int nz, float ox, float oy, float oz, float h, float* points, hipStream_t stream)
{
    HM_CHECK_ARG(points && rm_dims_ok(nx, ny, nz));
    HM_CHECK_ARG(rm_finite(ox) && rm_finite(oy) && rm_finite(oz) && rm_finite(h) && h > 0.f);
    const long total = (long)nx * ny * nz;
    hipLaunchKernelGGL(k_lattice_corners, dim3(hm_cdiv(total, RM_THREADS)), dim3(RM_THREADS), 0, stream, nx, ny, total, ox, oy, oz,
                       h, points);
    return hm_launch_status();
}

int hm_lattice_repair(const int* flags, int nx, int ny, int nz, void* bits, int* report, hipStream_t stream)
{
    HM_CHECK_ARG(flags && bits && report && rm_dims_ok(nx, ny, nz));
    HM_CHECK_ARG(HM_ALIGNED(bits, 8));
    const int W = rm_words(nx);
    const long words = (long)ny * nz * W;
    rm_word* buf[2] = {(rm_word*)bits, (rm_word*)bits + words};
    if (hipMemsetAsync(report, 0, RM_REPORT_INTS * sizeof(int), stream) != hipSuccess) return HM_ERR_LAUNCH;
    hipLaunchKernelGGL(k_lattice_pack, dim3(hm_cdiv(words, RM_WAVES)), dim3(RM_THREADS), 0, stream, flags, nx, ny, nz, W, buf[0]);
    for (int p = 0; p <= RM_MAX_PASSES; ++p)
        hipLaunchKernelGGL(k_repair_pass, dim3(hm_cdiv(words, RM_THREADS)), dim3(RM_THREADS), 0, stream,
                           (const rm_word*)buf[p & 1], buf[(p + 1) & 1], ny, nz, W, report + RM_REPORT_PASS0, p);
    hipLaunchKernelGGL(k_repair_report, dim3(1), dim3(HM_WAVE), 0, stream, report);
    return hm_launch_status();
}

int hm_surface_nets_count(const void* bits, int nx, int ny, int nz, void* cell_bits, int* row_offsets, int* totals,
                          hipStream_t stream)
{
    HM_CHECK_ARG(bits && cell_bits && row_offsets && totals && rm_dims_ok(nx, ny, nz));
    HM_CHECK_ARG(HM_ALIGNED(bits, 8) && HM_ALIGNED(cell_bits, 8));
    const long rows = (long)ny * nz;
    hipLaunchKernelGGL(k_nets_count, dim3(hm_cdiv(rows, RM_THREADS)), dim3(RM_THREADS), 0, stream, (const rm_word*)bits, ny, nz,
                       rm_words(nx), (rm_word*)cell_bits, row_offsets);
    hipLaunchKernelGGL(k_nets_scan, dim3(4), dim3(RM_THREADS), 0, stream, row_offsets, rows, totals);
    return hm_launch_status();
}

int hm_surface_nets_emit(const void* bits, const void* cell_bits, const int* row_offsets, const int* totals, int nx, int ny, int nz,
                         float ox, float oy, float oz, float h, int max_vertices, int max_triangles, float* vertices,
                         int* triangles, hipStream_t stream)
{
    HM_CHECK_ARG(bits && cell_bits && row_offsets && totals && rm_dims_ok(nx, ny, nz));
    HM_CHECK_ARG(HM_ALIGNED(bits, 8) && HM_ALIGNED(cell_bits, 8));
    HM_CHECK_ARG(max_vertices >= 0 && max_triangles >= 0 && (vertices || max_vertices == 0) && (triangles || max_triangles == 0));
    HM_CHECK_ARG(rm_finite(ox) && rm_finite(oy) && rm_finite(oz) && rm_finite(h) && h > 0.f);
    const int W = rm_words(nx);
    const int blocks = hm_cdiv((long)ny * nz * W, RM_WAVES);
    const float half_h = 0.5f * h;
    if (max_vertices > 0)
        hipLaunchKernelGGL(k_nets_vertices, dim3(blocks), dim3(RM_THREADS), 0, stream, (const rm_word*)bits,
                           (const rm_word*)cell_bits, row_offsets, ny, nz, W, ox, oy, oz, half_h, max_vertices, vertices);
    if (max_triangles > 0)
        hipLaunchKernelGGL(k_nets_faces, dim3(blocks, 3), dim3(RM_THREADS), 0, stream, (const rm_word*)bits,
                           (const rm_word*)cell_bits, row_offsets, totals, nx, ny, nz, W, max_triangles, triangles);
    return hm_launch_status();
}

int hm_lattice_snap(const float* lattice, const float* closest, const float* d2, long n, float snap_limit, float h, float* out,
                    int* snapped, hipStream_t stream)
{
    HM_CHECK_ARG(lattice && closest && d2 && out && n >= 0);
    HM_CHECK_ARG(rm_finite(snap_limit) && snap_limit > 0.f && rm_finite(h) && h > 0.f);
    if (n == 0) return HM_OK;
    const float limit2 = (snap_limit * snap_limit) * (h * h);
    hipLaunchKernelGGL(k_lattice_snap, dim3(hm_cdiv(n, RM_THREADS)), dim3(RM_THREADS), 0, stream, lattice, closest, d2, n, limit2,
                       out, snapped);
    return hm_launch_status();
}
}  // extern "C"
