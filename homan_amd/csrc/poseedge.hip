// poseedge.hip -- the one-way edge-chamfer term of the object-pose initialisation (reference homan/pose_optimization.py:
// 74-88 and :136-150, the PHOSA term): max-pool edges of the render x the distance transform of the target's edge band.
//
//   hm_edge_edt         the distance-transform image of a target mask (:84-85: scipy distance_transform_edt of the complement
//                       of `maxpool_k(ref) - ref > 0`, to the power 2 * power), exact, on the device;
//   hm_pose_edge_terms  per candidate the masked L2 / IoU of :144-147, the chamfer sum of :148-149, their weighted total, and
//                       the per-sample gradient image of that total (what autograd forms through MaxPool2d's backward),
//                       ready for hm_sil_bwd mode 3.
//
// Every sum is formed in one fixed order and there is no floating-point atomic: two calls on the same input agree bit for bit.
#include "hm_common.h"

#define PE_THREADS 256
#define PE_R 3                              // largest window radius (kernel_size <= 7)
#define PE_TW 64                            // tile: 64 x 32 samples per workgroup
#define PE_TH 32
#define PE_IW (PE_TW + 4 * PE_R)            // image tile: the samples of every window that can name a sample of the tile
#define PE_IH (PE_TH + 4 * PE_R)
#define PE_WW (PE_TW + 2 * PE_R)            // window tile: the windows that can name a sample of the tile
#define PE_WH (PE_TH + 2 * PE_R)
#define PE_NONE 255                         // a window centred outside the image: names nobody
#define EDT_MAX_SIZE 2048
#define EDT_FAR 16384                       // "no band sample in this column": FAR^2 + EDT_MAX_SIZE^2 < 2^31

// ------------------------------------------------------------------------------------------------ distance transform
// Three launches over the (size, size) image, the output buffer doubling as the integer scratch:
//   k_edt_band  g = 0 on the edge band, EDT_FAR elsewhere; the number of band samples
//   k_edt_cols  g = distance, along the column, to the column's nearest band sample (two scans)
//   k_edt_rows  d2(y, x) = min_x' (x - x')^2 + g(y, x')^2 with the row's g^2 in LDS; out = d2 ^ power
// All integer: d2 is the exact squared Euclidean distance.
__global__ __launch_bounds__(PE_THREADS) void k_edt_band(const float* __restrict__ ref, int size, int stride, int r,
                                                          int* __restrict__ g, int* __restrict__ count)
{
    __shared__ float red[16];
    const int pix = blockIdx.x * PE_THREADS + threadIdx.x;
    float band = 0.f;
    if (pix < size * size) {
        const int y = pix / size, x = pix - y * size;
        const int y0 = max(y - r, 0), y1 = min(y + r, size - 1), x0 = max(x - r, 0), x1 = min(x + r, size - 1);
        const float own = ref[(long)y * stride + x];
        float top = own;
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) top = fmaxf(top, ref[(long)yy * stride + xx]);
        band = top - own > 0.f ? 1.f : 0.f;
        g[(long)y * stride + x] = band != 0.f ? 0 : EDT_FAR;
    }
    const float total = hm_block_sum(band, red);              // (<= 256 ones: exact)
    if (threadIdx.x == 0 && total > 0.f) atomicAdd(count, (int)total);
}

__global__ __launch_bounds__(PE_THREADS) void k_edt_cols(int size, int stride, int* __restrict__ g)
{
    const int x = blockIdx.x * PE_THREADS + threadIdx.x;
    if (x >= size) return;
    int d = EDT_FAR;
    for (int y = 0; y < size; ++y) {
        int* at = g + (long)y * stride + x;
        d = *at == 0 ? 0 : min(d + 1, EDT_FAR);
        *at = d;
    }
    d = EDT_FAR;
    for (int y = size - 1; y >= 0; --y) {
        int* at = g + (long)y * stride + x;
        const int down = *at;
        d = down == 0 ? 0 : min(d + 1, EDT_FAR);
        *at = min(down, d);
    }
}

__device__ __forceinline__ float edt_power(int d2, float power)
{
    const double v = (double)d2;
    if (power == 0.25f) return (float)sqrt(sqrt(v));           // (the reference's default: bit-equal to its numpy expression)
    if (power == 0.5f) return (float)sqrt(v);
    if (power == 1.f) return (float)v;
    return (float)pow(v, (double)power);
}

__global__ __launch_bounds__(PE_THREADS) void k_edt_rows(int size, int stride, float power, const int* __restrict__ count,
                                                          float* __restrict__ out)
{
    __shared__ int s_g2[EDT_MAX_SIZE];
    const int y = blockIdx.x;
    const int* g = reinterpret_cast<const int*>(out) + (long)y * stride;
    for (int x = threadIdx.x; x < size; x += PE_THREADS) {
        const int v = g[x];
        s_g2[x] = v * v;
    }
    __syncthreads();                                           // the row is in LDS: it may now be overwritten
    const bool none = *count == 0;                             // no band at all (empty or full target): the transform is 0
    for (int x = threadIdx.x; x < size; x += PE_THREADS) {
        int best = 0x7fffffff;
        for (int xx = 0; xx < size; ++xx) {
            const int dx = x - xx;
            best = min(best, dx * dx + s_g2[xx]);
        }
        out[(long)y * stride + x] = none ? 0.f : edt_power(best, power);
    }
}

int hm_edge_edt(const float* ref, int size, int stride, int kernel_size, float power, float* edt, int* band_count,
                hipStream_t stream)
{
    HM_CHECK_ARG(ref && edt && band_count && size > 0 && size <= EDT_MAX_SIZE && stride >= size);
    HM_CHECK_ARG(power > 0.f);
    if (kernel_size < 1 || kernel_size > 2 * PE_R + 1 || kernel_size % 2 == 0) return HM_ERR_UNSUPPORTED;
    if (hipMemsetAsync(band_count, 0, sizeof(int), stream) != hipSuccess) return HM_ERR_LAUNCH;
    int* g = reinterpret_cast<int*>(edt);
    k_edt_band<<<hm_cdiv((long)size * size, PE_THREADS), PE_THREADS, 0, stream>>>(ref, size, stride, kernel_size / 2, g, band_count);
    k_edt_cols<<<hm_cdiv(size, PE_THREADS), PE_THREADS, 0, stream>>>(size, stride, g);
    k_edt_rows<<<size, PE_THREADS, 0, stream>>>(size, stride, power, band_count, edt);
    return hm_launch_status();
}

// ------------------------------------------------------------------------------------------------ per-step terms
// grid (tiles of the (stride, stride) image, candidates); workgroup = one 64 x 32 tile of one candidate.
//   1. image = keep * alpha of the tile and a 2r halo into LDS (-inf outside the image: never a maximum), edt with an r halo;
//   2. per image row and window column: the maximum of the row's 2r + 1 samples and the FIRST column that holds it;
//   3. per window: the FIRST row whose row maximum is the window's -> the window's argmax in torch's max-pool rule (the first
//      sample in row-major order of the clipped window that holds the maximum), packed in a byte;
//   4. per sample of the tile: the loss terms, and the gather sum over q of edt[q] [argmax(q) == p] over the (2r + 1)^2 windows around it, row-major.
// The tile's four partial sums go to the workspace; the candidate's last tile adds them in tile order.
__global__ __launch_bounds__(PE_THREADS) void k_pose_edge_terms(const float* __restrict__ alpha, const float* __restrict__ keep,
                                                                 const float* __restrict__ ref, const float* __restrict__ edt,
                                                                 int size, int stride, int r, float lw, float* __restrict__ terms,
                                                                 float* __restrict__ grad, unsigned int* __restrict__ tickets,
                                                                 float* __restrict__ partials)
{
    __shared__ float s_img[PE_IH][PE_IW];
    __shared__ float s_hv[PE_IH][PE_WW];
    __shared__ signed char s_hx[PE_IH][PE_WW];
    __shared__ unsigned char s_am[PE_WH][PE_WW];
    __shared__ float s_edt[PE_WH][PE_WW];
    __shared__ float red[64];
    __shared__ int s_flag;
    const int cand = blockIdx.y, tiles_x = (stride + PE_TW - 1) / PE_TW, ntiles = gridDim.x;
    const int ty0 = (blockIdx.x / tiles_x) * PE_TH, tx0 = (blockIdx.x % tiles_x) * PE_TW;
    const long base = (long)cand * stride * stride;
    const float ninf = -__builtin_inff();
    float sums[4] = {0.f, 0.f, 0.f, 0.f};          // sum of squares, intersection, union, chamfer

    if (ty0 < size && tx0 < size) {
        for (int i = threadIdx.x; i < PE_IH * PE_IW; i += PE_THREADS) {
            const int iy = i / PE_IW, ix = i - iy * PE_IW, gy = ty0 - 2 * PE_R + iy, gx = tx0 - 2 * PE_R + ix;
            float v = ninf;
            if (gy >= 0 && gy < size && gx >= 0 && gx < size) v = keep[(long)gy * stride + gx] * alpha[base + (long)gy * stride + gx];
            s_img[iy][ix] = v;
        }
        for (int i = threadIdx.x; i < PE_WH * PE_WW; i += PE_THREADS) {
            const int wy = i / PE_WW, wx = i - wy * PE_WW, gy = ty0 - PE_R + wy, gx = tx0 - PE_R + wx;
            s_edt[wy][wx] = (gy >= 0 && gy < size && gx >= 0 && gx < size) ? edt[(long)gy * stride + gx] : 0.f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < PE_IH * PE_WW; i += PE_THREADS) {
            const int iy = i / PE_WW, wx = i - iy * PE_WW;
            float best = ninf;
            int at = 0;
            for (int dx = -r; dx <= r; ++dx) {
                const float v = s_img[iy][wx + PE_R + dx];
                if (v > best) { best = v; at = dx; }
            }
            s_hv[iy][wx] = best;
            s_hx[iy][wx] = (signed char)at;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < PE_WH * PE_WW; i += PE_THREADS) {
            const int wy = i / PE_WW, wx = i - wy * PE_WW, gy = ty0 - PE_R + wy, gx = tx0 - PE_R + wx;
            int code = PE_NONE;
            if (gy >= 0 && gy < size && gx >= 0 && gx < size) {
                float best = ninf;
                int at = 0;
                for (int dy = -r; dy <= r; ++dy) {
                    const float v = s_hv[wy + PE_R + dy][wx];
                    if (v > best) { best = v; at = dy; }
                }
                code = (at + PE_R) * 8 + ((int)s_hx[wy + PE_R + at][wx] + PE_R);
            }
            s_am[wy][wx] = (unsigned char)code;
        }
        __syncthreads();
    }

    const int lx = threadIdx.x & (PE_TW - 1);
    for (int ly = threadIdx.x / PE_TW; ly < PE_TH; ly += PE_THREADS / PE_TW) {
        const int gy = ty0 + ly, gx = tx0 + lx;
        if (gy >= stride || gx >= stride) continue;
        float gout = 0.f;
        if (gy < size && gx < size) {
            const long at = (long)gy * stride + gx;
            const float img = s_img[ly + 2 * PE_R][lx + 2 * PE_R], rf = ref[at], kp = keep[at], e = s_edt[ly + PE_R][lx + PE_R];
            const float d = img - rf;
            sums[0] += d * d;
            sums[1] += img * rf;
            sums[2] += fminf(fmaxf(img + rf, 0.f), 1.f);
            const int own = s_am[ly + PE_R][lx + PE_R];
            const float pooled = s_img[ly + PE_R + (own >> 3)][lx + PE_R + (own & 7)];
            sums[3] += (pooled - img) * e;
            float named = 0.f;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const int want = (PE_R - dy) * 8 + (PE_R - dx);
                    if (s_am[ly + PE_R + dy][lx + PE_R + dx] == want) named += s_edt[ly + PE_R + dy][lx + PE_R + dx];
                }
            gout = kp * (2.f * d + lw * (named - e));
        }
        grad[base + (long)gy * stride + gx] = gout;
    }

    hm_block_sum_n<4>(sums, red);
    float* mine = partials + ((long)cand * ntiles + blockIdx.x) * 4;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) hm_partial_store(mine + k, sums[k]);
    }
    if (hm_last_block(tickets + cand, ntiles, &s_flag)) {
        const float* all = partials + (long)cand * ntiles * 4;
        const float sq = hm_last_block_sum(all, ntiles, 4, red);
        const float in = hm_last_block_sum(all + 1, ntiles, 4, red);
        const float un = hm_last_block_sum(all + 2, ntiles, 4, red);
        const float ch = hm_last_block_sum(all + 3, ntiles, 4, red);
        if (threadIdx.x == 0) {
            const float weighted = lw * ch;                    // loss_dict["chamfer"] (:148)
            terms[4 * cand] = sq + weighted;                   // sum(loss_dict.values()) before "offscreen" joins
            terms[4 * cand + 1] = in / (un + 1e-6f);           // batch_mask_iou
            terms[4 * cand + 2] = sq;
            terms[4 * cand + 3] = ch;
        }
    }
}

static inline int pe_tiles(int stride) { return hm_cdiv(stride, PE_TW) * hm_cdiv(stride, PE_TH); }

size_t hm_pose_edge_workspace_bytes(int N, int stride)
{
    if (N <= 0 || stride <= 0) return 0;
    return (size_t)N * sizeof(unsigned int) + (size_t)N * pe_tiles(stride) * 4 * sizeof(float);
}

int hm_pose_edge_terms(const float* alpha, const float* keep, const float* ref, const float* edt, int N, int size, int stride,
                       int kernel_size, float lw_chamfer, float* terms, float* grad, void* workspace, hipStream_t stream)
{
    HM_CHECK_ARG(alpha && keep && ref && edt && terms && grad && workspace);
    HM_CHECK_ARG(HM_ALIGNED(workspace, 4));          // 32-bit tickets (atomic targets), then fp32 partial sums
    HM_CHECK_ARG(N > 0 && N <= 65535 && size > 0 && stride >= size);
    if (kernel_size < 3 || kernel_size > 2 * PE_R + 1 || kernel_size % 2 == 0) return HM_ERR_UNSUPPORTED;
    unsigned int* tickets = static_cast<unsigned int*>(workspace);
    float* partials = reinterpret_cast<float*>(tickets + N);
    k_pose_edge_terms<<<dim3(pe_tiles(stride), N), PE_THREADS, 0, stream>>>(alpha, keep, ref, edt, size, stride, kernel_size / 2,
                                                                             lw_chamfer, terms, grad, tickets, partials);
    return hm_launch_status();
}
