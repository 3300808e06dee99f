// maskcrop.hip -- crop-and-resize of instance masks, the -1 / 0 / 1 target masks built from it, and per-instance
// visibility masks off the rasteriser's face-index map.
//
// Replaces detectron2's `BitMasks.crop_and_resize` as called at reference homan/lib2d/maskutils.py:29-30, :61-64 and
// homan/prepare/gtmasks.py:87-101: ROIAlign (output (S,S), spatial_scale 1, sampling_ratio 0, aligned) of the binarised
// mask in fp32, then >= 0.5.  Every operation is a separate fp32 rounding (the library builds with -ffp-contract=off) and
// the samples of one output pixel are summed by ONE lane, row by row: the result is the float a scalar loop in the same
// order produces, so exact 0.5 ties fall the same way as in tests/maskcrop_ref.py.
#include "hm_common.h"

#define MC_THREADS 256
#define MC_MAX_INSTANCES 8
#define MC_MAX_GRID_Y 65535

template <typename T>
__device__ __forceinline__ float mc_bit(const T* __restrict__ m, long at) { return m[at] != (T)0 ? 1.f : 0.f; }

// ROIAlign's bilinear_interpolate on the binarised mask m (H,W); (y, x) in pixels of the mask.
template <typename T>
__device__ __forceinline__ float mc_bilinear(const T* __restrict__ m, int H, int W, float y, float x)
{
    if (!(y >= -1.f && y <= (float)H && x >= -1.f && x <= (float)W)) return 0.f;      // (also rejects NaN)
    if (y <= 0.f) y = 0.f;
    if (x <= 0.f) x = 0.f;
    int yl = (int)y, xl = (int)x, yh, xh;
    if (yl >= H - 1) { yh = yl = H - 1; y = (float)yl; } else yh = yl + 1;
    if (xl >= W - 1) { xh = xl = W - 1; x = (float)xl; } else xh = xl + 1;
    const float ly = y - (float)yl, lx = x - (float)xl, hy = 1.f - ly, hx = 1.f - lx;
    const float v1 = mc_bit(m, (long)yl * W + xl), v2 = mc_bit(m, (long)yl * W + xh);
    const float v3 = mc_bit(m, (long)yh * W + xl), v4 = mc_bit(m, (long)yh * W + xh);
    return ((hy * hx) * v1 + (hy * lx) * v2) + ((ly * hx) * v3 + (ly * lx) * v4);
}

// output pixel (ph, pw) of the S x S crop of mask m to `box` (x1 y1 x2 y2): true iff the sample mean is >= 0.5
template <typename T>
__device__ __forceinline__ bool mc_crop_pixel(const T* __restrict__ m, int H, int W, const float* __restrict__ box, int S,
                                              int ph, int pw)
{
    const float x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
    const float sx = x1 - 0.5f, sy = y1 - 0.5f, rw = x2 - x1, rh = y2 - y1;
    const float bw = rw / (float)S, bh = rh / (float)S;
    // A bin more than four images wide holds under a third of its samples (spaced <= 1 pixel) inside the image, the others
    // read 0: the mean stays below 0.5.  Decided here so that no box, however large, makes the sample loop long.
    if (bw > 4.f * (float)(W + 2) || bh > 4.f * (float)(H + 2)) return false;
    const int gw = (int)fmaxf(ceilf(rw / (float)S), 1.f), gh = (int)fmaxf(ceilf(rh / (float)S), 1.f);
    const float y0 = sy + (float)ph * bh, x0 = sx + (float)pw * bw;
    float acc = 0.f;
    for (int iy = 0; iy < gh; ++iy) {
        const float y = y0 + (((float)iy + 0.5f) * bh) / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
            const float x = x0 + (((float)ix + 0.5f) * bw) / (float)gw;
            acc += mc_bilinear(m, H, W, y, x);
        }
    }
    return acc / (float)(gh * gw) >= 0.5f;
}

// either element type behind one pointer (the dicts of the reference hold bool / byte masks and float ones)
__device__ __forceinline__ bool mc_crop_any(const void* __restrict__ masks, int is_f32, long n, int H, int W,
                                            const float* __restrict__ box, int S, int ph, int pw)
{
    const long at = n * H * W;
    return is_f32 ? mc_crop_pixel((const float*)masks + at, H, W, box, S, ph, pw)
                  : mc_crop_pixel((const uint8_t*)masks + at, H, W, box, S, ph, pw);
}

// grid (ceil(S*S/256), ROIs of this launch); ROI = r0 + blockIdx.y; one lane per output pixel.  An index outside [0, N)
// gives an empty crop.
__global__ __launch_bounds__(MC_THREADS) void k_mask_crop_resize(const void* __restrict__ masks, int is_f32, int N, int H, int W,
                                                                  const int* __restrict__ index,
                                                                  const float* __restrict__ boxes, int S,
                                                                  uint8_t* __restrict__ out, int r0)
{
    const long r = (long)r0 + blockIdx.y;
    const int pix = blockIdx.x * MC_THREADS + threadIdx.x;
    if (pix >= S * S) return;
    const int ph = pix / S, pw = pix - ph * S;
    const int n = index ? index[r] : (int)r;
    bool on = false;
    if (n >= 0 && n < N) on = mc_crop_any(masks, is_f32, n, H, W, boxes + 4 * r, S, ph, pw);
    out[r * S * S + pix] = on ? 1 : 0;
}

// mode 0 (hand, maskutils.py:61-65): t = crop(target); -1 where a cropped occluder is set
// mode 1 (object, maskutils.py:29-36): target is an (S,S) crop already; -1 where a cropped occluder is set, 1 where the
//         target is set
// mode 2 (ground-truth masks, gtmasks.py:105-107): crop(target) - (any cropped occluder)
// occ_index (R,K): occluder masks of the ROI, negative entries are skipped.  Same launch shape as k_mask_crop_resize.
__global__ __launch_bounds__(MC_THREADS) void k_target_masks(int mode, const void* __restrict__ target, int target_f32, int Nt,
                                                              const int* __restrict__ target_index,
                                                              const void* __restrict__ occ, int occ_f32, int No,
                                                              const int* __restrict__ occ_index, int K, int H, int W,
                                                              const float* __restrict__ boxes, int S,
                                                              float* __restrict__ out, int r0)
{
    const long r = (long)r0 + blockIdx.y;
    const int pix = blockIdx.x * MC_THREADS + threadIdx.x;
    if (pix >= S * S) return;
    const int ph = pix / S, pw = pix - ph * S;
    const float* box = boxes + 4 * r;
    const int nt = target_index ? target_index[r] : (int)r;
    bool t = false;
    if (nt >= 0 && nt < Nt) {
        if (mode == 1) {
            const long at = (long)nt * S * S + pix;
            t = target_f32 ? ((const float*)target)[at] != 0.f : ((const uint8_t*)target)[at] != 0;
        } else {
            t = mc_crop_any(target, target_f32, nt, H, W, box, S, ph, pw);
        }
    }
    bool o = false;
    if (!(mode == 1 && t)) {                  // (the object wins: its pixels do not need the occluders)
        for (int k = 0; k < K && !o; ++k) {
            const int no = occ_index[r * K + k];
            if (no >= 0 && no < No) o = mc_crop_any(occ, occ_f32, no, H, W, box, S, ph, pw);
        }
    }
    float v;
    if (mode == 0) v = o ? -1.f : (t ? 1.f : 0.f);
    else if (mode == 1) v = t ? 1.f : (o ? -1.f : 0.f);
    else v = (t ? 1.f : 0.f) - (o ? 1.f : 0.f);
    out[r * S * S + pix] = v;
}

struct McRanges { int start[MC_MAX_INSTANCES + 1]; };

// idx_map (B,2S,2S): owner face of every sample as the rasteriser leaves it (-1 empty, f + F = the reversed copy of face f,
// sample rows bottom-up).  out (B,I,S,S): how many of the pixel's 2x2 samples a face of [start[i], start[i+1]) owns (0..4);
// count / 4 is the anti-aliased render of a one-hot face colour under ambient light 1, count > 0 the instance mask.
__global__ __launch_bounds__(MC_THREADS) void k_instance_masks(const int* __restrict__ idx_map, int S, int F, McRanges rg, int I,
                                                                uint8_t* __restrict__ out)
{
    const long b = blockIdx.y;
    const int pix = blockIdx.x * MC_THREADS + threadIdx.x;
    if (pix >= S * S) return;
    const int r = pix / S, c = pix - r * S, is = 2 * S;
    const int* idx = idx_map + b * is * is;
    int cnt[MC_MAX_INSTANCES];
#pragma unroll
    for (int i = 0; i < MC_MAX_INSTANCES; ++i) cnt[i] = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int yi = is - 1 - (2 * r + (q >> 1)), xi = 2 * c + (q & 1);
        const int fn = idx[(long)yi * is + xi];
        if (fn < 0) continue;
        const int f = fn >= F ? fn - F : fn;
#pragma unroll
        for (int i = 0; i < MC_MAX_INSTANCES; ++i)
            if (i < I && f >= rg.start[i] && f < rg.start[i + 1]) ++cnt[i];
    }
#pragma unroll
    for (int i = 0; i < MC_MAX_INSTANCES; ++i)
        if (i < I) out[((b * I + i) * S) * S + pix] = (uint8_t)cnt[i];
}

extern "C" {
int hm_mask_crop_resize(const void* masks, int masks_f32, int N, int H, int W, const int* index, const float* boxes, int R,
                        int S, unsigned char* out, hipStream_t stream)
{
    HM_CHECK_ARG(R >= 0 && S > 0 && S <= 4096 && N > 0 && H > 0 && W > 0 && (long)H * W <= 0x7fffffffL);
    if (R == 0) return HM_OK;
    HM_CHECK_ARG(masks && boxes && out);
    HM_CHECK_ARG(!masks_f32 || HM_ALIGNED(masks, 4));                 // the void pointer: bytes or fp32
    for (int r0 = 0; r0 < R; r0 += MC_MAX_GRID_Y) {
        const int nr = min(R - r0, MC_MAX_GRID_Y);
        hipLaunchKernelGGL(k_mask_crop_resize, dim3(hm_cdiv((long)S * S, MC_THREADS), nr), dim3(MC_THREADS), 0, stream, masks,
                           masks_f32, N, H, W, index, boxes, S, out, r0);
    }
    return hm_launch_status();
}

int hm_target_masks(int mode, const void* target, int target_f32, int Nt, const int* target_index, const void* occluders,
                    int occluders_f32, int No, const int* occluder_index, int K, int H, int W, const float* boxes, int R, int S,
                    float* out, hipStream_t stream)
{
    HM_CHECK_ARG(mode >= 0 && mode <= 2 && R >= 0 && S > 0 && S <= 4096 && Nt > 0 && No >= 0 && K >= 0 && H > 0 && W > 0 &&
                 (long)H * W <= 0x7fffffffL);
    if (R == 0) return HM_OK;
    HM_CHECK_ARG(target && boxes && out && (K == 0 || (occluders && occluder_index && No > 0)));
    HM_CHECK_ARG((!target_f32 || HM_ALIGNED(target, 4)) && (!occluders_f32 || HM_ALIGNED(occluders, 4)));      // void: bytes or fp32
    for (int r0 = 0; r0 < R; r0 += MC_MAX_GRID_Y) {
        const int nr = min(R - r0, MC_MAX_GRID_Y);
        hipLaunchKernelGGL(k_target_masks, dim3(hm_cdiv((long)S * S, MC_THREADS), nr), dim3(MC_THREADS), 0, stream, mode, target,
                           target_f32, Nt, target_index, occluders, occluders_f32, No, occluder_index, K, H, W, boxes, S, out,
                           r0);
    }
    return hm_launch_status();
}

int hm_instance_masks(const int* idx_map, int B, int S, int F, const int* face_start, int I, unsigned char* out,
                      hipStream_t stream)
{
    HM_CHECK_ARG(idx_map && face_start && out && B > 0 && B <= MC_MAX_GRID_Y && S > 0 && S <= 8192 && F > 0 && I > 0);
    if (I > MC_MAX_INSTANCES) return HM_ERR_UNSUPPORTED;
    McRanges rg;
    for (int i = 0; i <= MC_MAX_INSTANCES; ++i) rg.start[i] = face_start[i <= I ? i : I];
    for (int i = 0; i < I; ++i) HM_CHECK_ARG(rg.start[i] >= 0 && rg.start[i] <= rg.start[i + 1] && rg.start[i + 1] <= F);
    hipLaunchKernelGGL(k_instance_masks, dim3(hm_cdiv((long)S * S, MC_THREADS), B), dim3(MC_THREADS), 0, stream, idx_map, S, F, rg,
                       I, out);
    return hm_launch_status();
}
}  // extern "C"
