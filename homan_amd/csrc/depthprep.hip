// depthprep.hip -- raw sensor depth frames registered onto the fit's pixel grid (a homan_amd extra, not in the reference tree;
// the rule is in include/homan_amd.h and DESIGN.md section 7, restated in tests/depthprep_ref.py)
#include "hm_common.h"

// Three launches on one stream: k_depth_fill (the output becomes a z-buffer of +inf patterns, the statistics zero),
// k_depth_splat (one workgroup per 64x16 source tile) and k_depth_finish (the sentinel becomes 0.0f, valid pixels are counted).
// The splat stages its tile with a halo of `r` pixels in LDS as METRES (0.0f = no measurement: a valid value is >= znear > 0),
// so the edge filter reads LDS only; every lane then owns four source pixels, one per four rows.  A surviving pixel writes its
// transformed depth with an UNSIGNED INTEGER atomicMin - positive floats order like their bit patterns - so a target pixel's
// value is the minimum of the SET of values it received: the same bits in any order of lanes, workgroups and frames.
// Statistics are integer sums: per lane, across the wave, one LDS add per wave, one global atomic per workgroup and column.
#define DREG_TW 64
#define DREG_TH 16
#define DREG_RMAX 3
#define DREG_PITCH (DREG_TW + 2 * DREG_RMAX)
#define DREG_ROWS (DREG_TH + 2 * DREG_RMAX)
#define DREG_INF 0x7f800000u
#define DREG_PX_MAX 16777216.0f        // 2^24: a projected corner beyond it (or NaN) drops the pixel

__device__ __forceinline__ int dreg_wave_sum(int v)      // integers: the order is immaterial
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid ceil(max(items, 4 B) / 256): items = B S S / 4 sixteen-byte stores (vec) or B S S words
__global__ __launch_bounds__(256) void k_depth_fill(unsigned* __restrict__ out, long items, int vec, int* __restrict__ stats, int B)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < items) {
        if (vec) reinterpret_cast<uint4*>(out)[i] = make_uint4(DREG_INF, DREG_INF, DREG_INF, DREG_INF);
        else out[i] = DREG_INF;
    }
    if (i < 4L * B) stats[i] = 0;
}

__device__ __forceinline__ float dreg_metres(float raw, float scale, float znear, float zfar)
{
    const float z = raw * scale;
    return (z >= znear && z <= zfar) ? z : 0.f;         // (false for NaN, +-inf, zero and negative values)
}

// grid (ceil(Wd / 64), ceil(Hd / 16), B)
__global__ __launch_bounds__(256) void k_depth_splat(const void* __restrict__ frames, int is_f32, int vecload, int Hd, int Wd,
                                                      float scale, const float* __restrict__ Kd, int kd_stride,
                                                      const float* __restrict__ T, int t_stride, const float* __restrict__ Kc,
                                                      int kc_stride, int S, float znear, float zfar, int r, float jump_abs,
                                                      float jump_rel, int max_splat, unsigned* out, int* stats)
{
    __shared__ float tile[DREG_ROWS * DREG_PITCH];
    __shared__ int s_cnt[4];            // valid, edge-dropped, range / splat-dropped; [3]: the tile holds a measurement
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * DREG_TW, y0 = blockIdx.y * DREG_TH;
    const long fbase = (long)b * Hd * Wd;
    const float* f32 = static_cast<const float*>(frames);
    const unsigned short* u16 = static_cast<const unsigned short*>(frames);
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    // ---- stage the tile and its halo as metres
    const int tw = DREG_TW + 2 * r, th = DREG_TH + 2 * r;
    const bool vec = vecload && x0 + DREG_TW <= Wd;      // (block-uniform: whole 16-byte groups of a row that starts aligned)
    bool any = false;
    for (int i = tid; i < tw * th; i += 256) {
        const int ty = i / tw, tx = i - ty * tw;
        if (vec && tx >= r && tx < r + DREG_TW && ty >= r && ty < r + DREG_TH) continue;
        const int gx = x0 - r + tx, gy = y0 - r + ty;
        float z = 0.f;
        if (gx >= 0 && gx < Wd && gy >= 0 && gy < Hd) {
            const long idx = fbase + (long)gy * Wd + gx;
            z = dreg_metres(is_f32 ? f32[idx] : (float)u16[idx], scale, znear, zfar);
        }
        tile[ty * DREG_PITCH + tx] = z;
        any = any || z != 0.f;
    }
    if (vec && is_f32) {                                  // 16 rows x 16 lanes, four floats each
        const int row = tid >> 4, seg = tid & 15, gy = y0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool in = gy < Hd;
        if (in) v = *reinterpret_cast<const float4*>(f32 + fbase + (long)gy * Wd + x0 + 4 * seg);
        const float raw[4] = {v.x, v.y, v.z, v.w};
        float* dst = tile + (row + r) * DREG_PITCH + r + 4 * seg;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float z = in ? dreg_metres(raw[k], scale, znear, zfar) : 0.f;
            dst[k] = z;
            any = any || z != 0.f;
        }
    } else if (vec && tid < 128) {                        // 16 rows x 8 lanes, eight uint16 each
        const int row = tid >> 3, seg = tid & 7, gy = y0 + row;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        const bool in = gy < Hd;
        if (in) v = *reinterpret_cast<const uint4*>(u16 + fbase + (long)gy * Wd + x0 + 8 * seg);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        float* dst = tile + (row + r) * DREG_PITCH + r + 8 * seg;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned raw = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
            const float z = in ? dreg_metres((float)raw, scale, znear, zfar) : 0.f;
            dst[k] = z;
            any = any || z != 0.f;
        }
    }
    if (any) s_cnt[3] = 1;
    __syncthreads();
    if (!s_cnt[3]) return;              // (workgroup-uniform: nothing measured in the tile or its halo)
    // ---- the frame's cameras, in registers
    const float* kd = Kd + 9L * kd_stride * b;
    const float* tm = T + 12L * t_stride * b;
    const float* kc = Kc + 9L * kc_stride * b;
    const float fxd = kd[0], cxd = kd[2], fyd = kd[4], cyd = kd[5];
    float t[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = tm[k];
    const float Sf = (float)S;
    const float Fx = kc[0] * Sf, Cx = kc[2] * Sf, Fy = kc[4] * Sf, Cy = kc[5] * Sf;
    const long obase = (long)b * S * S;
    int n_valid = 0, n_edge = 0, n_drop = 0;
    const int lx = tid & 63;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int ly = (tid >> 6) + 4 * k;
        const float z = tile[(ly + r) * DREG_PITCH + lx + r];
        if (z == 0.f) continue;         // invalid, or outside the frame
        ++n_valid;
        const float thr = jump_rel * z + jump_abs;
        bool edge = false;
        for (int dy = 0; dy <= 2 * r; ++dy)
            for (int dx = 0; dx <= 2 * r; ++dx) {
                const float zn = tile[(ly + dy) * DREG_PITCH + lx + dx];
                edge = edge || (zn != 0.f && fabsf(zn - z) > thr);
            }
        if (edge) { ++n_edge; continue; }
        const int gx = x0 + lx, gy = y0 + ly;
        const float u0 = (float)gx, v0 = (float)gy, u1 = (float)(gx + 1), v1 = (float)(gy + 1);
        const float um = u0 + 0.5f, vm = v0 + 0.5f;
        const float X0 = ((u0 - cxd) / fxd) * z, Y0 = ((v0 - cyd) / fyd) * z;
        const float X1 = ((u1 - cxd) / fxd) * z, Y1 = ((v1 - cyd) / fyd) * z;
        const float Xm = ((um - cxd) / fxd) * z, Ym = ((vm - cyd) / fyd) * z;
        const float zc = ((t[8] * Xm + t[9] * Ym) + t[10] * z) + t[11];
        const float Xc0 = ((t[0] * X0 + t[1] * Y0) + t[2] * z) + t[3], Yc0 = ((t[4] * X0 + t[5] * Y0) + t[6] * z) + t[7];
        const float Zc0 = ((t[8] * X0 + t[9] * Y0) + t[10] * z) + t[11];
        const float Xc1 = ((t[0] * X1 + t[1] * Y1) + t[2] * z) + t[3], Yc1 = ((t[4] * X1 + t[5] * Y1) + t[6] * z) + t[7];
        const float Zc1 = ((t[8] * X1 + t[9] * Y1) + t[10] * z) + t[11];
        if (!(zc >= znear && zc <= zfar && Zc0 >= znear && Zc1 >= znear)) { ++n_drop; continue; }
        const float px0 = (Xc0 / Zc0) * Fx + Cx, py0 = (Yc0 / Zc0) * Fy + Cy;
        const float px1 = (Xc1 / Zc1) * Fx + Cx, py1 = (Yc1 / Zc1) * Fy + Cy;
        if (!(fabsf(px0) <= DREG_PX_MAX && fabsf(px1) <= DREG_PX_MAX && fabsf(py0) <= DREG_PX_MAX && fabsf(py1) <= DREG_PX_MAX)) {
            ++n_drop;
            continue;
        }
        // target pixels whose centre c + 0.5 lies in [lo, hi): ceil(lo - 0.5) <= c < ceil(hi - 0.5), clipped to the image
        const float xa = fminf(px0, px1), xb = fmaxf(px0, px1), ya = fminf(py0, py1), yb = fmaxf(py0, py1);
        const int c0 = (int)fmaxf(ceilf(xa - 0.5f), 0.f), c1 = (int)fminf(ceilf(xb - 0.5f), Sf);
        const int r0 = (int)fmaxf(ceilf(ya - 0.5f), 0.f), r1 = (int)fminf(ceilf(yb - 0.5f), Sf);
        if (c1 <= c0 || r1 <= r0) continue;               // no pixel centre inside: nothing written, nothing counted
        if (c1 - c0 > max_splat || r1 - r0 > max_splat) { ++n_drop; continue; }
        const unsigned bits = __float_as_uint(zc);
        for (int row = r0; row < r1; ++row)
            for (int col = c0; col < c1; ++col) atomicMin(out + obase + (long)row * S + col, bits);
    }
    n_valid = dreg_wave_sum(n_valid); n_edge = dreg_wave_sum(n_edge); n_drop = dreg_wave_sum(n_drop);
    if ((tid & 63) == 0) {
        if (n_valid) atomicAdd(&s_cnt[0], n_valid);
        if (n_edge) atomicAdd(&s_cnt[1], n_edge);
        if (n_drop) atomicAdd(&s_cnt[2], n_drop);
    }
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(stats + 4 * b + tid, s_cnt[tid]);
}

// grid (ceil(groups / 256), B): four pixels per lane when S * S is a multiple of 4, else one
__global__ __launch_bounds__(256) void k_depth_finish(unsigned* out, int S, int vec, int* stats)
{
    __shared__ int s_n;
    const int b = blockIdx.y, npix = S * S;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned* o = out + (long)b * npix;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int n = 0;
    if (vec) {
        if (4 * i < npix) {
            uint4 v = reinterpret_cast<uint4*>(o)[i];
            v.x = v.x == DREG_INF ? 0u : v.x; v.y = v.y == DREG_INF ? 0u : v.y;
            v.z = v.z == DREG_INF ? 0u : v.z; v.w = v.w == DREG_INF ? 0u : v.w;
            n = (v.x != 0u) + (v.y != 0u) + (v.z != 0u) + (v.w != 0u);
            reinterpret_cast<uint4*>(o)[i] = v;
        }
    } else if (i < npix) {
        const unsigned v = o[i] == DREG_INF ? 0u : o[i];
        n = v != 0u;
        o[i] = v;
    }
    n = dreg_wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(stats + 4 * b + 3, s_n);
}

extern "C" {
// ALIGNMENT (checked here, before any HIP call): frames to its element (2 bytes uint16, 4 bytes fp32); out 16 bytes when S * S
// is a multiple of 4 (fill and finish move four pixels at a time), else 4.  The 16-byte loads of the source rows are taken only
// where `frames` and the row pitch allow them (vecload), so they ask for nothing.
int hm_depth_register(const void* frames, int frames_f32, int B, int Hd, int Wd, float depth_scale, const float* Kd, int Kd_stride,
                      const float* T, int T_stride, const float* Kc, int Kc_stride, int S, float znear, float zfar,
                      int edge_radius, float edge_jump_abs, float edge_jump_rel, int max_splat, float* out, int* stats,
                      hipStream_t stream)
{
    HM_CHECK_ARG(frames && Kd && T && Kc && out && stats);
    HM_CHECK_ARG(B >= 1 && B <= 65535 && Hd >= 1 && Wd >= 1 && S >= 1 && S <= 1024);
    HM_CHECK_ARG((long)Hd * Wd <= 0x7fffffffL && hm_cdiv(Hd, DREG_TH) <= 65535);
    HM_CHECK_ARG(edge_radius >= 0 && edge_radius <= DREG_RMAX && max_splat >= 1);
    HM_CHECK_ARG(depth_scale > 0.f && depth_scale <= 3.402823466e38f);
    HM_CHECK_ARG(znear > 0.f && zfar > znear && zfar <= 100.f);
    HM_CHECK_ARG(edge_jump_abs >= 0.f && edge_jump_abs <= 3.402823466e38f && edge_jump_rel >= 0.f && edge_jump_rel <= 3.402823466e38f);
    HM_CHECK_ARG((Kd_stride == 0 || Kd_stride == 1) && (T_stride == 0 || T_stride == 1) && (Kc_stride == 0 || Kc_stride == 1));
    const bool vec = ((long)S * S) % 4 == 0;
    HM_CHECK_ARG(HM_ALIGNED(frames, frames_f32 ? 4 : 2) && HM_ALIGNED(out, vec ? 16 : 4));
    HM_CHECK_ARG(HM_ALIGNED(Kd, 4) && HM_ALIGNED(T, 4) && HM_ALIGNED(Kc, 4) && HM_ALIGNED(stats, 4));
    const int vecload = HM_ALIGNED(frames, 16) && Wd % (frames_f32 ? 4 : 8) == 0;
    const long items = vec ? (long)B * S * S / 4 : (long)B * S * S;
    unsigned* o = reinterpret_cast<unsigned*>(out);
    hipLaunchKernelGGL(k_depth_fill, dim3(hm_cdiv(items > 4L * B ? items : 4L * B, 256)), dim3(256), 0, stream, o, items, (int)vec,
                       stats, B);
    hipLaunchKernelGGL(k_depth_splat, dim3(hm_cdiv(Wd, DREG_TW), hm_cdiv(Hd, DREG_TH), B), dim3(256), 0, stream, frames,
                       frames_f32 != 0, vecload, Hd, Wd, depth_scale, Kd, Kd_stride, T, T_stride, Kc, Kc_stride, S, znear, zfar,
                       edge_radius, edge_jump_abs, edge_jump_rel, max_splat, o, stats);
    hipLaunchKernelGGL(k_depth_finish, dim3(hm_cdiv(vec ? S * S / 4 : S * S, 256), B), dim3(256), 0, stream, o, S, (int)vec, stats);
    return hm_launch_status();
}
}  // extern "C"
