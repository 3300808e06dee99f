// softsil.hip -- soft silhouette rasteriser with its true gradient (Liu et al. 2019, "Soft Rasterizer", silhouette branch).
// A NON-PARITY extra beside the hard rasteriser the reference calls at homan/losses.py:187: same projection, another image
// formation.  Semantics (include/homan_amd.h, hm_softsil_fwd): per pixel p and participating face j, d2 = squared NDC distance
// to the nearest edge segment, x = +-d2 / sigma (+ inside), D = sigmoid(x), outside pairs with d2 >= 16 sigma dropped,
// A_p = 1 - prod_j (1 - D_jp); backward dA_p / dx_jp = (1 - A_p) D_jp.
//
//   k_softsil_setup    one thread per (frame, face): projection, validity, pixel box enlarged by the cutoff radius
//   k_softsil_fwd      one workgroup per 16x16-pixel tile: faces staged through LDS in index order, 256 at a time, the ones
//                      whose box misses the tile compacted out (ballot + prefix: order kept); a lane owns a pixel
//   k_softsil_bwd      one wave per (frame, face) over the pixels of its box; six NDC partials per lane, DPP butterfly
//   k_softsil_gather   one thread per (frame, vertex): CSR sum in stored order, then the projection's Jacobian
// No atomics on results, every sum in a fixed order: two calls agree bit for bit.  sigma is read on the device by every kernel.
#include "hm_common.h"

#define SOFTSIL_TILE 16
#define SOFTSIL_CHUNK 256          // faces staged per pass = threads of a tile workgroup
#define SOFTSIL_CUT 16.0f          // outside pairs with d2 >= SOFTSIL_CUT * sigma are dropped: sigmoid(-16) = 1.13e-7
#define SOFTSIL_MIN_AREA2 1e-10f   // |twice the signed NDC area| below this: the face takes no part
#define SOFTSIL_MAX_BLOCKS (1 << 20)

struct SoftFace {                  // 48 bytes per (frame, face)
    float x0, y0, x1, y1, x2, y2;  // NDC corners
    int c0, r0, c1, r1;            // pixel box (inclusive) enlarged by the cutoff radius, clipped to the image; empty: c1 < c0
    int valid, pad;
};

static size_t softsil_parts_offset(int B, int F) { return (size_t)B * F * sizeof(SoftFace); }

// nr.projection with zero distortion: the operations of project_vertex (raster_setup.hip), in its order, so that hard and soft
// mode place a vertex on the same NDC floats
__device__ __forceinline__ void softsil_project(const float* __restrict__ p, const float* __restrict__ k, float orig_size, float* uv)
{
    const float zz = p[2] + 1e-9f;
    const float xn = p[0] / zz, yn = p[1] / zz;
    float u = xn * k[0] + yn * k[1];
    u = u + k[2];
    float v = xn * k[3] + yn * k[4];
    v = v + k[5];
    v = orig_size - v;
    uv[0] = 2.0f * (u - orig_size / 2.0f) / orig_size;
    uv[1] = 2.0f * (v - orig_size / 2.0f) / orig_size;
}

__device__ __forceinline__ bool softsil_sigma_ok(float s) { return s > 0.0f && s <= 3.0e38f; }

__global__ __launch_bounds__(256) void k_softsil_setup(const float* __restrict__ verts, const int* __restrict__ faces,
                                                       const float* __restrict__ K, long BF, int V, int F, int S,
                                                       float orig_size, float znear, float zfar,
                                                       const float* __restrict__ sigma, SoftFace* __restrict__ rec)
{
    const float sg = sigma[0];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < BF; i += (long)gridDim.x * blockDim.x) {
        const long b = i / F;
        const int f = (int)(i - b * F);
        SoftFace o;
        o.x0 = o.y0 = o.x1 = o.y1 = o.x2 = o.y2 = 0.0f;
        o.c0 = o.r0 = 32767; o.c1 = o.r1 = -1; o.valid = 0; o.pad = 0;
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (softsil_sigma_ok(sg) && i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
            const float* p0 = verts + (b * V + i0) * 3;
            const float* p1 = verts + (b * V + i1) * 3;
            const float* p2 = verts + (b * V + i2) * 3;
            float a[2], c[2], d[2];
            softsil_project(p0, K + b * 9, orig_size, a);
            softsil_project(p1, K + b * 9, orig_size, c);
            softsil_project(p2, K + b * 9, orig_size, d);
            const float area2 = (c[0] - a[0]) * (d[1] - a[1]) - (d[0] - a[0]) * (c[1] - a[1]);
            const bool zin = p0[2] > znear && p0[2] < zfar && p1[2] > znear && p1[2] < zfar && p2[2] > znear && p2[2] < zfar;
            if (zin && fabsf(area2) >= SOFTSIL_MIN_AREA2) {          // (a NaN anywhere fails one of the comparisons)
                o.valid = 1;
                o.x0 = a[0]; o.y0 = a[1]; o.x1 = c[0]; o.y1 = c[1]; o.x2 = d[0]; o.y2 = d[1];
                // Pixel (r, c) has its centre at x = (2c + 1 - S) / S, y = (S - 1 - 2r) / S.  A pixel that counts lies inside
                // the face or nearer than the cutoff radius to it, i.e. within the corners' bounds grown by that radius;
                // floor / ceil the other way round leave up to a pixel of slack, far above the rounding of these few operations.
                const float rad = sqrtf(SOFTSIL_CUT * sg) * 1.000001f;
                const float xmin = fminf(a[0], fminf(c[0], d[0])) - rad, xmax = fmaxf(a[0], fmaxf(c[0], d[0])) + rad;
                const float ymin = fminf(a[1], fminf(c[1], d[1])) - rad, ymax = fmaxf(a[1], fmaxf(c[1], d[1])) + rad;
                const float fs = (float)S;
                const float cl = (xmin * fs + fs - 1.0f) * 0.5f, ch = (xmax * fs + fs - 1.0f) * 0.5f;
                const float rl = (fs - 1.0f - ymax * fs) * 0.5f, rh = (fs - 1.0f - ymin * fs) * 0.5f;
                // (clamped as floats first: far off-screen corners, infinities and NaN never reach the conversion)
                const int c0 = (int)floorf(fmaxf(fminf(cl, fs), -1.0f)), c1 = (int)ceilf(fmaxf(fminf(ch, fs), -1.0f));
                const int r0 = (int)floorf(fmaxf(fminf(rl, fs), -1.0f)), r1 = (int)ceilf(fmaxf(fminf(rh, fs), -1.0f));
                o.c0 = max(c0, 0); o.c1 = min(c1, S - 1); o.r0 = max(r0, 0); o.r1 = min(r1, S - 1);
                if (o.c1 < o.c0 || o.r1 < o.r0) { o.c0 = o.r0 = 32767; o.c1 = o.r1 = -1; }      // off-screen beyond the cutoff
            }
        }
        rec[i] = o;
    }
}

// One (pixel, face) pair: x = +-d2 / sigma and whether the pair counts.  With `grad`, also the nearest segment's foot
// parameters for the backward: d2 = |q|^2 with q = (p - a) - t (b - a), t clamped to [0, 1]; a and b = corners e and (e + 1) % 3.
struct SoftPair { float x; bool keep; int e; float t, qx, qy; };

template <bool GRAD>
__device__ __forceinline__ SoftPair softsil_pair(float px, float py, const float* __restrict__ f, float sg)
{
    float best = 0.0f, bt = 0.0f, bqx = 0.0f, bqy = 0.0f;
    int be = 0;
    bool allpos = true, allneg = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int n = (e + 1) % 3;
        const float ax = f[2 * e], ay = f[2 * e + 1];
        const float abx = f[2 * n] - ax, aby = f[2 * n + 1] - ay;
        const float apx = px - ax, apy = py - ay;
        float t = (apx * abx + apy * aby) / (abx * abx + aby * aby);
        t = fminf(fmaxf(t, 0.0f), 1.0f);
        const float qx = apx - t * abx, qy = apy - t * aby;
        const float d2 = qx * qx + qy * qy;
        const float cr = abx * apy - aby * apx;
        allpos = allpos && cr >= 0.0f;
        allneg = allneg && cr <= 0.0f;
        if (e == 0 || d2 < best) {
            best = d2;
            if (GRAD) { be = e; bt = t; bqx = qx; bqy = qy; }
        }
    }
    const bool inside = allpos || allneg;
    SoftPair r;
    r.keep = inside || best < SOFTSIL_CUT * sg;
    r.x = (inside ? best : -best) / sg;
    r.e = be; r.t = bt; r.qx = bqx; r.qy = bqy;
    return r;
}

// sigmoid(x) = 1 / (1 + exp(-x)); exp(-x) overflows to +inf for x < -88 and the quotient is then an exact 0
__device__ __forceinline__ float softsil_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

__device__ __forceinline__ float softsil_px(int c, int S) { return (float)(2 * c + 1 - S) / (float)S; }
__device__ __forceinline__ float softsil_py(int r, int S) { return (float)(S - 1 - 2 * r) / (float)S; }

__global__ __launch_bounds__(SOFTSIL_CHUNK) void k_softsil_fwd(const SoftFace* __restrict__ rec, const float* __restrict__ sigma,
                                                               float* __restrict__ alpha, long ntiles_all, int F, int S, int nt)
{
    __shared__ float s_tri[SOFTSIL_CHUNK][6];
    __shared__ int s_wcnt[SOFTSIL_CHUNK / HM_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float sg = sigma[0];
    for (long item = blockIdx.x; item < ntiles_all; item += gridDim.x) {        // (workgroup-uniform: barriers inside are safe)
        const long b = item / (nt * nt);
        const int tile = (int)(item - b * (nt * nt));
        const int tc0 = (tile % nt) * SOFTSIL_TILE, tr0 = (tile / nt) * SOFTSIL_TILE;
        const int c = tc0 + (tid & 15), r = tr0 + (tid >> 4);
        const float px = softsil_px(c, S), py = softsil_py(r, S);
        const SoftFace* fr = rec + b * F;
        float keep_prod = 1.0f;                                   // prod_j (1 - D_j), ascending face index
        for (int base = 0; base < F; base += SOFTSIL_CHUNK) {
            const int f = base + tid;
            bool hit = false;
            SoftFace me;
            if (f < F) {
                me = fr[f];
                hit = me.valid && me.c0 <= tc0 + SOFTSIL_TILE - 1 && me.c1 >= tc0 && me.r0 <= tr0 + SOFTSIL_TILE - 1 && me.r1 >= tr0;
            }
            const unsigned long long bal = __ballot(hit);
            if (lane == 0) s_wcnt[wave] = __popcll(bal);
            __syncthreads();
            int pos = __popcll(bal & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
            for (int w = 0; w < SOFTSIL_CHUNK / HM_WAVE; ++w) {
                const int cw = s_wcnt[w];
                pos += w < wave ? cw : 0;
                n += cw;
            }
            if (hit) {
                s_tri[pos][0] = me.x0; s_tri[pos][1] = me.y0; s_tri[pos][2] = me.x1;
                s_tri[pos][3] = me.y1; s_tri[pos][4] = me.x2; s_tri[pos][5] = me.y2;
            }
            __syncthreads();
            for (int j = 0; j < n; ++j) {                          // (every lane reads the same LDS words: broadcast)
                const SoftPair p = softsil_pair<false>(px, py, s_tri[j], sg);
                if (p.keep) keep_prod *= softsil_sigmoid(-p.x);    // 1 - D formed as sigmoid(-x), never as a subtraction
            }
            __syncthreads();                                       // s_tri / s_wcnt are rewritten by the next pass
        }
        if (c < S && r < S) alpha[(b * S + r) * S + c] = 1.0f - keep_prod;
    }
}

__global__ __launch_bounds__(256) void k_softsil_bwd(const SoftFace* __restrict__ rec, const float* __restrict__ sigma,
                                                     const float* __restrict__ alpha, const float* __restrict__ grad_alpha,
                                                     float* __restrict__ parts, long BF, int F, int S)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float sg = sigma[0];
    for (long i = (long)blockIdx.x * 4 + wave; i < BF; i += (long)gridDim.x * 4) {       // (wave-uniform)
        const SoftFace me = rec[i];
        float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (me.valid && me.c1 >= me.c0) {
            const long b = i / F;
            const float f6[6] = {me.x0, me.y0, me.x1, me.y1, me.x2, me.y2};
            const int w = me.c1 - me.c0 + 1, n = w * (me.r1 - me.r0 + 1);              // <= 4096^2
            const float* al = alpha + b * S * S;
            const float* ga = grad_alpha + b * S * S;
            for (int q = lane; q < n; q += HM_WAVE) {
                const int rr = q / w, r = me.r0 + rr, c = me.c0 + (q - rr * w);
                const SoftPair p = softsil_pair<true>(softsil_px(c, S), softsil_py(r, S), f6, sg);
                if (!p.keep) continue;
                const int at = r * S + c;
                // dL/dd2 = dL/dA (1 - A) D (+-1 / sigma);  d d2 / da = -2 (1 - t) q,  d d2 / db = -2 t q
                const float up = ga[at] * (1.0f - al[at]) * softsil_sigmoid(p.x) / sg;
                const float s2 = (p.x >= 0.0f ? -2.0f : 2.0f) * up;
                const float wa = s2 * (1.0f - p.t), wb = s2 * p.t;
                const int ea = p.e, eb = (p.e + 1) % 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {                      // (selects, not indexed registers)
                    const float wk = (k == ea ? wa : 0.0f) + (k == eb ? wb : 0.0f);
                    g[2 * k] += wk * p.qx;
                    g[2 * k + 1] += wk * p.qy;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = hm_wave_sum(g[k]);      // fixed DPP tree
        if (lane < 6) {
            float v = g[0];
#pragma unroll
            for (int k = 1; k < 6; ++k) v = lane == k ? g[k] : v;
            parts[i * 6 + lane] = v;
        }
    }
}

__global__ __launch_bounds__(256) void k_softsil_gather(const float* __restrict__ verts, const float* __restrict__ K,
                                                        const float* __restrict__ parts, const int* __restrict__ adj_off,
                                                        const int* __restrict__ adj_items, long BV, int V, int F,
                                                        float orig_size, float* __restrict__ grad_verts)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < BV; i += (long)gridDim.x * blockDim.x) {
        const long b = i / V;
        const int v = (int)(i - b * V);
        const int lo = max(adj_off[v], 0), hi = min(adj_off[v + 1], 3 * F);
        float gu = 0.0f, gv = 0.0f;
        for (int k = lo; k < hi; ++k) {                            // stored order
            const int it = adj_items[k];
            if (it < 0 || it >= 3 * F) continue;
            const float* p = parts + (b * F) * 6 + (long)it * 2;   // (face * 3 + corner) * 2
            gu += p[0];
            gv += p[1];
        }
        // u = 2 ((xn k0 + yn k1 + k2) - o / 2) / o,  v = 2 ((o - (xn k3 + yn k4 + k5)) - o / 2) / o,  xn = x / zz, yn = y / zz
        const float* k9 = K + b * 9;
        const float* p = verts + i * 3;
        const float zz = p[2] + 1e-9f;
        const float s = 2.0f / orig_size;
        const float gxn = s * (gu * k9[0] - gv * k9[3]), gyn = s * (gu * k9[1] - gv * k9[4]);
        float* o = grad_verts + i * 3;
        o[0] = gxn / zz;
        o[1] = gyn / zz;
        o[2] = -(gxn * p[0] + gyn * p[1]) / (zz * zz);
    }
}

static bool softsil_shape_ok(int B, int V, int F, int S) { return B >= 1 && V >= 1 && F >= 1 && S >= 1 && S <= 4096; }

static int softsil_blocks(long n) { return (int)(n < SOFTSIL_MAX_BLOCKS ? n : SOFTSIL_MAX_BLOCKS); }

extern "C" size_t hm_softsil_workspace_bytes(int B, int V, int F, int S)
{
    if (!softsil_shape_ok(B, V, F, S)) return 0;
    return softsil_parts_offset(B, F) + (size_t)B * F * 6 * sizeof(float);
}

extern "C" int hm_softsil_fwd(const float* verts, const int* faces, const float* K, int B, int V, int F, int S, float orig_size,
                              float znear, float zfar, const float* sigma, float* alpha, void* workspace, hipStream_t stream)
{
    HM_CHECK_ARG(verts && faces && K && sigma && alpha && workspace);
    HM_CHECK_ARG(HM_ALIGNED(workspace, 4));          // face records and partial sums of 4-byte members
    HM_CHECK_ARG(softsil_shape_ok(B, V, F, S) && orig_size > 0.0f && znear < zfar);
    SoftFace* rec = (SoftFace*)workspace;
    const long BF = (long)B * F;
    const int nt = hm_cdiv(S, SOFTSIL_TILE);
    const long tiles = (long)B * nt * nt;
    hipLaunchKernelGGL(k_softsil_setup, dim3(softsil_blocks(hm_cdiv(BF, 256))), dim3(256), 0, stream, verts, faces, K, BF, V, F, S,
                       orig_size, znear, zfar, sigma, rec);
    hipLaunchKernelGGL(k_softsil_fwd, dim3(softsil_blocks(tiles)), dim3(SOFTSIL_CHUNK), 0, stream, (const SoftFace*)rec, sigma,
                       alpha, tiles, F, S, nt);
    return hm_launch_status();
}

extern "C" int hm_softsil_bwd(const float* verts, const int* faces, const float* K, int B, int V, int F, int S, float orig_size,
                              float znear, float zfar, const float* sigma, const float* alpha, const float* grad_alpha,
                              const int* adj_off, const int* adj_items, float* grad_verts, void* workspace, hipStream_t stream)
{
    HM_CHECK_ARG(verts && faces && K && sigma && alpha && grad_alpha && adj_off && adj_items && grad_verts && workspace);
    HM_CHECK_ARG(HM_ALIGNED(workspace, 4));          // face records and partial sums of 4-byte members
    HM_CHECK_ARG(softsil_shape_ok(B, V, F, S) && orig_size > 0.0f && znear < zfar);
    SoftFace* rec = (SoftFace*)workspace;
    float* parts = (float*)((char*)workspace + softsil_parts_offset(B, F));
    const long BF = (long)B * F, BV = (long)B * V;
    // the records are formed again from the arguments: the backward does not depend on what ran on the workspace in between
    hipLaunchKernelGGL(k_softsil_setup, dim3(softsil_blocks(hm_cdiv(BF, 256))), dim3(256), 0, stream, verts, faces, K, BF, V, F, S,
                       orig_size, znear, zfar, sigma, rec);
    hipLaunchKernelGGL(k_softsil_bwd, dim3(softsil_blocks(hm_cdiv(BF, 4))), dim3(256), 0, stream, (const SoftFace*)rec, sigma, alpha,
                       grad_alpha, parts, BF, F, S);
    hipLaunchKernelGGL(k_softsil_gather, dim3(softsil_blocks(hm_cdiv(BV, 256))), dim3(256), 0, stream, verts, K, (const float*)parts,
                       adj_off, adj_items, BV, V, F, orig_size, grad_verts);
    return hm_launch_status();
}
