// surfdist_walk.h -- the per-face part of the exact point-to-mesh distance: the face record, Ericson's region walk and the three
// segments of a degenerate face.  Shared by csrc/surfdist.hip (the search) and csrc/surfcontact.hip (the contact terms), so that
// both compute q and D by the same operations in the same order (include/homan_amd.h, tests/surfmetrics_ref.py).  The walk is
// one function, sd_closest_w: with WEIGHTS it also yields the barycentric weights of q on (a, b, c); without, those stores do
// not exist and the function is the distance alone.  Every operation is fp32 IEEE without contraction.
#pragma once
#include "hm_common.h"

// launch geometry of the kernels that walk every (point, face) pair: csrc/surfdist.hip and csrc/winding.hip
#define SD_THREADS 256
#define SD_CHUNK 256                     // faces staged per pass: one record per thread (ops.SURFDIST_CHUNK mirrors it)
#define SD_MAX_GRID_Z 65535
#define SD_TARGET_BLOCKS 1024            // four workgroups on each of the 256 CUs before the faces stop being split

#define SD_SKIPPED 0
#define SD_TRIANGLE 1
#define SD_SEGMENTS 2

struct SdFace { float a[3], b[3], c[3], ab[3], ac[3]; int kind; };      // 16 words: four b128 LDS reads

__device__ __forceinline__ float sd_dot(const float* u, const float* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ __forceinline__ bool sd_finite(float x) { return fabsf(x) <= 3.4028234e38f; }       // (a NaN fails)

// face f of the frame's mesh as a record; SD_SKIPPED when it names a vertex outside [0, V) or holds a non-finite coordinate
__device__ __forceinline__ void sd_load_face(const float* __restrict__ v, const int* __restrict__ faces, long f, int V,
                                             SdFace& r)
{
    const int* t = faces + 3 * f;
    const int i0 = t[0], i1 = t[1], i2 = t[2];
    r.kind = SD_SKIPPED;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.a[k] = r.b[k] = r.c[k] = r.ab[k] = r.ac[k] = 0.f;
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.a[k] = v[3L * i0 + k]; r.b[k] = v[3L * i1 + k]; r.c[k] = v[3L * i2 + k];
        ok = ok && sd_finite(r.a[k]) && sd_finite(r.b[k]) && sd_finite(r.c[k]);
        r.ab[k] = r.b[k] - r.a[k];
        r.ac[k] = r.c[k] - r.a[k];
    }
    if (!ok) return;
    const float nx = r.ab[1] * r.ac[2] - r.ab[2] * r.ac[1];
    const float ny = r.ab[2] * r.ac[0] - r.ab[0] * r.ac[2];
    const float nz = r.ab[0] * r.ac[1] - r.ab[1] * r.ac[0];
    r.kind = (nx == 0.f && ny == 0.f && nz == 0.f) ? SD_SEGMENTS : SD_TRIANGLE;
}

// clamped projection of p on the segment u -> v: q, |p - q|^2 and the parameter t (q = u + t (v - u))
__device__ __forceinline__ float sd_segment(const float* p, const float* u, const float* v, float* q, float* t_out)
{
    const float e[3] = {v[0] - u[0], v[1] - u[1], v[2] - u[2]};
    const float w[3] = {p[0] - u[0], p[1] - u[1], p[2] - u[2]};
    const float len2 = sd_dot(e, e);
    float t = 0.f;
    if (len2 > 0.f) {
        t = sd_dot(w, e) / len2;
        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
    }
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { q[k] = u[k] + t * e[k]; d[k] = p[k] - q[k]; }
    *t_out = t;
    return sd_dot(d, d);
}

// closest point q of the face to p, D = |p - q|^2 (kind != SD_SKIPPED) and, with WEIGHTS, the barycentric weights w of q on
// (a, b, c): a corner gives a unit weight, an edge u -> v gives (1 - t, t) on its ends, the interior (1 - tv - tw, tv, tw)
// formed as (1 - tv) - tw; a degenerate face gives the winning segment's (1 - t, t) on that segment's two ends (ab, bc, ca: the
// segment ca runs from c to a) and 0 on the third.  dv = p - q as D was formed from it.
template <bool WEIGHTS>
__device__ __forceinline__ float sd_closest_w(const float* p, const SdFace& r, float* q, float* w, float* dv)
{
    if (r.kind == SD_SEGMENTS) {                                  // ab, bc, ca; ties to the first
        float t, t2, q2[3];
        float D = sd_segment(p, r.a, r.b, q, &t);
        if (WEIGHTS) { w[0] = 1.f - t; w[1] = t; w[2] = 0.f; }
        float D2 = sd_segment(p, r.b, r.c, q2, &t2);
        if (D2 < D) {
            D = D2; q[0] = q2[0]; q[1] = q2[1]; q[2] = q2[2];
            if (WEIGHTS) { w[0] = 0.f; w[1] = 1.f - t2; w[2] = t2; }
        }
        D2 = sd_segment(p, r.c, r.a, q2, &t2);
        if (D2 < D) {
            D = D2; q[0] = q2[0]; q[1] = q2[1]; q[2] = q2[2];
            if (WEIGHTS) { w[0] = t2; w[1] = 0.f; w[2] = 1.f - t2; }
        }
        if (WEIGHTS) { dv[0] = p[0] - q[0]; dv[1] = p[1] - q[1]; dv[2] = p[2] - q[2]; }
        return D;
    }
    const float ap[3] = {p[0] - r.a[0], p[1] - r.a[1], p[2] - r.a[2]};
    const float bp[3] = {p[0] - r.b[0], p[1] - r.b[1], p[2] - r.b[2]};
    const float cp[3] = {p[0] - r.c[0], p[1] - r.c[1], p[2] - r.c[2]};
    const float d1 = sd_dot(r.ab, ap), d2 = sd_dot(r.ac, ap), d3 = sd_dot(r.ab, bp), d4 = sd_dot(r.ac, bp);
    const float d5 = sd_dot(r.ab, cp), d6 = sd_dot(r.ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e1 = d4 - d3, e2 = d5 - d6;
    if (d1 <= 0.f && d2 <= 0.f) {                                  // A
        q[0] = r.a[0]; q[1] = r.a[1]; q[2] = r.a[2];
        if (WEIGHTS) { w[0] = 1.f; w[1] = 0.f; w[2] = 0.f; }
    } else if (d3 >= 0.f && d4 <= d3) {                            // B
        q[0] = r.b[0]; q[1] = r.b[1]; q[2] = r.b[2];
        if (WEIGHTS) { w[0] = 0.f; w[1] = 1.f; w[2] = 0.f; }
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {              // AB
        const float t = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = r.a[k] + t * r.ab[k];
        if (WEIGHTS) { w[0] = 1.f - t; w[1] = t; w[2] = 0.f; }
    } else if (d6 >= 0.f && d5 <= d6) {                            // C
        q[0] = r.c[0]; q[1] = r.c[1]; q[2] = r.c[2];
        if (WEIGHTS) { w[0] = 0.f; w[1] = 0.f; w[2] = 1.f; }
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {              // AC
        const float t = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = r.a[k] + t * r.ac[k];
        if (WEIGHTS) { w[0] = 1.f - t; w[1] = 0.f; w[2] = t; }
    } else if (va <= 0.f && e1 >= 0.f && e2 >= 0.f) {              // BC
        const float t = e1 / (e1 + e2);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = r.b[k] + t * (r.c[k] - r.b[k]);
        if (WEIGHTS) { w[0] = 0.f; w[1] = 1.f - t; w[2] = t; }
    } else {                                                       // interior
        const float s = (va + vb) + vc;
        const float tv = vb / s, tw = vc / s;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (r.a[k] + tv * r.ab[k]) + tw * r.ac[k];
        if (WEIGHTS) { w[0] = (1.f - tv) - tw; w[1] = tv; w[2] = tw; }
    }
    const float d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    if (WEIGHTS) { dv[0] = d[0]; dv[1] = d[1]; dv[2] = d[2]; }
    return sd_dot(d, d);
}

// the distance alone: q and D, the bits of hm_point_mesh_distance
__device__ __forceinline__ float sd_closest(const float* p, const SdFace& r, float* q)
{
    return sd_closest_w<false>(p, r, q, nullptr, nullptr);
}

// how many workgroups share the faces of one frame, and how many chunks each takes
static inline int sd_splits(int B, int N, int F, int* chunks_per_split)
{
    const long chunks = ((long)F + SD_CHUNK - 1) / SD_CHUNK;
    const long blocks = (long)B * (((long)N + SD_THREADS - 1) / SD_THREADS);
    long want = (SD_TARGET_BLOCKS + blocks - 1) / blocks;
    want = want < 1 ? 1 : (want > chunks ? chunks : want);
    const long per = (chunks + want - 1) / want;
    *chunks_per_split = (int)per;
    return (int)((chunks + per - 1) / per);
}
