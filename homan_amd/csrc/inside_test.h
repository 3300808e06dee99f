// inside_test.h -- the +x ray / triangle crossing rule of the inside-outside decisions, shared by the SDF sign pass (sdf.hip)
// and the solid voxeliser (solidvox.hip).  Conventions identical to oracle/csrc/sdf.c: every operation is fp32 IEEE (the
// build compiles with -ffp-contract=off), and a ray through an edge or a vertex of the projected triangle is given to
// exactly one of the triangles that share it by the half-open orientation rule of orient2.
#pragma once
#include "hm_common.h"

__device__ __forceinline__ int orient2(float x1, float y1, float x2, float y2, float* tsa)
{
    *tsa = y1 * x2 - x1 * y2;
    if (*tsa > 0.0f) return 1;
    if (*tsa < 0.0f) return -1;
    if (y2 > y1) return 1;
    if (y2 < y1) return -1;
    if (x1 > x2) return 1;
    if (x1 < x2) return -1;
    return 0;
}

// does the ray from (-inf, cy, cz) along +x cross the triangle (v1, v2, v3)?  *xhit = x of the crossing
__device__ __forceinline__ bool ray_x_crosses(float cy, float cz, const float* v1, const float* v2, const float* v3,
                                              float* xhit)
{
    const float y1 = v1[1] - cy, z1 = v1[2] - cz, y2 = v2[1] - cy, z2 = v2[2] - cz, y3 = v3[1] - cy, z3 = v3[2] - cz;
    float a, b, g;
    const int sa = orient2(y2, z2, y3, z3, &a);
    if (sa == 0) return false;
    const int sb = orient2(y3, z3, y1, z1, &b);
    if (sb != sa) return false;
    const int sc = orient2(y1, z1, y2, z2, &g);
    if (sc != sa) return false;
    const float sum = a + b + g;
    if (sum == 0.0f) return false;
    const float fa = a / sum, fb = b / sum, fc = g / sum;
    *xhit = fa * v1[0] + fb * v2[0] + fc * v3[0];
    return true;
}
