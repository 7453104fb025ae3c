// The camera rotation of the 'matrix_6dof_rotation' parametrisation, shared by pose.hip (the per-ray camera transform) and map.hip (the map export's
// unprojection).  Include inside a translation unit compiled with -ffp-contract=off: the products and sums below are in the tensor-op form's order.
#pragma once
#include "common.h"

namespace {

struct Rot {
    float b[3][3];        // rows b1, b2, b3
    float n1, n2, s;      // |a1|, |a2 - s b1|, s = b1 . a2
};

__device__ __forceinline__ float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// rotation_6d_to_matrix of pagnerf_amd/ba_pipeline.py (Gram-Schmidt, Zhou et al. 2019)
__device__ __forceinline__ Rot rotation(const float *p) {
    Rot r;
    r.n1 = __fsqrt_rn(dot3(p, p));
#pragma unroll
    for (int j = 0; j < 3; ++j) r.b[0][j] = p[j] / r.n1;
    r.s = dot3(r.b[0], p + 3);
    float q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = p[3 + j] - r.s * r.b[0][j];
    r.n2 = __fsqrt_rn(dot3(q, q));
#pragma unroll
    for (int j = 0; j < 3; ++j) r.b[1][j] = q[j] / r.n2;
    cross3(r.b[0], r.b[1], r.b[2]);
    return r;
}

}  // namespace
