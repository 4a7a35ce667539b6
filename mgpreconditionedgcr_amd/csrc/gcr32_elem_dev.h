// The element-wise expressions of the low-precision GCR's iteration (device side): the ONE copy that the single solve (gcr32.hip)
// and the k-wide lockstep solve (gcr32_multi.hip) both call, so a column of a block is built, updated and summed exactly as a
// single Field is.  Nothing is fused; every dot-product operand is converted to double first.
#pragma once
#include "gcr32_state.h"

namespace mgcr {

__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double norm2d(float re, float im) { return (double)re * (double)re + (double)im * (double)im; }

// <Ap_j, Ar> += conj(a) y, a = Ap_j's element, y = Ar's
__device__ __forceinline__ void g32_beta_dot(float axf, float ayf, double yx, double yy, double &re, double &im) {
    const double ax = (double)axf, ay = (double)ayf;
    re += ax * yx + ay * yy;
    im += ax * yy - ay * yx;
}

// beta_j = <Ap_j, Ar> / <Ap_j, Ap_j>, j < ND, from the apply's partial slab: folded 8 directions at a time, formed in fp64, rounded once
// and left in LDS (beta[2 j], beta[2 j + 1]; the caller's barrier publishes them): held in registers, 2 ND of them and the 2 ND + 2 lane
// addresses of an unrolled direction loop do not fit 64 VGPRs from 2 directions on
template <int ND, int J0 = 0>
__device__ __forceinline__ void fold_betas(const double *__restrict__ partsB, int nblk, const double *__restrict__ den, float *beta, double *lds) {
    constexpr int C = ND - J0 < 8 ? ND - J0 : 8;
    double v[2 * C];
    fold_partials<2 * C>(partsB + (size_t)2 * J0 * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, v, lds);
#pragma unroll
    for (int j = 0; j < C; j++) {
        const double d = den[J0 + j];
        if (threadIdx.x == 0) {
            beta[2 * (J0 + j)] = (float)(v[2 * j] / d);
            beta[2 * (J0 + j) + 1] = (float)(v[2 * j + 1] / d);
        }
    }
    if constexpr (J0 + C < ND) fold_betas<ND, J0 + C>(partsB, nblk, den, beta, lds);
}

// o -= beta v, un-fused
__device__ __forceinline__ void g32_sub_scaled(float bx, float by, float vx, float vy, float &ox, float &oy) {
    ox -= bx * vx - by * vy;
    oy -= bx * vy + by * vx;
}
__device__ __forceinline__ void g32_build_dots(float qx, float qy, float rx, float ry, double (&acc)[3]) {
    const double dqx = (double)qx, dqy = (double)qy, drx = (double)rx, dry = (double)ry;
    acc[0] += dqx * dqx + dqy * dqy;
    acc[1] += dqx * drx + dqy * dry;
    acc[2] += dqx * dry - dqy * drx;
}

// x += alpha p, r -= alpha Ap, |r|^2
__device__ __forceinline__ void g32_update_one(float ax, float ay, float px, float py, float qx, float qy, float &xx, float &xy, float &rx, float &ry,
                                               double &acc) {
    xx += ax * px - ay * py;
    xy += ax * py + ay * px;
    rx -= ax * qx - ay * qy;
    ry -= ax * qy + ay * qx;
    acc += norm2d(rx, ry);
}

}  // namespace mgcr
