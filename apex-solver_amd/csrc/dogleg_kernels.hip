// dogleg_kernels.hip -- the Dog-Leg step on plain vectors (dogleg_kernels.h):
//   k_dl_dots     the inner products of the scaled gradient and the scaled Gauss-Newton step, D^2 g and the cached step on the way
//   k_dl_combine  one lane: dogleg_combine.hpp on the six sums and the radius
//   k_dl_blend    the blended step into the step vector, |step|^2
// HBM-bound and tiny next to the factorisation: three reads and two writes per entry for the dots, three and one for the blend.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "device_reduce.hpp"
#include "dogleg_combine.hpp"
#include "dogleg_kernels.h"

namespace apex {

// The inner products of the scaled gradient g_s = D g and the scaled Gauss-Newton step y = D^-1 d (d: the unscaled step the
// sweeps leave): partial = {g_s.g_s, y.y, g_s.y}.  On the way: a_out = D g_s (the direction the Gram pass prices g_s with; may be
// null without scaling, where it is g itself) and h_out = d (the cached step: d is overwritten by the blended step).
__global__ __launch_bounds__(256) void k_dl_dots(int64_t n, const double* __restrict__ g, const double* __restrict__ d,
                                                   const double* __restrict__ scale, double* __restrict__ a_out,
                                                   double* __restrict__ h_out, double* __restrict__ partial) {
    __shared__ double scratch[4];
    double gg = 0.0, hh = 0.0, gh = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double s = scale ? scale[i] : 1.0, di = d[i];
        const double gs = g[i] * s, y = scale ? di / s : di;
        gg += gs * gs; hh += y * y; gh += gs * y;
        if (a_out) a_out[i] = gs * s;
        h_out[i] = di;
    }
    gg = block_sum_256(gg, scratch);
    hh = block_sum_256(hh, scratch);
    gh = block_sum_256(gh, scratch);
    if (threadIdx.x == 0) { partial[3 * blockIdx.x] = gg; partial[3 * blockIdx.x + 1] = hh; partial[3 * blockIdx.x + 2] = gh; }
}

// one lane: the six sums and the radius -> {alpha, beta, c_g, c_h, |step_s|, predicted reduction, type}
__global__ void k_dl_combine(const double* __restrict__ sums6, double delta, double* __restrict__ out7) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const DoglegSums s{sums6[0], sums6[1], sums6[2], sums6[3], sums6[4], sums6[5]};
    const DoglegStep o = dogleg_combine(s, delta);
    out7[0] = o.alpha; out7[1] = o.beta; out7[2] = o.c_g; out7[3] = o.c_h; out7[4] = o.step_norm; out7[5] = o.predicted_reduction;
    out7[6] = (double)o.type;
}

// step = D (c_g (-g_s) + c_h y) = c_h h - c_g D^2 g into d_out, and the partial sums of |step|^2.  coef = {c_g, c_h} on the device.
__global__ __launch_bounds__(256) void k_dl_blend(int64_t n, const double* __restrict__ g, const double* __restrict__ scale,
                                                    const double* __restrict__ h, const double* __restrict__ coef,
                                                    double* __restrict__ d_out, double* __restrict__ partial) {
    __shared__ double scratch[4];
    const double cg = coef[0], ch = coef[1];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double s = scale ? scale[i] : 1.0;
        const double st = ch * h[i] - cg * ((g[i] * s) * s);
        d_out[i] = st;
        acc += st * st;
    }
    acc = block_sum_256(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ---- launchers -----------------------------------------------------------------------------------------------------
void launch_dl_dots(const DlSegment* segs, int n_seg, double* partial, int n_partial, double* out3, hipStream_t s) {
    const int per = n_partial / n_seg;
    for (int k = 0; k < n_seg; ++k)
        hipLaunchKernelGGL(k_dl_dots, dim3(per), dim3(256), 0, s, segs[k].n, segs[k].g, segs[k].d, segs[k].scale, segs[k].a, segs[k].h,
                           partial + 3 * (size_t)k * per);
    launch_sum_partials(partial, n_seg * per, 3, out3, s);
}
void launch_dl_combine(const double* sums6, double delta, double* out7, hipStream_t s) {
    hipLaunchKernelGGL(k_dl_combine, dim3(1), dim3(64), 0, s, sums6, delta, out7);
}
void launch_dl_blend(const DlSegment* segs, int n_seg, const double* coef, double* partial, int n_partial, double* out_sumsq,
                     hipStream_t s) {
    const int per = n_partial / n_seg;
    for (int k = 0; k < n_seg; ++k)
        hipLaunchKernelGGL(k_dl_blend, dim3(per), dim3(256), 0, s, segs[k].n, segs[k].g, segs[k].scale, segs[k].h, coef, segs[k].d,
                           partial + (size_t)k * per);
    launch_sum_partials(partial, n_seg * per, 1, out_sumsq, s);
}

}  // namespace apex
