// sr_moments.hpp — what the moment epilogues of sr_scale.hip and sr_genes.hip share: the fixed-order float64 wave sum, the float32 wave
// minimum / maximum, and the one-workgroup label statistics (ybar, Syy) both read, bit for bit the same.
#pragma once
#include "evogp_defs.hpp"

namespace evogp {

constexpr int kStatsThreads = 256;

template <int CTRL, int ROW_MASK>
__device__ inline double dpp_move_d(double v) {
    const int lo = dpp_move<CTRL, ROW_MASK>(0, __double2loint(v));
    const int hi = dpp_move<CTRL, ROW_MASK>(0, __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// wave_sum (evogp_defs.hpp) on a double: the same fixed association
__device__ inline double wave_sum_d(double x) {
    double v = x;
    v += dpp_move_d<kDppRowShr | 1, 0xf>(v);
    v += dpp_move_d<kDppRowShr | 2, 0xf>(v);
    v += dpp_move_d<kDppRowShr | 4, 0xf>(v);
    v += dpp_move_d<kDppRowShr | 8, 0xf>(v);
    v += dpp_move_d<kDppBcast15, 0xa>(v);
    v += dpp_move_d<kDppBcast31, 0xc>(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

__device__ inline float wave_min_f(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline float wave_max_f(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- label statistics: one workgroup, thread i takes rows i, i + 256, ...; lanes by the butterfly, waves in order ---------------------
// (static: every translation unit that launches it carries its own copy)
static __global__ __launch_bounds__(kStatsThreads) void label_stats_kernel(const float *y, int D, double *stats) {
    __shared__ double s_w[kStatsThreads / kWave];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    auto block_sum = [&](double x) {
        const double s = wave_sum_d(x);
        __syncthreads();   // (the previous round's reads are over)
        if (lane == 0) s_w[w] = s;
        __syncthreads();
        double total = 0.0;
        for (int k = 0; k < kStatsThreads / kWave; ++k) total += s_w[k];
        return total;
    };
    double s = 0.0;
    for (int i = threadIdx.x; i < D; i += kStatsThreads) s += (double)y[i];
    const double ybar = block_sum(s) / (double)D;
    double q = 0.0;
    for (int i = threadIdx.x; i < D; i += kStatsThreads) {
        const double v = (double)y[i] - ybar;
        q += v * v;
    }
    const double syy = block_sum(q);
    if (threadIdx.x == 0) { stats[0] = ybar; stats[1] = syy; }
}

}  // namespace evogp
