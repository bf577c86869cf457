// sr_moments.hpp — what the moment epilogues of sr_scale.hip and sr_genes.hip share: the fixed-order float64 wave sum, the float32 wave
// minimum / maximum, and the one-workgroup label statistics (ybar, Syy) both read, bit for bit the same; and what the weighted passes
// (sr_wloss.hip, the weighted builds of sr_grad.hip and sr_lm.hip) share: the one-workgroup weight statistics and rho.
#pragma once
#include <math.h>

#include "../../include/evogp_hip.h"
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

// ---- weight rows and rho: what the weighted passes share (sr_wloss.hip, and the weighted builds of sr_grad.hip and sr_lm.hip) ------------
struct WeightStat {   // one 16-byte slot of acquire_counter per weight row
    double sum;
    unsigned usable;  // != 0: no negative or non-finite weight and sum != 0
    unsigned pad;
};

// rho in float64; r = (double)p - (double)y.  `kind` is wave-uniform.  LC: the log-cosh build.  The float64 exp and log1p take registers
// the LEAN interpreter does not have (164 B of scratch per lane against 8 at KW = 2), so the other four kinds do not carry them
template <bool LC>
__device__ inline double wloss_rho(int kind, double prm, double r) {
    const double a = fabs(r);
    if (LC) return a + log1p(exp(-2.0 * a)) - M_LN2;   // log cosh r, no overflow
    switch (kind) {
    case EVOGP_LOSS_MSE: return r * r;
    case EVOGP_LOSS_MAE: return a;
    case EVOGP_LOSS_HUBER: return a <= prm ? r * r * 0.5 : prm * (a - prm * 0.5);
    default: {
        const double ry = -r;   // y - p
        return ry >= 0.0 ? prm * ry : (prm - 1.0) * ry;
    }
    }
}

// d rho / d r, the seed of the weighted reverse walk (sr_grad.hip); 0 at the kinks r = 0 of mae and pinball
template <bool LC>
__device__ inline double wloss_drho(int kind, double prm, double r) {
    if (LC) return tanh(r);
    switch (kind) {
    case EVOGP_LOSS_MSE: return 2.0 * r;
    case EVOGP_LOSS_MAE: return r > 0.0 ? 1.0 : r < 0.0 ? -1.0 : 0.0;
    case EVOGP_LOSS_HUBER: return fabs(r) <= prm ? r : (r > 0.0 ? prm : -prm);
    default: return r < 0.0 ? -prm : r > 0.0 ? 1.0 - prm : 0.0;
    }
}

// ---- weight statistics: one workgroup, thread i takes rows i, i + 256, ...; lanes by the butterfly, waves in order ----------------------
// (static, as label_stats_kernel)
struct WeightStatOut { WeightStat *slot[EVOGP_WLOSS_MAX_WEIGHTS]; };

static __global__ __launch_bounds__(kStatsThreads) void weight_stats_kernel(const float *W, int D, int nw, WeightStatOut out) {
    __shared__ double s_w[kStatsThreads / kWave];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = 0; k < nw; ++k) {
        const float *row = W + (size_t)k * D;
        double s = 0.0;
        int bad = 0;
        for (int i = threadIdx.x; i < D; i += kStatsThreads) {
            const float x = row[i];
            bad |= !finite_f(x) || x < 0.0f;
            s += (double)x;
        }
        const double ws = wave_sum_d(s);
        const int any_bad = __syncthreads_or(bad);   // (also: the previous round's reads of s_w are over)
        if (lane == 0) s_w[w] = ws;
        __syncthreads();
        if (threadIdx.x == 0) {
            double total = 0.0;
            for (int i = 0; i < kStatsThreads / kWave; ++i) total += s_w[i];
            out.slot[k]->sum = total;
            out.slot[k]->usable = !any_bad && total != 0.0 ? 1u : 0u;
        }
    }
}

}  // namespace evogp
