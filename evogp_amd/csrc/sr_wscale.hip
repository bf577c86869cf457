// sr_wscale.hip — linear scaling under sample weights with held-out scoring, in one pass over the dataset (gfx950; no counterpart in
// the reference).
//
// evogp_hip_sr_weighted_scaling (include/evogp_hip.h has the contract).  Weight row 0 is the FIT row: a + b * T(x) is fitted on it in
// closed form; every row k is then SCORED with those coefficients.  Per tree and weight row k three float64 sums over the float32
// predictions p_d, taken over the rows with W[k, d] != 0 (v_d = (double)y_d - ybar0, ybar0 the row-0 weighted mean of the labels):
//     Swp_k = sum w p      Swpp_k = sum w p^2      Swpv_k = sum w p v
// plus, for row 0 alone, min p, max p in float32, and per row "some such prediction is not finite".  The closed form needs nothing
// else, so the (pop, D) predictions are never stored, and a row a column gives no weight to is not looked at in that column.  The
// launches, all on the caller's stream, nothing synchronises with the host:
//   1. wscale_stats_kernel  ONE workgroup: ybar0, and per weight row W_k = sum w (weight_stats_kernel's order, sr_moments.hpp, hence its
//                           bits), whether the row may be used, how many rows it weights, vbar_k = sum w v / W_k and
//                           V_k = sum w (v - vbar_k)^2, in a fixed order; all of it stays on the device.  Launched without weights too
//                           (every weight 1): the labels' statistics are needed either way.
//   2. sr_wscale_kernel     sr_wloss_kernel's decomposition (sr_wloss.hip: the register interpreter, LEAN then FULL over the
//                           kSentinelHeavy marks, batches from a counter, the `single` path, the weights of a wave's tile parked in LDS)
//                           with the moment epilogue above.  Built for KW = 0 (no weights: the weight is 1, nothing is loaded), 2 and 8
//                           columns of three float64 accumulators per lane.  Every build cuts the rows the same way (4 per lane, tiles
//                           of 256 per wave), so which build runs a column changes nothing in it; the 8-column build holds fewer trees
//                           per batch (LDS) and is held to two resident waves per SIMD (48 accumulator registers).
//   3. sr_wscale_general_kernel   a wave per tree with the operand stack in scratch memory (run_general) for the trees too deep for the
//                           registers and for every tree of a forest with var_len > 32, as sr_wloss_general_kernel.
// Sums keep sr_scale_kernel's order: a lane's tiles ascending, the 64 lanes by wave_sum_d, the waves in wave order by one thread per
// tree, which also evaluates the closed form and stores the tree's results in ONE place.  The sums are uncentred (sr_scale.hip's
// scheme): every term is a product of the weight, so a weight row multiplied by a power of two multiplies every sum of its column
// exactly, and the closed form is homogeneous of degree 0 in each row -- no bit of the result moves.
#include <math.h>

#include "interp.hpp"
#include "launch.hpp"
#include "sr_moments.hpp"
#include "sr_params.hpp"

namespace evogp {

constexpr int kWscaleK = 4;        // rows per lane, the same in every build (the order of the sums must not depend on the build)
constexpr int kWscaleDepth = 16;   // register stack entries; deeper trees go to the scratch stack
constexpr int kWscaleWaves = 4;    // waves per workgroup: a workgroup's row tile is 64 * kWscaleK * kWscaleWaves = 1024 rows
static_assert(EVOGP_WLOSS_MAX_WEIGHTS == 8, "the accumulator widths end at 8");
// trees per batch: the LDS partial-sum slots (three doubles per tree, wave and column, double-buffered)
constexpr int wscale_batch(int KW) { return KW == 8 ? kMaxBatch / 4 : kMaxBatch; }
// resident waves per SIMD of the LEAN build: sr_scale.hip's three, two at 8 columns (48 accumulator registers per lane)
constexpr int wscale_lean_waves(int KW) { return KW == 8 ? 2 : 3; }

// per weight row, two 16-byte slots of acquire_counter
struct WscaleSum {
    double wsum;      // W_k
    unsigned usable;  // != 0: no negative or non-finite weight and W_k != 0
    unsigned rows;    // 1: exactly one row has weight; 2: more than one (0 for an all-zero row)
};
struct WscaleLab {
    double vbar;      // sum w v / W_k
    double V;         // sum w (v - vbar)^2
};
struct WscaleStats {
    double *ybar;     // the row-0 weighted mean of the labels (a slot of its own)
    WscaleSum *sum[EVOGP_WLOSS_MAX_WEIGHTS];
    WscaleLab *lab[EVOGP_WLOSS_MAX_WEIGHTS];
};

struct WscaleParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;        // [D][var_len]
    const float *y;        // [D]
    const float *W;        // [nw][D], or nullptr: one column of weights 1
    float *loss;           // [pop][nw]; column 0 carries the kSentinel marks between the passes
    float *coef;           // [pop][2]: intercept, slope
    WscaleStats st;        // (wscale_stats_kernel)
    unsigned *counter;     // as ScaleParams::counter
    int pop, D, gp_len, var_len, nw, batch, ntiles;
};

// ---- 1. label and weight statistics: one workgroup, thread i takes rows i, i + 256, ...; lanes by the butterfly, waves in order -------
static __global__ __launch_bounds__(kStatsThreads) void wscale_stats_kernel(const float *y, const float *W, int D, int nw, WscaleStats out) {
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
    // ybar0 = sum W[0, d] y_d / W_0
    double s = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < D; i += kStatsThreads) {
        const float x = W ? W[i] : 1.0f;
        s += (double)x;
        sy += x != 0.0f ? (double)x * (double)y[i] : 0.0;
    }
    const double w0 = block_sum(s);
    const double ybar = block_sum(sy) / w0;
    if (threadIdx.x == 0) *out.ybar = ybar;
    for (int k = 0; k < nw; ++k) {
        const float *row = W ? W + (size_t)k * D : nullptr;
        double sw = 0.0, sv = 0.0, cnt = 0.0;
        int bad = 0;
        for (int i = threadIdx.x; i < D; i += kStatsThreads) {
            const float x = row ? row[i] : 1.0f;
            bad |= !finite_f(x) || x < 0.0f;
            sw += (double)x;
            const bool on = x != 0.0f;
            cnt += on ? 1.0 : 0.0;
            sv += on ? (double)x * ((double)y[i] - ybar) : 0.0;
        }
        const int any_bad = __syncthreads_or(bad);
        const double wk = block_sum(sw);
        const double rows = block_sum(cnt);
        const double vbar = block_sum(sv) / wk;
        double q = 0.0;
        for (int i = threadIdx.x; i < D; i += kStatsThreads) {
            const float x = row ? row[i] : 1.0f;
            const double r = (double)y[i] - ybar - vbar;
            q += x != 0.0f ? (double)x * (r * r) : 0.0;
        }
        const double V = block_sum(q);
        if (threadIdx.x == 0) {
            out.sum[k]->wsum = wk;
            out.sum[k]->usable = !any_bad && wk != 0.0 ? 1u : 0u;
            out.sum[k]->rows = rows == 1.0 ? 1u : rows > 1.0 ? 2u : 0u;
            out.lab[k]->vbar = vbar;
            out.lab[k]->V = V;
        }
    }
}

// ---- the closed form (one thread per tree) ---------------------------------------------------------------------------------------------
struct WscaleFit {
    double b, m0, vbar0, c0;
    bool nan;    // everything is NaN: column 0 may not be used or met a non-finite prediction, or a coefficient is not finite as float32
};

// the fit on column 0: af, bf are the rounded coefficients (NaN with fit.nan)
__device__ inline WscaleFit wscale_fit(const WscaleParams &p, double swp, double swpp, double swpv, float mn, float mx, bool bad, float &af,
                                       float &bf) {
    const WscaleSum &s0 = *p.st.sum[0];
    const double W0 = s0.wsum, vbar0 = p.st.lab[0]->vbar;
    WscaleFit f;
    f.m0 = swp / W0;
    f.vbar0 = vbar0;
    const double M0 = swpp - swp * f.m0;
    f.c0 = swpv - swp * vbar0;
    const bool flat = mn == mx || M0 <= 0.0 || s0.rows == 1u;
    f.b = flat ? 0.0 : f.c0 / M0;
    const double a = flat ? *p.st.ybar + vbar0 : *p.st.ybar + vbar0 - f.b * f.m0;
    af = (float)a; bf = (float)f.b;
    f.nan = bad || s0.usable == 0u || !finite_f(af) || !finite_f(bf);
    if (f.nan) af = bf = __builtin_nanf("");
    return f;
}

// the score of column k under the fit; the sums are column k's
__device__ inline float wscale_score(const WscaleParams &p, const WscaleFit &f, int k, double swp, double swpp, double swpv, bool bad) {
    const WscaleSum &sk = *p.st.sum[k];
    const double Wk = sk.wsum, vbar = p.st.lab[k]->vbar, V = p.st.lab[k]->V;
    if (f.nan || bad || sk.usable == 0u) return __builtin_nanf("");
    double num;
    if (k == 0) {
        num = V - f.b * f.c0;
    } else {
        const double m = swp / Wk;
        const double M = swpp - swp * m;
        const double c = swpv - swp * vbar;
        const double delta = f.b * (m - f.m0) - (vbar - f.vbar0);
        num = f.b * f.b * M - 2.0 * f.b * c + V + Wk * (delta * delta);
    }
    return (float)((num < 0.0 ? 0.0 : num) / Wk);
}

// ---- 2. the register interpreter ---------------------------------------------------------------------------------------------------------
// KW: columns of three float64 accumulators per lane, 0 = no weights (one column, the weight of a row is 1)
// "Not looked at" without a select per column: a prediction that is not finite enters the sums as 0.0 -- every column that weights
// its row is marked bad and comes out NaN whatever the sums hold -- so every term is finite, and a weight of exactly 0 adds an exact
// zero through the multiply-add as it is.  The multiply-adds are explicit fma calls (one rounding; -ffp-contract=off leaves them be):
// a power-of-two factor on a weight row still passes through every one of them exactly.
template <int VL, bool LEAN, int KW>
__global__ __launch_bounds__(kWscaleWaves * 64, VL <= 16 ? (LEAN ? wscale_lean_waves(KW) : 2) : 1) void sr_wscale_kernel(WscaleParams p) {
    constexpr int K = kWscaleK, DEPTH = kWscaleDepth, TILE = kWave * K, NC = KW ? KW : 1, MB = wscale_batch(KW);
    __shared__ double part[2][MB][kWscaleWaves][NC][3];   // per tree, wave and column: Swp, Swpp, Swpv; double-buffered by batch parity
    __shared__ float pmn[2][MB][kWscaleWaves], pmx[2][MB][kWscaleWaves];   // column 0
    __shared__ int pbad[2][MB][kWscaleWaves];             // bit k: column k met a prediction that is not finite
    __shared__ float wts[kWscaleWaves][NC][K][kWave];     // the weights of the wave's tile; a lane reads only what it wrote
    __shared__ int cls_s[2][MB];
    __shared__ unsigned next_s[2];

    if (!LEAN && uni((int)p.counter[2]) == 0) return;   // the LEAN pass marked nothing
    unsigned *const batches = p.counter + (LEAN ? 0 : 3);
    using VARS = typename VecOf<VL>::type;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;
    const int batch = p.batch;
    const int nw = KW ? p.nw : 1;
    const bool single = p.ntiles <= W;   // every wave owns one tile for its whole life: rows, labels and weights are loaded once
    const double ybar = *p.st.ybar;

    VARS vars[K];
    float yv[K];
    bool valid[K];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long first = (long long)tile * TILE;   // (64 bits, wave-uniform: D may lie within a tile of INT_MAX)
            const long long left = (long long)p.D - first;
            const int rows = left < TILE ? (int)left : TILE;  // rows of this tile, >= 1
            const int off = k * kWave + lane;
            valid[k] = off < rows;
            const size_t dc = (size_t)first + (size_t)(valid[k] ? off : rows - 1);   // lanes past the end repeat the last row, with weight 0
            const float *xr = p.X + dc * p.var_len;
#pragma unroll
            for (int v = 0; v < VL; ++v) vars[k][v] = v < p.var_len ? xr[v] : 0.0f;
            yv[k] = p.y[dc];
            if (KW) {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c < nw) wts[w][c][k][lane] = valid[k] ? p.W[(size_t)c * p.D + dc] : 0.0f;
            }
        }
    };
    if (single) load_tile(w < p.ntiles ? w : 0);

    if (threadIdx.x == 0) next_s[0] = atomicAdd(batches, (unsigned)batch);
    __syncthreads();
    int par = 0;
    for (;;) {
        const unsigned next = uni(next_s[par]);
        if (next >= (unsigned)p.pop) break;
        const int t0 = (int)next;
        const int nb = p.pop - t0 < batch ? p.pop - t0 : batch;
        if (threadIdx.x == 0) next_s[par ^ 1] = atomicAdd(batches, (unsigned)batch);   // prefetch

        // ---- phase 1: classify the batch, trees split between the waves ----
        for (int b = w; b < nb; b += W) {
            const size_t row = (size_t)(t0 + b) * p.gp_len;
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
            int c = TREE_SKIP;   // (FULL pass: not marked for it)
            if (LEAN || uni(f2bits(p.loss[(size_t)(t0 + b) * nw])) == kSentinelHeavy)
                c = classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, DEPTH, LEAN ? 1 : 0);
            if (lane == 0) cls_s[par][b] = c;
        }
        __syncthreads();

        // ---- phase 2: every wave interprets every tree of the batch on its own rows ----
        for (int b = 0; b < nb; ++b) {
            if (uni(cls_s[par][b]) != TREE_OK) continue;
            const size_t row = (size_t)(t0 + b) * p.gp_len;
            const float *tv = p.value + row;
            const int16_t *tt = p.type + row;
            int len = uni((int)p.size[row]);
            len = len > p.gp_len ? p.gp_len : len;

            double s[NC][3];
#pragma unroll
            for (int c = 0; c < NC; ++c) s[c][0] = s[c][1] = s[c][2] = 0.0;
            float mn = __builtin_inff(), mx = -__builtin_inff();
            int bad = 0;
            for (int tile = w; tile < p.ntiles; tile += W) {
                if (!single) load_tile(tile);
                v16f outs[K];
                RegStack<K, DEPTH> st;
                st.h = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) st.tos[k] = 0.0f;
                for (int base = 0; base < len; base += kWave) {
                    const int r = base + lane;
                    uint32_t opv = 0, payv = 0;
                    if (r < len) {
                        const int i = len - 1 - r;
                        const Decoded dn = decode_node(tt[i], tv[i], false, p.var_len, 1);
                        opv = dn.op; payv = dn.pay;
                    }
                    const int n = len - base < kWave ? len - base : kWave;
                    run_chunk<false, LEAN, K, DEPTH>(opv, payv, n, st, RegVars<VL, K>{vars}, outs);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float pr = st.tos[k];
                    const int nf = finite_f(pr) ? 0 : 1;
                    const double pd = nf ? 0.0 : (double)pr;   // (see the note above the kernel: a weight of 0 then adds an exact 0)
                    const double pp = pd * pd, pv = pd * ((double)yv[k] - ybar);
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (c < nw) {
                            const float wv = KW ? wts[w][c][k][lane] : (valid[k] ? 1.0f : 0.0f);
                            const bool on = wv != 0.0f;   // a row without weight is not looked at
                            const double wd = (double)wv;
                            s[c][0] = fma(wd, pd, s[c][0]);
                            s[c][1] = fma(wd, pp, s[c][1]);
                            s[c][2] = fma(wd, pv, s[c][2]);
                            bad |= on ? nf << c : 0;
                            if (c == 0) {
                                mn = on ? fminf(mn, pr) : mn;
                                mx = on ? fmaxf(mx, pr) : mx;
                            }
                        }
                    }
                }
            }
            int wbad = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (c < nw) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const double ts = wave_sum_d(s[c][j]);
                        if (lane == 0) part[par][b][w][c][j] = ts;
                    }
                    wbad |= __any(bad & (1 << c)) ? 1 << c : 0;
                }
            }
            const float tmn = wave_min_f(mn), tmx = wave_max_f(mx);
            if (lane == 0) { pbad[par][b][w] = wbad; pmn[par][b][w] = tmn; pmx[par][b][w] = tmx; }
        }
        __syncthreads();

        // ---- phase 3: one thread per tree adds the waves' partials in wave order, evaluates the closed form and stores ----
        if ((int)threadIdx.x < nb) {
            const int b = threadIdx.x, t = t0 + b;
            const int c = cls_s[par][b];
            if (c != TREE_SKIP) {
                const float nan = __builtin_nanf("");
                float out[NC], af = nan, bf = nan;
#pragma unroll
                for (int k = 0; k < NC; ++k) out[k] = nan;
                if (c == TREE_OK) {
                    const int nwv = p.ntiles < W ? p.ntiles : W;
                    int tb = 0;
                    float mn = __builtin_inff(), mx = -__builtin_inff();
                    for (int i = 0; i < nwv; ++i) {
                        tb |= pbad[par][b][i];
                        mn = fminf(mn, pmn[par][b][i]); mx = fmaxf(mx, pmx[par][b][i]);
                    }
                    WscaleFit fit{};
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        if (k < nw) {
                            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
                            for (int i = 0; i < nwv; ++i) { s0 += part[par][b][i][k][0]; s1 += part[par][b][i][k][1]; s2 += part[par][b][i][k][2]; }
                            if (k == 0) fit = wscale_fit(p, s0, s1, s2, mn, mx, (tb & 1) != 0, af, bf);
                            out[k] = wscale_score(p, fit, k, s0, s1, s2, (tb >> k & 1) != 0);
                        }
                    }
                } else if (c == TREE_DEEP) {
                    out[0] = bits2f(kSentinelDeep); p.counter[1] = 1u;
                } else if (c == TREE_HEAVY) {
                    out[0] = bits2f(kSentinelHeavy); p.counter[2] = 1u;
                }
                float *lo = p.loss + (size_t)t * nw;
#pragma unroll
                for (int k = 0; k < NC; ++k)
                    if (k < nw) lo[k] = out[k];
                p.coef[2 * (size_t)t] = af;
                p.coef[2 * (size_t)t + 1] = bf;
            }
        }
        par ^= 1;
    }
}

// ---- 3. the scratch-stack interpreter: one wave per tree, lanes are rows -------------------------------------------------------------------
__global__ __launch_bounds__(64) void sr_wscale_general_kernel(WscaleParams p, int only_marked) {
    constexpr int NC = EVOGP_WLOSS_MAX_WEIGHTS;
    const int lane = threadIdx.x & 63;
    if (only_marked && uni((int)p.counter[1]) == 0) return;   // no tree was too deep for the register stack
    float stk[kMaxStack + 2];
    float outs[1];
    const int nw = p.nw;
    const double ybar = *p.st.ybar;
    auto process = [&](int t) {
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *tt = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int cls = uni(classify_tree(tt, tv, len, false, p.var_len, 1, kMaxStack));
        double s[NC][3];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c][0] = s[c][1] = s[c][2] = 0.0;
        float mn = __builtin_inff(), mx = -__builtin_inff();
        int bad = 0;
        if (cls == TREE_OK) {
            for (long long base = 0; base < p.D; base += kWave) {
                const long long d = base + lane;
                const bool valid = d < p.D;
                const size_t dc = valid ? (size_t)d : (size_t)p.D - 1;
                const float pr = run_general<false>(tt, tv, len, p.X + dc * p.var_len, p.var_len, 1, outs, stk);
                const int nf = finite_f(pr) ? 0 : 1;
                const double pd = nf ? 0.0 : (double)pr;
                const double pp = pd * pd, pv = pd * ((double)p.y[dc] - ybar);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (c < nw) {
                        const float wv = !valid ? 0.0f : p.W ? p.W[(size_t)c * p.D + dc] : 1.0f;
                        const bool on = wv != 0.0f;
                        const double wd = (double)wv;
                        s[c][0] = fma(wd, pd, s[c][0]);
                        s[c][1] = fma(wd, pp, s[c][1]);
                        s[c][2] = fma(wd, pv, s[c][2]);
                        bad |= on ? nf << c : 0;
                        if (c == 0) {
                            mn = on ? fminf(mn, pr) : mn;
                            mx = on ? fmaxf(mx, pr) : mx;
                        }
                    }
                }
            }
        }
        const float tmn = wave_min_f(mn), tmx = wave_max_f(mx);
        const float nan = __builtin_nanf("");
        float out[NC], af = nan, bf = nan;
        WscaleFit fit{};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            out[c] = nan;
            if (c < nw) {
                const double s0 = wave_sum_d(s[c][0]), s1 = wave_sum_d(s[c][1]), s2 = wave_sum_d(s[c][2]);
                const bool cbad = __any(bad & (1 << c)) != 0;
                if (cls == TREE_OK) {   // (a malformed tree: NaN everywhere)
                    if (c == 0) fit = wscale_fit(p, s0, s1, s2, tmn, tmx, cbad, af, bf);
                    out[c] = wscale_score(p, fit, c, s0, s1, s2, cbad);
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nw) p.loss[(size_t)t * nw + c] = out[c];
            p.coef[2 * (size_t)t] = af;
            p.coef[2 * (size_t)t + 1] = bf;
        }
    };
    if (!only_marked) {
        for (long long t = blockIdx.x; t < p.pop; t += gridDim.x) process((int)t);
        return;
    }
    // behind the register kernel: a contiguous chunk of the population per wave, its mark words read 64 at a time (sr_scale_general_kernel)
    const long long chunk = (((long long)p.pop + gridDim.x - 1) / gridDim.x + 63) & ~63ll;   // (64 bits: pop may lie near INT_MAX)
    const long long c0 = blockIdx.x * chunk < p.pop ? blockIdx.x * chunk : p.pop;
    const long long c1 = c0 + chunk < p.pop ? c0 + chunk : p.pop;
    for (long long base = c0; base < c1; base += kWave) {
        const long long t = base + lane;
        const bool hit = t < c1 && f2bits(p.loss[(size_t)t * nw]) == kSentinelDeep;
        unsigned long long mk = __ballot(hit);
        while (mk) {
            const int b = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            process((int)(base + b));
        }
    }
}

template <int VL, bool LEAN, int KW>
static hipError_t launch_wscale(WscaleParams p, hipStream_t stream) {
    auto kern = sr_wscale_kernel<VL, LEAN, KW>;
    const DeviceInfo &dev = device_info();
    p.ntiles = (int)(((long long)p.D + kWave * kWscaleK - 1) / (kWave * kWscaleK));
    const int W = p.ntiles < kWscaleWaves ? p.ntiles : kWscaleWaves;
    static int per_cu_cache[kWscaleWaves + 1] = {0};   // occupancy per block size of THIS instantiation
    int per_cu = per_cu_cache[W];
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, W * 64, 0);
        if (e != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        per_cu_cache[W] = per_cu;
    }
    long blocks = (long)dev.num_cus * per_cu;
    long batch = p.pop / (blocks * 16);   // ~16 batches per workgroup: a short tail, rare atomics
    batch = batch < 4 ? 4 : (batch > wscale_batch(KW) ? wscale_batch(KW) : batch);
    p.batch = (int)batch;
    const long need = (p.pop + batch - 1) / batch;
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(W * 64), 0, stream, p);
    return hipGetLastError();
}

template <int KW>
static hipError_t launch_wscale_pair(const WscaleParams &p, hipStream_t stream) {
    hipError_t e = p.var_len <= 12 ? launch_wscale<12, true, KW>(p, stream) : launch_wscale<32, true, KW>(p, stream);
    if (e != hipSuccess) return e;
    return p.var_len <= 12 ? launch_wscale<12, false, KW>(p, stream) : launch_wscale<32, false, KW>(p, stream);
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_weighted_scaling(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                             const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                             const float *labels, const float *weights, unsigned n_weights, float *loss, float *coef,
                                             evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (n_weights < 1 || n_weights > EVOGP_WLOSS_MAX_WEIGHTS || (!weights && n_weights != 1)) return EVOGP_E_BADARG;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    if (!value || !type || !size || !variables || !labels || !loss || !coef) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const DeviceInfo &dev = device_info();
    hipError_t e;
    WscaleParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.W = weights; p.loss = loss; p.coef = coef;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.nw = (int)n_weights;
    p.st.ybar = (double *)acquire_counter(stream, &e);
    if (!p.st.ybar) return (int)e;
    for (int k = 0; k < p.nw; ++k) {
        p.st.sum[k] = (WscaleSum *)acquire_counter(stream, &e);
        if (!p.st.sum[k]) return (int)e;
        p.st.lab[k] = (WscaleLab *)acquire_counter(stream, &e);
        if (!p.st.lab[k]) return (int)e;
    }
    hipLaunchKernelGGL(wscale_stats_kernel, dim3(1), dim3(kStatsThreads), 0, stream, labels, weights, p.D, p.nw, p.st);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    p.counter = acquire_counter(stream, &e);
    if (!p.counter) return (int)e;
    const bool regs = p.var_len <= 32;
    if (regs) {
        e = !weights ? launch_wscale_pair<0>(p, stream) : p.nw <= 2 ? launch_wscale_pair<2>(p, stream) : launch_wscale_pair<8>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    long blocks = (long)dev.num_cus * (regs ? 4 : 16);
    if (blocks > p.pop) blocks = p.pop;
    hipLaunchKernelGGL(sr_wscale_general_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, p, regs ? 1 : 0);
    return (int)hipGetLastError();
}
