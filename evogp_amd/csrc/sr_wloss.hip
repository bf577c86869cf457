// sr_wloss.hip — weighted, robust and held-out losses of single-output SR trees in one pass over the dataset (gfx950; no counterpart in
// the reference).
//
// evogp_hip_sr_weighted_loss (include/evogp_hip.h has the contract).  Per tree and weight row k one float64 sum over the float32
// predictions p_d,
//     S_k = sum over the rows with W[k, d] != 0 of  W[k, d] * rho((double)p_d - (double)y_d)
// and "some such row has a prediction that is not finite"; the result is (float)(S_k / sum_d W[k, d]).  The (pop, D) predictions are never
// stored, and a row a column gives no weight to is not looked at in that column.  The launches, all on the caller's stream, nothing
// synchronises with the host:
//   1. weight_stats_kernel  ONE workgroup (sr_moments.hpp, next to label_stats_kernel and rho): per weight row the float64 sum in a fixed order
//                           and whether the row may be used (no negative or non-finite weight, a sum that is not 0); both stay on the
//                           device.  Not launched without weights.
//   2. sr_wloss_kernel      sr_scale_kernel's decomposition (sr_scale.hip: the register interpreter, LEAN then FULL over the
//                           kSentinelHeavy marks, batches from a counter, the `single` path) with this epilogue.  The weights of a wave's
//                           tile are parked in LDS, every lane in slots of its own, when the tile's rows are loaded -- K rows of weights
//                           in registers next to the interpreter's do not fit the LEAN build -- and read back one at a time in the
//                           epilogue.  The kernel is built for KW = 0 (no weights: the weight is 1, nothing is loaded), 2 and 8 float64
//                           accumulators per lane, and once more for log-cosh alone (wloss_rho).  Which build runs a column changes
//                           nothing in it: the columns share rho and nothing else.
//   3. sr_wloss_general_kernel   a wave per tree with the operand stack in scratch memory (run_general) for the trees too deep for the
//                           registers and for every tree of a forest with var_len > 32, as sr_scale_general_kernel.
// Sums keep sr_scale_kernel's order: a lane's tiles ascending, the 64 lanes by wave_sum_d, the waves in wave order by one thread per tree.
#include <math.h>

#include "interp.hpp"
#include "launch.hpp"
#include "sr_moments.hpp"
#include "sr_params.hpp"

namespace evogp {

constexpr int kWlossK = 4;        // rows per lane
constexpr int kWlossDepth = 16;   // register stack entries; deeper trees go to the scratch stack
constexpr int kWlossWaves = 4;    // waves per workgroup: a workgroup's row tile is 64 * kWlossK * kWlossWaves = 1024 rows
constexpr int kWlossLeanWaves = 3;   // resident waves per SIMD of the LEAN build (sr_scale.hip kScaleLeanWaves)
static_assert(EVOGP_WLOSS_MAX_WEIGHTS == 8, "the accumulator widths end at 8");
// trees per batch: the LDS partial-sum slots.  At 8 columns 32 trees keep partials and weights under a third of a CU's LDS
constexpr int wloss_batch(int KW) { return KW == 8 ? kMaxBatch / 2 : kMaxBatch; }

struct WlossParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;        // [D][var_len]
    const float *y;        // [D]
    const float *W;        // [nw][D], or nullptr: one column of weights 1
    float *loss;           // [pop][nw]; column 0 carries the kSentinel marks between the passes
    const WeightStat *stat[EVOGP_WLOSS_MAX_WEIGHTS];   // (weight_stats_kernel; unused without W)
    unsigned *counter;     // as ScaleParams::counter
    double prm;            // delta (huber) or tau (pinball)
    int kind;
    int pop, D, gp_len, var_len, nw, batch, ntiles;
};

// (float)(S / Wsum), NaN for a column that may not be used or that met a non-finite prediction
__device__ inline float wloss_value(const WlossParams &p, int k, double s, bool bad) {
    double wsum = (double)p.D;
    bool usable = true;
    if (p.W) { wsum = p.stat[k]->sum; usable = p.stat[k]->usable != 0; }
    return usable && !bad ? (float)(s / wsum) : __builtin_nanf("");
}

// ---- 2. the register interpreter ---------------------------------------------------------------------------------------------------------
// KW: float64 accumulators per lane, 0 = no weights (one column, the weight of a row is 1)
template <int VL, bool LEAN, int KW, bool LC>
__global__ __launch_bounds__(kWlossWaves * 64, VL <= 16 ? (LEAN ? kWlossLeanWaves : 2) : 1) void sr_wloss_kernel(WlossParams p) {
    constexpr int K = kWlossK, DEPTH = kWlossDepth, TILE = kWave * K, NC = KW ? KW : 1, MB = wloss_batch(KW);
    __shared__ double part[2][MB][kWlossWaves][NC];   // per tree, wave and column: S; double-buffered by batch parity
    __shared__ int pbad[2][MB][kWlossWaves];          // bit k: column k met a prediction that is not finite
    __shared__ float wts[kWlossWaves][NC][K][kWave];  // the weights of the wave's tile; a lane reads only what it wrote
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
    const int kind = p.kind;
    const double prm = p.prm;

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

            double s[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) s[c] = 0.0;
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
                    const double rho = wloss_rho<LC>(kind, prm, (double)pr - (double)yv[k]);
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (c < nw) {
                            const float wv = KW ? wts[w][c][k][lane] : (valid[k] ? 1.0f : 0.0f);
                            const bool on = wv != 0.0f;   // a row without weight is not looked at
                            s[c] += on ? (double)wv * rho : 0.0;
                            bad |= on ? nf << c : 0;
                        }
                    }
                }
            }
            int wbad = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (c < nw) {
                    const double ts = wave_sum_d(s[c]);
                    if (lane == 0) part[par][b][w][c] = ts;
                    wbad |= __any(bad & (1 << c)) ? 1 << c : 0;
                }
            }
            if (lane == 0) pbad[par][b][w] = wbad;
        }
        __syncthreads();

        // ---- phase 3: one thread per tree adds the waves' partials in wave order ----
        if ((int)threadIdx.x < nb) {
            const int b = threadIdx.x, t = t0 + b;
            const int c = cls_s[par][b];
            float *out = p.loss + (size_t)t * nw;
            if (c == TREE_OK) {
                const int nwv = p.ntiles < W ? p.ntiles : W;
                int tb = 0;
                for (int i = 0; i < nwv; ++i) tb |= pbad[par][b][i];
                for (int k = 0; k < nw; ++k) {
                    double sum = 0.0;
                    for (int i = 0; i < nwv; ++i) sum += part[par][b][i][k];
                    out[k] = wloss_value(p, k, sum, (tb >> k & 1) != 0);
                }
            } else if (c != TREE_SKIP) {
                const float nan = __builtin_nanf("");
                for (int k = 0; k < nw; ++k) out[k] = nan;
                if (c == TREE_DEEP) { out[0] = bits2f(kSentinelDeep); p.counter[1] = 1u; }
                if (c == TREE_HEAVY) { out[0] = bits2f(kSentinelHeavy); p.counter[2] = 1u; }
            }
        }
        par ^= 1;
    }
}

// ---- 3. the scratch-stack interpreter: one wave per tree, lanes are rows -------------------------------------------------------------------
__global__ __launch_bounds__(64) void sr_wloss_general_kernel(WlossParams p, int only_marked) {
    constexpr int NC = EVOGP_WLOSS_MAX_WEIGHTS;
    const int lane = threadIdx.x & 63;
    if (only_marked && uni((int)p.counter[1]) == 0) return;   // no tree was too deep for the register stack
    float stk[kMaxStack + 2];
    float outs[1];
    const int nw = p.nw;
    auto process = [&](int t) {
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *tt = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int cls = uni(classify_tree(tt, tv, len, false, p.var_len, 1, kMaxStack));
        double s[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = 0.0;
        int bad = 0;
        if (cls == TREE_OK) {
            for (long long base = 0; base < p.D; base += kWave) {
                const long long d = base + lane;
                const bool valid = d < p.D;
                const size_t dc = valid ? (size_t)d : (size_t)p.D - 1;
                const float pr = run_general<false>(tt, tv, len, p.X + dc * p.var_len, p.var_len, 1, outs, stk);
                const int nf = finite_f(pr) ? 0 : 1;
                const double r = (double)pr - (double)p.y[dc];
                const double rho = p.kind == EVOGP_LOSS_LOGCOSH ? wloss_rho<true>(p.kind, p.prm, r) : wloss_rho<false>(p.kind, p.prm, r);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    if (c < nw) {
                        const float wv = !valid ? 0.0f : p.W ? p.W[(size_t)c * p.D + dc] : 1.0f;
                        const bool on = wv != 0.0f;
                        s[c] += on ? (double)wv * rho : 0.0;
                        bad |= on ? nf << c : 0;
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < nw) {
                const double ts = wave_sum_d(s[c]);
                const bool cbad = cls != TREE_OK || __any(bad & (1 << c)) != 0;   // (a malformed tree: NaN)
                if (lane == 0) p.loss[(size_t)t * nw + c] = wloss_value(p, c, ts, cbad);
            }
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

template <int VL, bool LEAN, int KW, bool LC>
static hipError_t launch_wloss(WlossParams p, hipStream_t stream) {
    auto kern = sr_wloss_kernel<VL, LEAN, KW, LC>;
    const DeviceInfo &dev = device_info();
    p.ntiles = (int)(((long long)p.D + kWave * kWlossK - 1) / (kWave * kWlossK));
    const int W = p.ntiles < kWlossWaves ? p.ntiles : kWlossWaves;
    static int per_cu_cache[kWlossWaves + 1] = {0};   // occupancy per block size of THIS instantiation
    int per_cu = per_cu_cache[W];
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, W * 64, 0);
        if (e != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        per_cu_cache[W] = per_cu;
    }
    long blocks = (long)dev.num_cus * per_cu;
    long batch = p.pop / (blocks * 16);   // ~16 batches per workgroup: a short tail, rare atomics
    batch = batch < 4 ? 4 : (batch > wloss_batch(KW) ? wloss_batch(KW) : batch);
    p.batch = (int)batch;
    const long need = (p.pop + batch - 1) / batch;
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(W * 64), 0, stream, p);
    return hipGetLastError();
}

template <int KW, bool LC>
static hipError_t launch_wloss_pair(const WlossParams &p, hipStream_t stream) {
    hipError_t e = p.var_len <= 12 ? launch_wloss<12, true, KW, LC>(p, stream) : launch_wloss<32, true, KW, LC>(p, stream);
    if (e != hipSuccess) return e;
    return p.var_len <= 12 ? launch_wloss<12, false, KW, LC>(p, stream) : launch_wloss<32, false, KW, LC>(p, stream);
}

template <int KW>
static hipError_t launch_wloss_kind(const WlossParams &p, hipStream_t stream) {
    return p.kind == EVOGP_LOSS_LOGCOSH ? launch_wloss_pair<KW, true>(p, stream) : launch_wloss_pair<KW, false>(p, stream);
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_weighted_loss(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                          const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                          const float *labels, const float *weights, unsigned n_weights, int loss_kind, double loss_param,
                                          float *loss, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (n_weights < 1 || n_weights > EVOGP_WLOSS_MAX_WEIGHTS || (!weights && n_weights != 1)) return EVOGP_E_BADARG;
    if (loss_kind < EVOGP_LOSS_MSE || loss_kind > EVOGP_LOSS_LOGCOSH || loss_param != loss_param) return EVOGP_E_BADARG;
    if (loss_kind == EVOGP_LOSS_HUBER && !(loss_param > 0.0 && loss_param < HUGE_VAL)) return EVOGP_E_BADARG;
    if (loss_kind == EVOGP_LOSS_PINBALL && !(loss_param > 0.0 && loss_param < 1.0)) return EVOGP_E_BADARG;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    if (!value || !type || !size || !variables || !labels || !loss) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const DeviceInfo &dev = device_info();
    hipError_t e;
    WlossParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.W = weights; p.loss = loss;
    p.kind = loss_kind; p.prm = loss_param;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.nw = (int)n_weights;
    if (weights) {
        WeightStatOut out{};
        for (int k = 0; k < p.nw; ++k) {
            out.slot[k] = (WeightStat *)acquire_counter(stream, &e);   // 16 bytes: a sum and a flag
            if (!out.slot[k]) return (int)e;
            p.stat[k] = out.slot[k];
        }
        hipLaunchKernelGGL(weight_stats_kernel, dim3(1), dim3(kStatsThreads), 0, stream, weights, p.D, p.nw, out);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    p.counter = acquire_counter(stream, &e);
    if (!p.counter) return (int)e;
    const bool regs = p.var_len <= 32;
    if (regs) {
        e = !weights ? launch_wloss_kind<0>(p, stream) : p.nw <= 2 ? launch_wloss_kind<2>(p, stream) : launch_wloss_kind<8>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    long blocks = (long)dev.num_cus * (regs ? 4 : 16);
    if (blocks > p.pop) blocks = p.pop;
    hipLaunchKernelGGL(sr_wloss_general_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, p, regs ? 1 : 0);
    return (int)hipGetLastError();
}
