// sr_scale.hip — linear scaling of single-output SR trees (Keijzer 2003): the mean squared error of  a + b * T(x)  with the
// least-squares a, b of every tree, and the rewrite that writes those coefficients into the tree (gfx950; no counterpart in the reference).
//
// evogp_hip_sr_linear_scaling (include/evogp_hip.h has the contract).  Per tree three float64 sums over the float32 predictions p_d,
//     Sp = sum p_d      Spp = sum p_d^2      Spv = sum p_d * ((double)y_d - ybar)
// plus min p_d, max p_d and "some p_d is not finite" in float32: the closed form needs nothing else, so the (pop, D) predictions are
// never stored.  Four launches on the caller's stream, nothing synchronises with the host:
//   1. label_stats_kernel   (sr_moments.hpp) ONE workgroup: ybar and Syy = sum ((double)y_d - ybar)^2 in a fixed order, two doubles that stay on the device
//   2. sr_scale_kernel      sr_fast_kernel's decomposition (sr_fitness.hip) on the register interpreter (interp.hpp run_chunk), launched
//                           twice as sr_fitness.hip's launch_pair: the LEAN build over every tree, then the FULL build (all 29 functions)
//                           over the trees the LEAN one marked as using a transcendental function or pow.  The rows are cut into tiles of 64 x K, wave w of a workgroup takes tiles w, w + W, ...; the
//                           workgroup pulls batches of trees from a counter, the waves split the batch to classify it and then every
//                           wave interprets every tree of the batch on its own rows.  A lane adds its rows into float64 partials (its
//                           tiles in ascending order), the 64 lanes are added by the fixed butterfly (wave_sum_d), the waves' partials
//                           are parked in LDS and added in wave order by one thread per tree, which also evaluates the closed form:
//                           no float atomics, and a tree's result depends on the tree and the dataset alone
//   3. sr_scale_general_kernel   a wave per tree with the operand stack in scratch memory (run_general) for the trees the kernels of 2 marked
//                           too deep for its registers -- it leaves at once when there are none -- and for every tree of a forest with
//                           more variables than the register tuples hold (kernel 2 is then not launched)
// The kernel's p_d are batch_evaluate's bits: the same node arithmetic (interp.hpp, -ffp-contract=off), one operation per node.
//
// evogp_hip_wrap_linear: one wave per tree, coalesced copies in the style of replace_row.hpp build_row.
#include "interp.hpp"
#include "launch.hpp"
#include "sr_moments.hpp"
#include "sr_params.hpp"

namespace evogp {

constexpr int kScaleK = 4;        // rows per lane
constexpr int kScaleDepth = 16;   // register stack entries; deeper trees go to the scratch stack
constexpr int kScaleWaves = 4;    // waves per workgroup: a workgroup's row tile is 64 * kScaleK * kScaleWaves = 1024 rows
// Resident waves per SIMD the LEAN build is held to.  Unbounded it takes 186 VGPRs (two waves); at the 168 of three waves it spills 10
// registers (36 B of scratch per lane) and is still the faster one: the interpreter waits on latency, not on registers.
constexpr int kScaleLeanWaves = 3;

struct ScaleParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;        // [D][var_len]
    const float *y;        // [D]
    float *loss;           // [pop]
    float *coef;           // [pop][2]: intercept, slope
    const double *stats;   // ybar, Syy (label_stats_kernel)
    unsigned *counter;     // [0] batch counter of the LEAN pass, [1] != 0: some tree carries kSentinelDeep, [2] != 0: some tree carries
                           // kSentinelHeavy, [3] batch counter of the FULL pass
    int pop, D, gp_len, var_len, batch, ntiles;
};

// ---- the closed form (one thread per tree) ---------------------------------------------------------------------------------------------
struct Moments {
    double sp, spp, spv;
    float mn, mx;
    bool bad;   // a prediction that is not finite
};

__device__ inline void scale_store(const ScaleParams &p, int t, const Moments &m) {
    const float nan = __builtin_nanf("");
    float lf = nan, af = nan, bf = nan;
    if (!m.bad) {
        const double D = (double)p.D, ybar = p.stats[0], syy = p.stats[1];
        const double mean = m.sp / D;
        const double var = m.spp / D - mean * mean;
        const double cov = m.spv / D;
        double a = ybar, b = 0.0, loss = syy / D;
        if (!(m.mn == m.mx || var <= 0.0 || p.D == 1)) {
            b = cov / var;
            a = ybar - b * mean;
            loss = syy / D - b * cov;
            loss = loss > 0.0 ? loss : 0.0;
        }
        lf = (float)loss; af = (float)a; bf = (float)b;
        if (!finite_f(af) || !finite_f(bf)) lf = af = bf = nan;
    }
    p.loss[t] = lf;
    p.coef[2 * (size_t)t] = af;
    p.coef[2 * (size_t)t + 1] = bf;
}

// ---- 2. the register interpreter -----------------------------------------------------------------------------------------------------
// Two builds, as sr_fitness.hip's launch_pair: the LEAN one (no transcendental function, no pow: fewer registers, more resident waves --
// the interpreter is latency bound) takes every tree and marks those that use such a function with kSentinelHeavy; the FULL one, right
// behind it, takes the marked trees only and leaves at once when there are none.  Which build evaluates a tree depends on the tree alone.
template <int VL, bool LEAN>
__global__ __launch_bounds__(kScaleWaves * 64, VL <= 16 ? (LEAN ? kScaleLeanWaves : 2) : 1) void sr_scale_kernel(ScaleParams p) {
    constexpr int K = kScaleK, DEPTH = kScaleDepth, TILE = kWave * K;
    __shared__ double part[2][kMaxBatch][kScaleWaves][3];   // per tree and wave: Sp, Spp, Spv; double-buffered by batch parity
    __shared__ float pmn[2][kMaxBatch][kScaleWaves], pmx[2][kMaxBatch][kScaleWaves];
    __shared__ int pbad[2][kMaxBatch][kScaleWaves];
    __shared__ int cls_s[2][kMaxBatch];
    __shared__ unsigned next_s[2];   // (unsigned: the counter runs past pop by up to two batches per workgroup)

    if (!LEAN && uni((int)p.counter[2]) == 0) return;   // the LEAN pass marked nothing
    unsigned *const batches = p.counter + (LEAN ? 0 : 3);
    using VARS = typename VecOf<VL>::type;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;
    const int batch = p.batch;
    const bool single = p.ntiles <= W;   // every wave owns one tile for its whole life: rows and labels are loaded once
    const double ybar = p.stats[0];

    VARS vars[K];
    float yv[K];   // (centred in the epilogue: ybar is wave-uniform)
    bool valid[K];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long first = (long long)tile * TILE;   // (64 bits, wave-uniform: D may lie within a tile of INT_MAX)
            const long long left = (long long)p.D - first;
            const int rows = left < TILE ? (int)left : TILE;  // rows of this tile, >= 1
            const int off = k * kWave + lane;
            valid[k] = off < rows;
            const size_t dc = (size_t)first + (size_t)(valid[k] ? off : rows - 1);   // lanes past the end repeat the last row: min, max and "finite" are not disturbed
            const float *xr = p.X + dc * p.var_len;
#pragma unroll
            for (int v = 0; v < VL; ++v) vars[k][v] = v < p.var_len ? xr[v] : 0.0f;
            yv[k] = p.y[dc];
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
            if (LEAN || uni(f2bits(p.loss[t0 + b])) == kSentinelHeavy)
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

            double sp = 0.0, spp = 0.0, spv = 0.0;
            float mn = __builtin_inff(), mx = -__builtin_inff();
            bool bad = false;
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
                    bad |= !finite_f(pr);
                    mn = fminf(mn, pr);
                    mx = fmaxf(mx, pr);
                    const double pd = valid[k] ? (double)pr : 0.0;
                    sp += pd;
                    spp += pd * pd;
                    spv += pd * ((double)yv[k] - ybar);
                }
            }
            const bool any_bad = __any(bad) != 0;
            const double tsp = wave_sum_d(sp), tspp = wave_sum_d(spp), tspv = wave_sum_d(spv);
            const float tmn = wave_min_f(mn), tmx = wave_max_f(mx);
            if (lane == 0) {
                part[par][b][w][0] = tsp; part[par][b][w][1] = tspp; part[par][b][w][2] = tspv;
                pmn[par][b][w] = tmn; pmx[par][b][w] = tmx; pbad[par][b][w] = any_bad ? 1 : 0;
            }
        }
        __syncthreads();

        // ---- phase 3: one thread per tree adds the waves' partials in wave order and evaluates the closed form ----
        if ((int)threadIdx.x < nb) {
            const int b = threadIdx.x, t = t0 + b;
            const int c = cls_s[par][b];
            if (c == TREE_OK) {
                const int nw = p.ntiles < W ? p.ntiles : W;
                Moments m{0.0, 0.0, 0.0, __builtin_inff(), -__builtin_inff(), false};
                for (int i = 0; i < nw; ++i) {
                    m.sp += part[par][b][i][0]; m.spp += part[par][b][i][1]; m.spv += part[par][b][i][2];
                    m.mn = fminf(m.mn, pmn[par][b][i]); m.mx = fmaxf(m.mx, pmx[par][b][i]);
                    m.bad = m.bad || pbad[par][b][i] != 0;
                }
                scale_store(p, t, m);
            } else if (c != TREE_SKIP) {
                const float nan = __builtin_nanf("");
                p.loss[t] = c == TREE_DEEP ? bits2f(kSentinelDeep) : c == TREE_HEAVY ? bits2f(kSentinelHeavy) : nan;
                p.coef[2 * (size_t)t] = nan;
                p.coef[2 * (size_t)t + 1] = nan;
                if (c == TREE_DEEP) p.counter[1] = 1u;
                if (c == TREE_HEAVY) p.counter[2] = 1u;
            }
        }
        par ^= 1;
    }
}

// ---- 3. the scratch-stack interpreter: one wave per tree, lanes are rows --------------------------------------------------------------
__global__ __launch_bounds__(64) void sr_scale_general_kernel(ScaleParams p, int only_marked) {
    const int lane = threadIdx.x & 63;
    if (only_marked && uni((int)p.counter[1]) == 0) return;   // no tree was too deep for the register stack
    float stk[kMaxStack + 2];
    float outs[1];
    const double ybar = p.stats[0];
    auto process = [&](int t) {
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *tt = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int cls = uni(classify_tree(tt, tv, len, false, p.var_len, 1, kMaxStack));
        Moments m{0.0, 0.0, 0.0, __builtin_inff(), -__builtin_inff(), cls != TREE_OK};
        if (cls == TREE_OK) {
            double sp = 0.0, spp = 0.0, spv = 0.0;
            float mn = __builtin_inff(), mx = -__builtin_inff();
            bool bad = false;
            for (long long base = 0; base < p.D; base += kWave) {
                const long long d = base + lane;
                const bool valid = d < p.D;
                const size_t dc = valid ? (size_t)d : (size_t)p.D - 1;
                const float pr = run_general<false>(tt, tv, len, p.X + dc * p.var_len, p.var_len, 1, outs, stk);
                bad |= !finite_f(pr);
                mn = fminf(mn, pr);
                mx = fmaxf(mx, pr);
                const double pd = valid ? (double)pr : 0.0;
                sp += pd;
                spp += pd * pd;
                spv += pd * ((double)p.y[dc] - ybar);
            }
            m.bad = __any(bad) != 0;
            m.sp = wave_sum_d(sp); m.spp = wave_sum_d(spp); m.spv = wave_sum_d(spv);
            m.mn = wave_min_f(mn); m.mx = wave_max_f(mx);
        }
        if (lane == 0) scale_store(p, t, m);   // (a malformed tree: bad -> NaN)
    };
    if (!only_marked) {
        for (long long t = blockIdx.x; t < p.pop; t += gridDim.x) process((int)t);
        return;
    }
    // behind the register kernel: a contiguous chunk of the population per wave, its mark words read 64 at a time (sr_general_kernel)
    const long long chunk = (((long long)p.pop + gridDim.x - 1) / gridDim.x + 63) & ~63ll;   // (64 bits: pop may lie near INT_MAX)
    const long long c0 = blockIdx.x * chunk < p.pop ? blockIdx.x * chunk : p.pop;
    const long long c1 = c0 + chunk < p.pop ? c0 + chunk : p.pop;
    for (long long base = c0; base < c1; base += kWave) {
        const long long t = base + lane;
        const bool hit = t < c1 && f2bits(p.loss[t]) == kSentinelDeep;
        unsigned long long mk = __ballot(hit);
        while (mk) {
            const int b = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            process((int)(base + b));
        }
    }
}

// ---- the rewrite: T -> ADD(MUL(T, slope), intercept) ------------------------------------------------------------------------------------
constexpr int kWrapWaves = 4;

struct WrapParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *coef;
    float *out_value;
    int16_t *out_type;
    int16_t *out_size;
    unsigned char *applied;
    int pop, gp_len, out_len;
};

__global__ __launch_bounds__(kWrapWaves * 64) void wrap_linear_kernel(WrapParams q) {
    const int lane = threadIdx.x & 63;
    const int t = uni((int)(blockIdx.x * kWrapWaves) + (int)(threadIdx.x >> 6));
    if (t >= q.pop) return;
    const int L = q.gp_len, Lo = q.out_len;
    const size_t row = (size_t)t * L, orow = (size_t)t * Lo;
    int len = uni((int)q.size[row]);
    len = len < 0 ? 0 : (len > L ? L : len);
    const int cls = uni(classify_tree(q.type + row, q.value + row, len, false, 1, 1, kMaxStack));
    const float a = q.coef[2 * (size_t)t], b = q.coef[2 * (size_t)t + 1];
    const bool wrap = cls == TREE_OK && finite_f(a) && finite_f(b) && len + 4 <= Lo;
    for (int j = lane; j < Lo; j += kWave) {
        float v = 0.0f;
        int ty = 0, s = 0;
        if (!wrap) {
            if (j < L) { v = q.value[row + j]; ty = q.type[row + j]; s = q.size[row + j]; }
        } else if (j == 0) {
            v = (float)F_ADD; ty = T_BFUNC; s = len + 4;
        } else if (j == 1) {
            v = (float)F_MUL; ty = T_BFUNC; s = len + 2;
        } else if (j < len + 2) {
            v = q.value[row + j - 2]; ty = q.type[row + j - 2]; s = q.size[row + j - 2];
        } else if (j < len + 4) {
            v = j == len + 2 ? b : a; ty = T_CONST; s = 1;
        }
        q.out_value[orow + j] = v;
        q.out_type[orow + j] = (int16_t)ty;
        q.out_size[orow + j] = (int16_t)s;
    }
    if (lane == 0) q.applied[t] = wrap ? 1 : 0;
}

template <int VL, bool LEAN>
static hipError_t launch_scale(ScaleParams p, hipStream_t stream) {
    auto kern = sr_scale_kernel<VL, LEAN>;
    const DeviceInfo &dev = device_info();
    p.ntiles = (int)(((long long)p.D + kWave * kScaleK - 1) / (kWave * kScaleK));
    const int W = p.ntiles < kScaleWaves ? p.ntiles : kScaleWaves;
    static int per_cu_cache[kScaleWaves + 1] = {0};   // occupancy per block size of THIS instantiation
    int per_cu = per_cu_cache[W];
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, W * 64, 0);
        if (e != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        per_cu_cache[W] = per_cu;
    }
    long blocks = (long)dev.num_cus * per_cu;
    long batch = p.pop / (blocks * 16);   // ~16 batches per workgroup: a short tail, rare atomics
    batch = batch < 4 ? 4 : (batch > kMaxBatch ? kMaxBatch : batch);
    p.batch = (int)batch;
    const long need = (p.pop + batch - 1) / batch;
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(W * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_linear_scaling(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                           const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                           const float *labels, float *loss, float *coef, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    if (!value || !type || !size || !variables || !labels || !loss || !coef) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const DeviceInfo &dev = device_info();
    hipError_t e;
    unsigned *stats = acquire_counter(stream, &e);   // 16 bytes: the two doubles of the label statistics
    if (!stats) return (int)e;
    ScaleParams p{};
    p.counter = acquire_counter(stream, &e);
    if (!p.counter) return (int)e;
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.loss = loss; p.coef = coef;
    p.stats = (const double *)stats;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    hipLaunchKernelGGL(label_stats_kernel, dim3(1), dim3(kStatsThreads), 0, stream, labels, p.D, (double *)stats);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const bool regs = p.var_len <= 32;
    if (regs) {
        e = p.var_len <= 12 ? launch_scale<12, true>(p, stream) : launch_scale<32, true>(p, stream);
        if (e != hipSuccess) return (int)e;
        e = p.var_len <= 12 ? launch_scale<12, false>(p, stream) : launch_scale<32, false>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    long blocks = (long)dev.num_cus * (regs ? 4 : 16);
    if (blocks > p.pop) blocks = p.pop;
    hipLaunchKernelGGL(sr_scale_general_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, p, regs ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_wrap_linear(unsigned pop_size, unsigned gp_len, unsigned out_gp_len, const float *value, const int16_t *type,
                                     const int16_t *size, const float *coef, float *out_value, int16_t *out_type, int16_t *out_size,
                                     unsigned char *applied, evogp_stream_t stream_) {
    if (pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || out_gp_len < gp_len || out_gp_len > (unsigned)kMaxStack ||
        pop_size > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !coef || !out_value || !out_type || !out_size || !applied) return EVOGP_E_NULLPTR;
    if (out_value == value || out_type == type || out_size == size) return EVOGP_E_BADARG;   // not in place
    WrapParams q{};
    q.value = value; q.type = type; q.size = size; q.coef = coef;
    q.out_value = out_value; q.out_type = out_type; q.out_size = out_size; q.applied = applied;
    q.pop = (int)pop_size; q.gp_len = (int)gp_len; q.out_len = (int)out_gp_len;
    const unsigned blocks = (pop_size + kWrapWaves - 1) / kWrapWaves;
    hipLaunchKernelGGL(wrap_linear_kernel, dim3(blocks), dim3(kWrapWaves * 64), 0, (hipStream_t)stream_, q);
    return (int)hipGetLastError();
}
