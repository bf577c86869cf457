// sr_hessian.hip — second input derivatives d^2 T / dx_a dx_b of single-output trees on the rows of the dataset, and the curvature loss
// and convexity counts computed from them without a (pop, D) array (gfx950; no counterpart in the reference).  DESIGN.md section 3.36.
// Reached through evogp_hip_sr_input_gradient / evogp_hip_sr_derivative_loss (sr_xgrad.hip) when wrt holds pair codes
// EVOGP_XGRAD_PAIR | a << 15 | b (include/evogp_hip.h).
//
// Forward mode on hyper-dual numbers in the register-stack interpreter: a stack entry is (v, t_a, t_b, t_ab), four float32 words
// (RegStack<4, 16>: 64 VGPRs); the rules are sr_hyperdual.hpp's.  No tape, no adjoint slot, no LDS on the node path.
//   sr_hessian_kernel   one workgroup per tree (trees gridDim apart), wave w takes the row tiles w, w + W, ... of 64 rows, a lane per row.  The
//                       tree is classified and decoded ONCE per workgroup: the (opv, payv) register pair up to 64 nodes, LDS beyond.  A
//                       tile's X row is loaded once -- a register tuple up to 32 variables, the wave's [variable][lane] block of LDS up
//                       to 128, the row in global memory beyond -- and the P <= 8 pairs run as one interpretation each over it.  A pair
//                       whose variables the tree does not both hold is not interpreted: its second derivative is +0.0f exactly.
//                       LEAN / FULL builds as in sr_scale.hip (the LEAN one marks the trees that use a transcendental function or pow,
//                       the FULL one takes them); the DEEP build takes the trees whose operand stack exceeds 16 entries with the stack as
//                       an [entry][word][lane] block of the per-stream workspace and the SAME node rules, waves and order of summation:
//                       a tree gives the same bits whichever build takes it.
// The primal word is computed by the functions the tape's forward walk calls (interp.hpp), so pred is sr_xgrad.hip's bit for bit.
// Materialising: pred [pop][D], dpred [P][pop][D]; a malformed tree is NaN in both.
// Fused: loss [pop][1 + P], viol [pop][P] by sr_xgrad.hip's epilogue: a lane adds its rows' float64 terms into its own words of an LDS
// block [wave][column][lane] in ascending tile order, the 64 lanes by the fixed butterfly, the waves in wave order; a column is NaN exactly
// when a row term is not finite; violations by ballot and popcount.  A malformed tree: NaN columns, D violations.  No float atomics,
// nothing synchronises with the host: the same inputs give the same bits.
#include "sr_hyperdual.hpp"
#include "sr_moments.hpp"

namespace evogp {

constexpr int kHessWaves = 4;                       // waves per workgroup: the row tiles of one tree
constexpr int kHessDepth = 16;                      // register stack entries (of four words each)
constexpr int kHessMaxPairs = EVOGP_XGRAD_MAX_VARS;
constexpr int kHessCols = 1 + kHessMaxPairs;
constexpr int kHessLdsVars = 128;                   // wider rows are read from global memory
constexpr size_t kHessLdsX = 32 * 1024;             // dynamic LDS of a workgroup, the waves' X blocks: 59 KiB with the static 27 KiB, no grant needed
constexpr uint32_t kHessNoVar = 0xFFFFFFFFu;        // a seed no VAR node matches: the plain interpretation

struct HessParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;      // [D][var_len]
    const float *y;      // [D]            (fused)
    const float *dy;     // [D][P] or nullptr: zeros (fused)
    const float *dmin;   // [P] or nullptr: -inf (fused)
    const float *dmax;   // [P] or nullptr: +inf (fused)
    float *pred;         // [pop][D]       (materialising)
    float *dpred;        // [P][pop][D]    (materialising)
    float *loss;         // [pop][1 + P]   (fused)
    int *viol;           // [pop][P]       (fused)
    float *deep;         // [deep blocks * W][gp_len + 2][4][64]: the operand stacks of the DEEP build
    int *cls;            // [pop]
    unsigned *flags;     // [1] != 0: some tree is TREE_DEEP, [2] != 0: some tree is TREE_HEAVY
    int va[kHessMaxPairs], vb[kHessMaxPairs];
    int pop, D, gp_len, var_len, P, ntiles, x_in_lds;
};

// where a lane's X row lives
template <int VL>
struct HessTuple {
    typename VecOf<VL>::type v;
    __device__ inline float get(uint32_t var) const { return v[var]; }
};
struct HessStrided {   // the lane's column of the wave's [variable][lane] LDS block (stride 64), or its row in global memory (stride 1)
    const float *base;
    int stride;
    __device__ inline float get(uint32_t var) const { return base[(size_t)var * stride]; }
};

// ---- run_chunk (interp.hpp) on hyper-dual numbers --------------------------------------------------------------------------------------
template <bool LEAN, class VA>
__device__ inline void run_chunk_hd(uint32_t opv, uint32_t payv, int n, RegStack<4, kHessDepth> &st, const VA &vars, uint32_t va, uint32_t vb) {
    uint32_t next_op = (uint32_t)__builtin_amdgcn_readlane((int)opv, 0);
    for (int j = 0; j < n; ++j) {
        const uint32_t op = next_op;
        next_op = (uint32_t)__builtin_amdgcn_readlane((int)opv, (j + 1) & 63);
        if (op < H_ADD) {
            const uint32_t pay = (uint32_t)__builtin_amdgcn_readlane((int)payv, j);
            const int h = st.h;
            st.h = h + 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) st.s[k][h] = st.tos[k];
            if (op == H_CONST) {
                st.tos[0] = bits2f(pay); st.tos[1] = 0.0f; st.tos[2] = 0.0f;
            } else {
                st.tos[0] = vars.get(pay);
                st.tos[1] = pay == va ? 1.0f : 0.0f;
                st.tos[2] = pay == vb ? 1.0f : 0.0f;
            }
            st.tos[3] = 0.0f;
        } else if (op < H_UN) {   // a = top (left operand), b = next
            const int h = st.h - 1;
            st.h = h;
            const HyperDual A{st.tos[0], st.tos[1], st.tos[2], st.tos[3]}, B{st.s[0][h], st.s[1][h], st.s[2][h], st.s[3][h]};
            const HyperDual R = hd_binary<LEAN>(op, A, B);
            st.tos[0] = R.v; st.tos[1] = R.ta; st.tos[2] = R.tb; st.tos[3] = R.tab;
        } else if (op < H_IF) {
            const HyperDual R = hd_unary<LEAN>(op, HyperDual{st.tos[0], st.tos[1], st.tos[2], st.tos[3]});
            st.tos[0] = R.v; st.tos[1] = R.ta; st.tos[2] = R.tb; st.tos[3] = R.tab;
        } else {   // IF: cond = top, then = next, else = third; the condition's tangents are dropped
            const int h = st.h - 2;
            st.h = h;
            const bool take_b = st.tos[0] > 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float b = st.s[k][h + 1], c = st.s[k][h];
                st.tos[k] = take_b ? b : c;
            }
        }
    }
}

// ---- run_general (interp.hpp) on hyper-dual numbers: word k of entry h is stk[(h * 4 + k) * 64], the lane's column -------------------------
template <class VA>
__device__ inline HyperDual run_deep_hd(const uint32_t *dop, const uint32_t *dpay, int len, float *stk, const VA &vars, uint32_t va, uint32_t vb) {
    auto load = [&](int h) { return HyperDual{stk[(h * 4) * kWave], stk[(h * 4 + 1) * kWave], stk[(h * 4 + 2) * kWave], stk[(h * 4 + 3) * kWave]}; };
    int h = 0;
    for (int r = 0; r < len; ++r) {
        const uint32_t op = uni(dop[r]), pay = uni(dpay[r]);
        HyperDual R;
        if (op < H_ADD) {
            if (op == H_CONST) R = {bits2f(pay), 0.0f, 0.0f, 0.0f};
            else R = {vars.get(pay), pay == va ? 1.0f : 0.0f, pay == vb ? 1.0f : 0.0f, 0.0f};
        } else if (op < H_UN) {
            R = hd_binary<false>(op, load(h - 1), load(h - 2));
            h -= 2;
        } else if (op < H_IF) {
            R = hd_unary<false>(op, load(h - 1));
            h -= 1;
        } else {
            R = stk[((h - 1) * 4) * kWave] > 0.0f ? load(h - 2) : load(h - 3);
            h -= 3;
        }
        stk[(h * 4) * kWave] = R.v; stk[(h * 4 + 1) * kWave] = R.ta; stk[(h * 4 + 2) * kWave] = R.tb; stk[(h * 4 + 3) * kWave] = R.tab;
        ++h;
    }
    return load(h - 1);   // (a TREE_OK tree ends at height 1)
}

// ---- the kernel.  VL: the register tuple of the X row (0: HessStrided).  BUILD 0: LEAN, 1: FULL, 2: DEEP -----------------------------------
template <int VL, int BUILD>
__global__ __launch_bounds__(kHessWaves * 64) void sr_hessian_kernel(HessParams p) {
    constexpr bool LEAN = BUILD == 0, DEEP = BUILD == 2;
    using VARS = typename std::conditional<VL == 0, HessStrided, HessTuple<VL == 0 ? 16 : VL>>::type;
    extern __shared__ __attribute__((aligned(16))) float hess_x[];   // [W][var_len][64] (x_in_lds)
    __shared__ uint32_t dec_s[2][kMaxStack];
    __shared__ double acc_s[kHessWaves][kHessCols][kWave];           // (fused) the lanes' float64 sums
    __shared__ double part_s[kHessWaves][kHessCols];
    __shared__ int bad_s[kHessWaves];
    __shared__ int viol_s[kHessWaves][kHessMaxPairs];

    if (BUILD == 1 && uni((int)p.flags[2]) == 0) return;
    if (DEEP && uni((int)p.flags[1]) == 0) return;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;
    const int P = p.P, D = p.D;
    const bool fused = p.loss != nullptr;
    const float nan = __builtin_nanf("");
    float *const dstack = DEEP ? p.deep + ((size_t)blockIdx.x * W + w) * (size_t)(p.gp_len + 2) * 4 * kWave + lane : nullptr;

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        if (BUILD == 1 && uni(p.cls[t]) != TREE_HEAVY) continue;
        if (DEEP && uni(p.cls[t]) != TREE_DEEP) continue;
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *ty = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int c = uni(classify_tree(ty, tv, len, false, p.var_len, 1, DEEP ? kMaxStack : kHessDepth, LEAN ? 1 : 0));
        if (LEAN && threadIdx.x == 0) p.cls[t] = c;
        if (c != TREE_OK) {
            if (c == TREE_BAD) {   // malformed: NaN rows (materialising); NaN columns and D violations (fused)
                if (fused) {
                    if ((int)threadIdx.x <= P) p.loss[(size_t)t * (1 + P) + threadIdx.x] = nan;
                    if ((int)threadIdx.x < P) p.viol[(size_t)t * P + threadIdx.x] = D;
                } else {
                    for (int d = threadIdx.x; d < D; d += blockDim.x) {
                        p.pred[(size_t)t * D + d] = nan;
                        for (int k = 0; k < P; ++k) p.dpred[((size_t)k * p.pop + t) * D + d] = nan;
                    }
                }
            } else if (threadIdx.x == 0) {
                if (c == TREE_DEEP) { p.cls[t] = TREE_DEEP; p.flags[1] = 1u; }
                else p.flags[2] = 1u;
            }
            continue;
        }

        // ---- decode once per tree ----
        uint32_t opv = 0, payv = 0;
        const bool in_regs = !DEEP && len <= kWave;
        if (in_regs) {
            if (lane < len) {
                const int i = len - 1 - lane;
                const Decoded dn = decode_node(ty[i], tv[i], false, p.var_len, 1);
                opv = dn.op; payv = dn.pay;
            }
        } else {
            for (int r = threadIdx.x; r < len; r += blockDim.x) {
                const int i = len - 1 - r;
                const Decoded dn = decode_node(ty[i], tv[i], false, p.var_len, 1);
                dec_s[0][r] = dn.op; dec_s[1][r] = dn.pay;
            }
            __syncthreads();
        }
        // bit k: the tree holds both variables of pair k (wave-uniform)
        unsigned present = 0;
        for (int k = 0; k < P; ++k) {
            const uint32_t va = (uint32_t)p.va[k], vb = (uint32_t)p.vb[k];
            bool ha = false, hb = false;
            for (int base = 0; base < len; base += kWave) {
                uint32_t o = opv, q = payv;
                if (!in_regs) {
                    const int r = base + lane;
                    o = r < len ? dec_s[0][r] : 0u;
                    q = r < len ? dec_s[1][r] : 0u;
                }
                ha = ha || __any(o == H_VAR && q == va);
                hb = hb || __any(o == H_VAR && q == vb);
            }
            if (ha && hb) present |= 1u << k;
        }
        // one interpretation of the tree on the lane's row: the pair (va, vb), or kHessNoVar for the plain one
        auto interpret = [&](const VARS &vars, uint32_t va, uint32_t vb) -> HyperDual {
            if constexpr (DEEP) {
                return run_deep_hd(dec_s[0], dec_s[1], len, dstack, vars, va, vb);
            } else {
                RegStack<4, kHessDepth> st;
                st.h = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) st.tos[k] = 0.0f;
                for (int base = 0; base < len; base += kWave) {
                    uint32_t o = opv, q = payv;
                    if (!in_regs) {
                        const int r = base + lane;
                        o = r < len ? dec_s[0][r] : 0u;
                        q = r < len ? dec_s[1][r] : 0u;
                    }
                    const int n = len - base < kWave ? len - base : kWave;
                    run_chunk_hd<LEAN>(o, q, n, st, vars, va, vb);
                }
                return HyperDual{st.tos[0], st.tos[1], st.tos[2], st.tos[3]};
            }
        };

        if (fused) {
#pragma unroll
            for (int k = 0; k < kHessCols; ++k) acc_s[w][k][lane] = 0.0;
        }
        int vcnt = 0;   // (fused) lane k < P: the violating rows of pair k in this wave's tiles
        int bad = 0;    // (fused) bit c: a row term of column c was not finite
        for (int tile = w; tile < p.ntiles; tile += W) {
            const long long d = (long long)tile * kWave + lane;   // (64 bits: D may lie within a tile of INT_MAX)
            const bool valid = d < D;
            const size_t dc = (size_t)(valid ? d : D - 1);        // lanes past the end repeat the last row
            const float *xr = p.X + dc * p.var_len;
            VARS vars;
            if constexpr (VL == 0) {
                if (p.x_in_lds) {
                    float *xs = hess_x + (size_t)w * p.var_len * kWave + lane;
                    for (int v = 0; v < p.var_len; ++v) xs[v * kWave] = xr[v];
                    vars.base = xs; vars.stride = kWave;
                } else {
                    vars.base = xr; vars.stride = 1;
                }
            } else {
#pragma unroll
                for (int v = 0; v < VL; ++v) vars.v[v] = v < p.var_len ? xr[v] : 0.0f;
            }
            float pred = 0.0f;
            bool have_pred = false;
#pragma unroll 1
            for (int k = 0; k < P; ++k) {
                float hk = 0.0f;   // +0.0f exactly for a pair the tree lacks
                if ((present >> k) & 1u) {
                    const HyperDual R = interpret(vars, (uint32_t)p.va[k], (uint32_t)p.vb[k]);
                    hk = R.tab;
                    if (!have_pred) { pred = R.v; have_pred = true; }
                }
                if (fused) {
                    const float label = p.dy ? p.dy[dc * P + k] : 0.0f;
                    const double e = (double)hk - (double)label;
                    const double tk = e * e;
                    acc_s[w][1 + k][lane] += valid ? tk : 0.0;
                    bad |= valid && !__builtin_isfinite(tk) ? 2 << k : 0;
                    const float lo = p.dmin ? p.dmin[k] : -__builtin_inff(), hi = p.dmax ? p.dmax[k] : __builtin_inff();
                    const int nv = __popcll(__ballot(valid && !(lo <= hk && hk <= hi)));
                    vcnt += lane == k ? nv : 0;
                } else if (valid) {
                    p.dpred[((size_t)k * p.pop + t) * D + d] = hk;
                }
            }
            if (!have_pred) pred = interpret(vars, kHessNoVar, kHessNoVar).v;
            if (fused) {
                const double r = (double)pred - (double)p.y[dc];
                const double t0 = r * r;
                acc_s[w][0][lane] += valid ? t0 : 0.0;
                bad |= valid && !__builtin_isfinite(t0) ? 1 : 0;
            } else if (valid) {
                p.pred[(size_t)t * D + d] = pred;
            }
        }

        if (fused) {
            // ---- reduce: lanes by the fixed butterfly, waves in wave order ----
            int wbad = 0;
            for (int k = 0; k <= P; ++k) {
                const double s = wave_sum_d(acc_s[w][k][lane]);
                if (lane == 0) part_s[w][k] = s;
                if (__any((bad >> k) & 1)) wbad |= 1 << k;
            }
            if (lane == 0) bad_s[w] = wbad;
            if (lane < P) viol_s[w][lane] = vcnt;
            __syncthreads();
            const int k = (int)threadIdx.x;
            const int nw = p.ntiles < W ? p.ntiles : W;
            if (k <= P) {
                double s = 0.0;
                int anybad = 0;
                for (int i = 0; i < nw; ++i) { s += part_s[i][k]; anybad |= bad_s[i]; }
                p.loss[(size_t)t * (1 + P) + k] = (anybad >> k) & 1 ? nan : (float)(s / (double)D);
            }
            if (k < P) {
                int n = 0;
                for (int i = 0; i < nw; ++i) n += viol_s[i][k];
                p.viol[(size_t)t * P + k] = n;
            }
        }
        __syncthreads();   // dec_s and the partial sums are rewritten for the next tree
    }
}

// ---- the launch --------------------------------------------------------------------------------------------------------------------------
struct HessPlan { unsigned W, blocks, deep_blocks; size_t lds; int x_in_lds; };

// W and the blocks depend on (pop, D, var_len) and the device alone: the order of the float64 sums is fixed by them
static HessPlan hess_plan(int pop, int D, int var_len) {
    const DeviceInfo &dev = device_info();
    const int ntiles = (int)(((long long)D + kWave - 1) / kWave);
    unsigned W = ntiles < kHessWaves ? (unsigned)ntiles : (unsigned)kHessWaves;
    const int x_in_lds = var_len > 32 && var_len <= kHessLdsVars;
    const size_t per_wave = x_in_lds ? (size_t)var_len * kWave * sizeof(float) : 0;
    while (W > 1 && W * per_wave > kHessLdsX) --W;
    long blocks = (long)dev.num_cus * 32;
    if (blocks > pop) blocks = pop;
    long deep = (long)dev.num_cus / (long)W;
    if (deep < 1) deep = 1;
    if (deep > pop) deep = pop;
    return {W, (unsigned)blocks, (unsigned)deep, W * per_wave, x_in_lds};
}

template <int VL>
static hipError_t launch_hessian_builds(const HessParams &p, const HessPlan &plan, hipStream_t stream) {
    hipLaunchKernelGGL((sr_hessian_kernel<VL, 0>), dim3(plan.blocks), dim3(plan.W * 64), VL == 0 ? plan.lds : 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((sr_hessian_kernel<VL, 1>), dim3(plan.blocks), dim3(plan.W * 64), VL == 0 ? plan.lds : 0, stream, p);
    return hipGetLastError();
}

// The pair codes of wrt -> (a, b); EVOGP_E_BADARG for an entry that is no pair code, stray bits, a > b, an index outside [0, var_len)
// or a repeated code.  n_wrt is already in 1 .. 8.
static int hess_pairs(unsigned var_len, unsigned n_wrt, const int *wrt, HessParams *p) {
    for (unsigned k = 0; k < n_wrt; ++k) {
        const unsigned code = (unsigned)wrt[k];
        if ((code >> 30) != 1u) return EVOGP_E_BADARG;
        const unsigned a = (code >> 15) & 0x7FFFu, b = code & 0x7FFFu;
        if (a > b || b >= var_len) return EVOGP_E_BADARG;
        for (unsigned j = 0; j < k; ++j)
            if (wrt[j] == wrt[k]) return EVOGP_E_BADARG;
        p->va[k] = (int)a; p->vb[k] = (int)b;
    }
    return EVOGP_OK;
}

// Both forms: (pred, dpred) or (loss, viol) is null.  The workspace is the per-stream block the tape kernels use.
int hessian_run(unsigned pop, unsigned D, unsigned gp_len, unsigned var_len, const float *value, const int16_t *type, const int16_t *size,
                const float *X, const float *y, const float *dy, const float *dmin, const float *dmax, unsigned n_wrt, const int *wrt,
                float *pred, float *dpred, float *loss, int *viol, hipStream_t stream) {
    HessParams p{};
    p.value = value; p.type = type; p.size = size; p.X = X; p.y = y; p.dy = dy; p.dmin = dmin; p.dmax = dmax;
    p.pred = pred; p.dpred = dpred; p.loss = loss; p.viol = viol;
    p.pop = (int)pop; p.D = (int)D; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    if (const int rc = hess_pairs(var_len, n_wrt, wrt, &p)) return rc;
    p.P = (int)n_wrt;
    for (int k = p.P; k < kHessMaxPairs; ++k) p.va[k] = p.vb[k] = -1;
    p.ntiles = (int)(((long long)p.D + kWave - 1) / kWave);
    const HessPlan plan = hess_plan(p.pop, p.D, p.var_len);
    p.x_in_lds = plan.x_in_lds;
    Arena sizes{nullptr};
    sizes.take<int>((size_t)p.pop);
    sizes.take<float>((size_t)plan.deep_blocks * plan.W * (size_t)(p.gp_len + 2) * 4 * kWave);
    int rc = 0;
    float *ws = grad_workspace(stream, sizes.off, &rc);
    if (!ws) return rc;
    Arena a{(char *)ws};
    p.cls = a.take<int>((size_t)p.pop);
    p.deep = a.take<float>((size_t)plan.deep_blocks * plan.W * (size_t)(p.gp_len + 2) * 4 * kWave);
    hipError_t e;
    p.flags = acquire_counter(stream, &e);
    if (!p.flags) return (int)e;
    e = p.var_len <= 16 ? launch_hessian_builds<16>(p, plan, stream)
        : p.var_len <= 32 ? launch_hessian_builds<32>(p, plan, stream) : launch_hessian_builds<0>(p, plan, stream);
    if (e != hipSuccess) return (int)e;
    // (the DEEP build exists with the strided row only: its X block is sized by its own plan.W waves)
    HessParams q = p;
    q.x_in_lds = p.var_len <= kHessLdsVars;
    const size_t lds = q.x_in_lds ? (size_t)plan.W * p.var_len * kWave * sizeof(float) : 0;
    hipLaunchKernelGGL((sr_hessian_kernel<0, 2>), dim3(plan.deep_blocks), dim3(plan.W * 64), lds, stream, q);
    return (int)hipGetLastError();
}

}  // namespace evogp
