// sr_simulate_sens.hip — constant tuning under simulation fitness: the forward sensitivities s_k = d x / d c_k of a simulated trajectory in the
// tree's optimised constants, carried through time INSIDE one kernel by a dual-number build of the register interpreter (gfx950; no
// counterpart in the reference).  include/evogp_hip.h has the definition (evogp_hip_sr_simulation_sensitivities /
// evogp_hip_sr_simulation_normal_eq); DESIGN.md 3.34 the design.
//
//   s_k+ = J_x(x, u) s_k + d f / d c_k   is ONE interpretation of the tree on dual numbers: a state variable v < S is seeded with s[v][k],
//                                        the CONST node of constant k with 1, everything else with 0.  No tape: a gradient by the tape
//                                        kernels (sr_grad.hip) would be paid at every step and stage of every trajectory.
//   0. sens_transpose_kernel   sr_simulate.hip's: u and target -> [t][column][b]
//   1. sr_sim_sens_kernel      sr_simulate_kernel's split: one workgroup per tree, wave w takes the tiles w, w + W, ... of 64 trajectories, a
//                              lane per trajectory, the tree classified and decoded ONCE (the (opv, payv) pair up to 64 nodes, LDS beyond),
//                              the loads of step t + 1 issued before step t is interpreted.  A stack entry is a value and NT tangents
//                              (RegStack<1 + NT, 16>: 80 VGPRs at NT = 4); a stage runs ceil(nc / NT) interpretations, each owning NT
//                              COLUMNS of the sensitivity matrix.  The matrix s[S][K] -- and for rk4 the stage tangent and the tangent of
//                              the running sum -- lives in the wave's LDS block [s][k][lane]: every access is the lane's own word, so no
//                              barrier and no bank conflict; registers hold only the NT tangents in flight and the 44 accumulators.
//                              LEAN / FULL builds as in sr_simulate.hip; the DEEP build (one wave per tree, NT = 1, the operand stack a
//                              [entry][lane] block of the workspace) takes the trees too deep for 16 registers with the SAME node rules
//                              and the same order of summation: a tree gives the same bits whichever build takes it.
// The primal is computed by the functions sr_simulate.hip's interpreter calls, so the states and the float64 loss are its bits.
// Tangent rule (one written rule, sr_adjoint.hpp's pinned table with g = 1, every operation rounded separately):
//   binary  t_r = fadd(fmul(pa, t_a), fmul(pb, t_b)), (pa, pb) = binary_adjoint(op, a, b, r, 1);  unary  t_r = fmul(unary_adjoint(op, a, r, 1), t_a)
//   IF: the tangent of the branch taken;  comparisons and unknown ids: 0;  ADD, SUB, NEG: the shortcuts with the same bits.
#include "sr_adjoint.hpp"
#include "sr_moments.hpp"

namespace evogp {

constexpr int kSensWaves = 4;                      // waves per workgroup: the tiles of one tree
constexpr int kSensDepth = 16;                     // register stack entries (of 1 + NT words each)
constexpr int kSensNT = 4;                         // tangents per interpretation
constexpr int kSensK = kLmMaxConsts;               // optimised constants per tree
constexpr int kSensS = EVOGP_SIM_MAX_STATE;
constexpr int kSensTri = kSensK * (kSensK + 1) / 2;
constexpr int kSensWords = kSensTri + kSensK;      // a row of `normal`
constexpr int kSensStaticLds = 12 * 1024;          // upper bound of the kernel's static LDS (10.3 KiB), for the launch plan
static_assert(kSensWords == EVOGP_LM_NORMAL_WORDS && kSensK % kSensNT == 0 && kSensS <= 9, "layout");

typedef float v9f_t __attribute__((ext_vector_type(9)));

struct SensParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *x0;      // [B][S]
    const float *ut;      // [T][U][B]
    const float *tt;      // [T][SC][B] (the fused form)
    const float *wgt;     // [SC] state weights (the fused form)
    float *states;        // [pop][B][T][S]     the materialising form, or nullptr
    float *sens;          // [pop][B][T][S][K]
    double *loss64;       // [pop][SC]          the fused form, or nullptr
    float *loss32;        // [pop]
    float *normal;        // [pop][44]
    float *deep;          // [deep blocks][2][gp_len + 2][64]: the operand stacks of the DEEP build
    int *cls;
    unsigned *flags;      // [1] != 0: some tree is TREE_DEEP, [2] != 0: some tree is TREE_HEAVY
    int pop, gp_len, B, T, S, U, SC, ntiles, scheme;
    float dt, h2, h6;
};

// ---- 0. the transposition (sr_simulate.hip's sim_transpose_kernel) ----------------------------------------------------------------------
static __global__ __launch_bounds__(256) void sens_transpose_kernel(const float *u, float *ut, int U, const float *target, float *tt, int SC, int B, int T) {
    const size_t nu = (size_t)B * T * U, nt = target ? (size_t)B * T * SC : 0;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < nu + nt; o += (size_t)gridDim.x * blockDim.x) {
        const bool first = o < nu;
        const size_t e = first ? o : o - nu;
        const int C = first ? U : SC;
        const size_t b = e % (size_t)B, r = e / (size_t)B, c = r % (size_t)C, t = r / (size_t)C;
        const size_t from = (b * T + t) * C + c;
        if (first) ut[e] = u[from];
        else tt[e] = target[from];
    }
}

// sr_lm.hip's find_optimised_consts: the first kSensK CONST nodes of [0, len) in prefix order -> cidx (this wave's LDS), -1 beyond nc
__device__ inline int sens_find_consts(const int16_t *type_row, int len, int *cidx) {
    const int lane = threadIdx.x & 63;
    int nc = 0;
    for (int base = 0; base < len && nc < kSensK; base += kWave) {
        const int i = base + lane;
        unsigned long long m = __ballot(i < len && type_row[i] == T_CONST);
        while (m != 0 && nc < kSensK) {
            const int bit = __ffsll((long long)m) - 1;
            if (lane == 0) cidx[nc] = base + bit;
            m &= m - 1;
            ++nc;
        }
    }
    if (lane == 0)
        for (int j = nc; j < kSensK; ++j) cidx[j] = -1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return nc;
}

// ---- the node rules on dual numbers -------------------------------------------------------------------------------------------------------
// The LEAN build names the operations it can meet, so the table's transcendental rows are not compiled into it.
template <bool LEAN>
__device__ inline void binary_partials(uint32_t op, float a, float b, float r, float &pa, float &pb) {
    switch (op) {
    case H_MUL: binary_adjoint(H_MUL, a, b, r, 1.0f, pa, pb); break;
    case H_DIV: binary_adjoint(H_DIV, a, b, r, 1.0f, pa, pb); break;
    case H_BIN_OTHER + (F_LOOSE_DIV - F_LOOSE_DIV): binary_adjoint(H_BIN_OTHER + (F_LOOSE_DIV - F_LOOSE_DIV), a, b, r, 1.0f, pa, pb); break;
    case H_BIN_OTHER + (F_MAX - F_LOOSE_DIV): binary_adjoint(H_BIN_OTHER + (F_MAX - F_LOOSE_DIV), a, b, r, 1.0f, pa, pb); break;
    case H_BIN_OTHER + (F_MIN - F_LOOSE_DIV): binary_adjoint(H_BIN_OTHER + (F_MIN - F_LOOSE_DIV), a, b, r, 1.0f, pa, pb); break;
    default:
        pa = 0.0f; pb = 0.0f;
        if (!LEAN) binary_adjoint(op, a, b, r, 1.0f, pa, pb);
    }
}

template <bool LEAN>
__device__ inline float unary_partial(uint32_t op, float a, float r) {
    switch (op) {
    case H_UN + (F_INV - F_SIN): return unary_adjoint(H_UN + (F_INV - F_SIN), a, r, 1.0f);
    case H_UN + (F_LOOSE_INV - F_SIN): return unary_adjoint(H_UN + (F_LOOSE_INV - F_SIN), a, r, 1.0f);
    case H_UN + (F_ABS - F_SIN): return unary_adjoint(H_UN + (F_ABS - F_SIN), a, r, 1.0f);
    case H_UN + (F_SQRT - F_SIN): return unary_adjoint(H_UN + (F_SQRT - F_SIN), a, r, 1.0f);
    case H_UN + (F_LOOSE_SQRT - F_SIN): return unary_adjoint(H_UN + (F_LOOSE_SQRT - F_SIN), a, r, 1.0f);
    default: return LEAN ? 0.0f : unary_adjoint(op, a, r, 1.0f);
    }
}

template <bool LEAN, int NT>
__device__ inline float dual_binary(uint32_t op, float a, const float (&ta)[NT], float b, const float (&tb)[NT], float (&tr)[NT]) {
    const float r = op == H_ADD ? a + b : op == H_SUB ? a - b : op == H_MUL ? a * b
                    : op == H_DIV ? (b == 0.0f ? __builtin_nanf("") : a / b) : op_binary_other<LEAN>(op, a, b);
    if (op == H_ADD) {
#pragma unroll
        for (int i = 0; i < NT; ++i) tr[i] = __fadd_rn(ta[i], tb[i]);
    } else if (op == H_SUB) {
#pragma unroll
        for (int i = 0; i < NT; ++i) tr[i] = __fsub_rn(ta[i], tb[i]);
    } else if (op >= H_BIN_OTHER + (F_LT - F_LOOSE_DIV)) {   // the comparisons, an unknown id
#pragma unroll
        for (int i = 0; i < NT; ++i) tr[i] = 0.0f;
    } else {
        float pa, pb;
        binary_partials<LEAN>(op, a, b, r, pa, pb);
#pragma unroll
        for (int i = 0; i < NT; ++i) tr[i] = __fadd_rn(__fmul_rn(pa, ta[i]), __fmul_rn(pb, tb[i]));
    }
    return r;
}

template <bool LEAN, int NT>
__device__ inline float dual_unary(uint32_t op, float a, const float (&ta)[NT], float (&tr)[NT]) {
    const float r = op_unary<LEAN>(op, a);
    if (op == H_UN + (F_NEG - F_SIN)) {
#pragma unroll
        for (int i = 0; i < NT; ++i) tr[i] = -ta[i];
    } else if (op == H_UN_ZERO) {
#pragma unroll
        for (int i = 0; i < NT; ++i) tr[i] = 0.0f;
    } else {
        const float pa = unary_partial<LEAN>(op, a, r);
#pragma unroll
        for (int i = 0; i < NT; ++i) tr[i] = __fmul_rn(pa, ta[i]);
    }
    return r;
}

// What seeds the leaves of one interpretation: columns k0 .. k0 + NT - 1 of the matrix `src` (the lane's words, [v][k] 64 floats apart)
// for the state variables, and the execution positions of those constants' CONST nodes (an absent constant: a position no node has).
template <int NT>
struct DualSeeds {
    const float *src;
    int S, k0;
    int cpos[NT];
};

// ---- run_chunk (interp.hpp) on dual numbers: rows 0 of the stack and of outs are the primal, rows 1 .. NT the tangents ----------------------
template <bool MO, bool LEAN, int NT, class VA>
__device__ inline void run_chunk_dual(uint32_t opv, uint32_t payv, int n, int base, RegStack<1 + NT, kSensDepth> &st, const VA &vars,
                                      const DualSeeds<NT> &sd, v9f_t (&outs)[1 + NT]) {
    uint32_t next_op = (uint32_t)__builtin_amdgcn_readlane((int)opv, 0);
    for (int j = 0; j < n; ++j) {
        const uint32_t op = next_op;
        next_op = (uint32_t)__builtin_amdgcn_readlane((int)opv, (j + 1) & 63);
        if (op < H_ADD) {
            const uint32_t pay = (uint32_t)__builtin_amdgcn_readlane((int)payv, j);
            const int h = st.h;
            st.h = h + 1;
#pragma unroll
            for (int k = 0; k <= NT; ++k) st.s[k][h] = st.tos[k];
            if (op == H_CONST) {
                st.tos[0] = bits2f(pay);
#pragma unroll
                for (int i = 0; i < NT; ++i) st.tos[1 + i] = base + j == sd.cpos[i] ? 1.0f : 0.0f;
            } else {
                st.tos[0] = vars.get(0, pay);
                if (pay < (uint32_t)sd.S) {
#pragma unroll
                    for (int i = 0; i < NT; ++i) st.tos[1 + i] = sd.src[(pay * kSensK + sd.k0 + i) * kWave];
                } else {
#pragma unroll
                    for (int i = 0; i < NT; ++i) st.tos[1 + i] = 0.0f;
                }
            }
        } else if (op < H_UN) {   // a = top (left operand), b = next
            const int h = st.h - 1;
            st.h = h;
            float ta[NT], tb[NT], tr[NT];
            const float a = st.tos[0], b = st.s[0][h];
#pragma unroll
            for (int i = 0; i < NT; ++i) { ta[i] = st.tos[1 + i]; tb[i] = st.s[1 + i][h]; }
            if (MO) {
                const uint32_t pay = (uint32_t)__builtin_amdgcn_readlane((int)payv, j);
                if (pay != kNoOut) {
                    const float r = dual_binary<LEAN, NT>(op, a, ta, b, tb, tr);
                    outs[0][pay] += r;
#pragma unroll
                    for (int i = 0; i < NT; ++i) outs[1 + i][pay] = __fadd_rn(outs[1 + i][pay], tr[i]);
                }
                st.tos[0] = b;   // the LAST popped operand goes to the parent
#pragma unroll
                for (int i = 0; i < NT; ++i) st.tos[1 + i] = tb[i];
            } else {
                st.tos[0] = dual_binary<LEAN, NT>(op, a, ta, b, tb, tr);
#pragma unroll
                for (int i = 0; i < NT; ++i) st.tos[1 + i] = tr[i];
            }
        } else if (op < H_IF) {
            float ta[NT], tr[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) ta[i] = st.tos[1 + i];
            if (MO) {
                const uint32_t pay = (uint32_t)__builtin_amdgcn_readlane((int)payv, j);
                if (pay != kNoOut) {
                    const float r = dual_unary<LEAN, NT>(op, st.tos[0], ta, tr);
                    outs[0][pay] += r;
#pragma unroll
                    for (int i = 0; i < NT; ++i) outs[1 + i][pay] = __fadd_rn(outs[1 + i][pay], tr[i]);
                }
            } else {
                st.tos[0] = dual_unary<LEAN, NT>(op, st.tos[0], ta, tr);
#pragma unroll
                for (int i = 0; i < NT; ++i) st.tos[1 + i] = tr[i];
            }
        } else {   // IF: cond = top, then = next, else = third; the condition's tangent is dropped
            const int h = st.h - 2;
            st.h = h;
            uint32_t pay = kNoOut;
            if (MO) pay = (uint32_t)__builtin_amdgcn_readlane((int)payv, j);
            const bool take_b = st.tos[0] > 0.0f;
#pragma unroll
            for (int k = 0; k <= NT; ++k) {
                const float b = st.s[k][h + 1], c = st.s[k][h];
                const float r = take_b ? b : c;
                if (MO) {
                    if (pay != kNoOut) outs[k][pay] = k == 0 ? outs[k][pay] + r : __fadd_rn(outs[k][pay], r);
                    st.tos[k] = c;
                } else {
                    st.tos[k] = r;
                }
            }
        }
    }
}

// ---- run_general (interp.hpp) on dual numbers, ONE tangent: the stack is the lane's column of two [entry][64] blocks -----------------------
template <bool MO, class VA>
__device__ inline void run_deep_dual(const uint32_t *dop, const uint32_t *dpay, int len, float *sv, float *sg, const VA &vars,
                                     const DualSeeds<1> &sd, v9f_t (&outs)[2], float &root, float &root_t) {
    int h = 0;
    for (int r = 0; r < len; ++r) {
        const uint32_t op = uni(dop[r]), pay = uni(dpay[r]);
        float v, g[1];
        if (op < H_ADD) {
            if (op == H_CONST) { v = bits2f(pay); g[0] = r == sd.cpos[0] ? 1.0f : 0.0f; }
            else { v = vars.get(0, pay); g[0] = pay < (uint32_t)sd.S ? sd.src[(pay * kSensK + sd.k0) * kWave] : 0.0f; }
            sv[h * kWave] = v; sg[h * kWave] = g[0];
            ++h;
            continue;
        }
        float last, last_t;
        if (op < H_UN) {
            const float a = sv[(h - 1) * kWave], b = sv[(h - 2) * kWave];
            const float ta[1] = {sg[(h - 1) * kWave]}, tb[1] = {sg[(h - 2) * kWave]};
            h -= 2;
            v = dual_binary<false, 1>(op, a, ta, b, tb, g);
            last = b; last_t = tb[0];
        } else if (op < H_IF) {
            --h;
            const float a = sv[h * kWave];
            const float ta[1] = {sg[h * kWave]};
            v = dual_unary<false, 1>(op, a, ta, g);
            last = a; last_t = ta[0];
        } else {
            const float a = sv[(h - 1) * kWave], b = sv[(h - 2) * kWave], c = sv[(h - 3) * kWave];
            const float tb = sg[(h - 2) * kWave], tc = sg[(h - 3) * kWave];
            h -= 3;
            v = a > 0.0f ? b : c; g[0] = a > 0.0f ? tb : tc;
            last = c; last_t = tc;
        }
        if (MO) {
            if (pay != kNoOut) { outs[0][pay] += v; outs[1][pay] = __fadd_rn(outs[1][pay], g[0]); }
            v = last; g[0] = last_t;
        }
        sv[h * kWave] = v; sg[h * kWave] = g[0];
        ++h;
    }
    root = h > 0 ? sv[(h - 1) * kWave] : 0.0f;
    root_t = h > 0 ? sg[(h - 1) * kWave] : 0.0f;
}

__device__ inline void sens_store_bad(const SensParams &p, int t) {
    const float nan = __builtin_nanf("");
    const size_t n = (size_t)p.B * p.T * p.S;
    if (p.states) {
        for (size_t i = threadIdx.x; i < n; i += blockDim.x) p.states[(size_t)t * n + i] = nan;
        for (size_t i = threadIdx.x; i < n * kSensK; i += blockDim.x) p.sens[(size_t)t * n * kSensK + i] = nan;
    } else {
        if ((int)threadIdx.x < p.SC) p.loss64[(size_t)t * p.SC + threadIdx.x] = __builtin_nan("");
        if (threadIdx.x < (unsigned)kSensWords) p.normal[(size_t)t * kSensWords + threadIdx.x] = 0.0f;
        if (threadIdx.x == 0) p.loss32[t] = nan;
    }
}

// Words of one wave's LDS block: the sensitivity matrix and, for rk4, the stage tangent and the tangent of the running sum
__host__ __device__ inline int sens_wave_words(int S, int scheme) { return (scheme == EVOGP_SIM_RK4 ? 3 : 1) * S * kSensK * kWave; }

// ---- 1. the kernel.  KIND 0: one state (map / euler / rk4), 1: several states (the multi-output forest), 2: narx.  BUILD 0: LEAN, 1: FULL, 2: DEEP
template <int VL, int KIND, int BUILD>
__global__ __launch_bounds__(kSensWaves * 64) void sr_sim_sens_kernel(SensParams p) {
    using VARS = typename VecOf<VL>::type;
    constexpr bool MO = KIND == 1, NARX = KIND == 2, LEAN = BUILD == 0, DEEP = BUILD == 2;
    constexpr int NS = KIND == 0 ? 1 : kSensS;   // state registers
    constexpr int NK = MO ? kSensS : 1;          // values of one interpretation
    constexpr int NT = DEEP ? 1 : kSensNT;
    extern __shared__ __attribute__((aligned(16))) float sens_lds[];
    __shared__ uint32_t dec_s[2][kMaxStack];
    __shared__ double part_d[2][kSensWaves][kSensS];
    __shared__ float part_f[2][kSensWaves][kSensWords];
    __shared__ int dead_s[2][kSensWaves];
    __shared__ int cidx_s[kSensWaves][kSensK];

    if (BUILD == 1 && uni((int)p.flags[2]) == 0) return;
    if (DEEP && uni((int)p.flags[1]) == 0) return;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;
    const int S = p.S, SC = p.SC, T = p.T, B = p.B;
    const int scheme = NARX ? EVOGP_SIM_NARX : p.scheme;
    const bool rk4 = scheme == EVOGP_SIM_RK4;
    const int nstage = rk4 ? 4 : 1;
    const int var_len = S + p.U, out_len = MO ? S : 1;
    const float nan = __builtin_nanf("");
    const bool fused = p.loss64 != nullptr;
    const int mat = S * kSensK * kWave;
    float *const mS = sens_lds + (size_t)w * sens_wave_words(S, scheme) + lane;   // s[v][k]: mS[(v * K + k) * 64]
    float *const mT = mS + mat, *const mU = mT + mat;                             // rk4: the stage's tangent, the running sum's
    float *const dstack = DEEP ? p.deep + (size_t)blockIdx.x * 2 * (p.gp_len + 2) * kWave + lane : nullptr;
    float wgt[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) wgt[s] = fused && s < SC ? p.wgt[s] : 0.0f;

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        if (BUILD == 1 && uni(p.cls[t]) != TREE_HEAVY) continue;
        if (DEEP && uni(p.cls[t]) != TREE_DEEP) continue;
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *ty = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int c = uni(classify_tree(ty, tv, len, MO, var_len, out_len, DEEP ? kMaxStack : kSensDepth, LEAN ? 1 : 0));
        if (LEAN && threadIdx.x == 0) p.cls[t] = c;
        if (c != TREE_OK) {
            if (c == TREE_BAD) sens_store_bad(p, t);
            else if (threadIdx.x == 0) {
                if (c == TREE_DEEP) { p.cls[t] = TREE_DEEP; p.flags[1] = 1u; }
                else p.flags[2] = 1u;
            }
            continue;
        }
        const int nc = sens_find_consts(ty, len, cidx_s[w]);

        // ---- decode once per tree ----
        uint32_t opv = 0, payv = 0;
        const bool in_regs = !DEEP && len <= kWave;
        if (in_regs) {
            if (lane < len) {
                const int i = len - 1 - lane;
                const Decoded dn = decode_node(ty[i], tv[i], MO, var_len, out_len);
                opv = dn.op; payv = dn.pay;
            }
        } else {
            for (int r = threadIdx.x; r < len; r += blockDim.x) {
                const int i = len - 1 - r;
                const Decoded dn = decode_node(ty[i], tv[i], MO, var_len, out_len);
                dec_s[0][r] = dn.op; dec_s[1][r] = dn.pay;
            }
            __syncthreads();
        }
        // the plain interpretation (a tree without a constant): sr_simulate_kernel's
        auto interpret = [&](const VARS &tup, float (&k)[NK]) {
            RegStack<1, kSensDepth> st;
            st.h = 0;
            st.tos[0] = 0.0f;
            v16f outs[1];
            if (MO) outs[0] = 0.0f;
            for (int base = 0; base < len; base += kWave) {
                uint32_t o = opv, q = payv;
                if (!in_regs) {
                    const int r = base + lane;
                    o = r < len ? dec_s[0][r] : 0u;
                    q = r < len ? dec_s[1][r] : 0u;
                }
                const int n = len - base < kWave ? len - base : kWave;
                run_chunk<MO, LEAN, 1, kSensDepth>(o, q, n, st, TupleVars<VL>{tup}, outs);
            }
            if (MO) {
#pragma unroll
                for (int s = 0; s < NK; ++s) k[s] = outs[0][s];
            } else {
                k[0] = st.tos[0];
            }
        };
        // the dual interpretation of columns k0 .. k0 + NT - 1, the state variables seeded from `src`
        auto interpret_dual = [&](const VARS &tup, const float *src, int k0, float (&k)[NK], float (&kt)[NK][NT]) {
            DualSeeds<NT> sd;
            sd.src = src; sd.S = S; sd.k0 = k0;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int ci = uni(cidx_s[w][k0 + i]);
                sd.cpos[i] = ci < 0 ? len : len - 1 - ci;
            }
            v9f_t outs[1 + NT];
#pragma unroll
            for (int i = 0; i <= NT; ++i) outs[i] = 0.0f;
            float root[1 + NT];
            if constexpr (DEEP) {
                run_deep_dual<MO>(dec_s[0], dec_s[1], len, dstack, dstack + (size_t)(p.gp_len + 2) * kWave, TupleVars<VL>{tup}, sd, outs, root[0], root[1]);
            } else {
                RegStack<1 + NT, kSensDepth> st;
                st.h = 0;
#pragma unroll
                for (int i = 0; i <= NT; ++i) st.tos[i] = 0.0f;
                for (int base = 0; base < len; base += kWave) {
                    uint32_t o = opv, q = payv;
                    if (!in_regs) {
                        const int r = base + lane;
                        o = r < len ? dec_s[0][r] : 0u;
                        q = r < len ? dec_s[1][r] : 0u;
                    }
                    const int n = len - base < kWave ? len - base : kWave;
                    run_chunk_dual<MO, LEAN, NT>(o, q, n, base, st, TupleVars<VL>{tup}, sd, outs);
                }
#pragma unroll
                for (int i = 0; i <= NT; ++i) root[i] = st.tos[i];
            }
#pragma unroll
            for (int s = 0; s < NK; ++s) {
                k[s] = MO ? outs[0][s] : root[0];
#pragma unroll
                for (int i = 0; i < NT; ++i) kt[s][i] = MO ? outs[1 + i][s] : root[1 + i];
            }
        };

        double tot = 0.0;    // thread s < SC: the loss sum of state s over the tiles so far, in index order
        float totf = 0.0f;   // thread i < 44: word i of the normal equations likewise
        int any_dead = 0;
        const int rounds = (p.ntiles + W - 1) / W;
        for (int r = 0; r < rounds; ++r) {
            const int tile = r * W + w, par = r & 1;
            if (tile < p.ntiles) {
                const long long b = (long long)tile * kWave + lane;
                const bool valid = b < B;
                const size_t bc = (size_t)(valid ? b : B - 1);
                float x[NS], tg[NS], tgn[NS];
                double acc[NS];
                float A[kSensTri], bv[kSensK];
#pragma unroll
                for (int k = 0; k < kSensTri; ++k) A[k] = 0.0f;
#pragma unroll
                for (int k = 0; k < kSensK; ++k) bv[k] = 0.0f;
                VARS tup, nxt;
#pragma unroll
                for (int v = 0; v < VL; ++v) { tup[v] = 0.0f; nxt[v] = 0.0f; }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    x[s] = s < S ? p.x0[bc * S + s] : 0.0f;
                    acc[s] = 0.0; tg[s] = 0.0f; tgn[s] = 0.0f;
                }
                for (int e = 0; e < (rk4 ? 3 : 1) * S * kSensK; ++e) mS[e * kWave] = 0.0f;   // d x0 / d c = 0
                auto load_step = [&](int ts) {
#pragma unroll
                    for (int v = 0; v < VL; ++v)
                        if (v >= S && v < var_len) nxt[v] = p.ut[((size_t)ts * p.U + (v - S)) * B + bc];
                    if (fused) {
#pragma unroll
                        for (int s = 0; s < NS; ++s)
                            if (s < SC) tgn[s] = p.tt[((size_t)ts * SC + s) * B + bc];
                    }
                };
                load_step(0);
                bool alive = true;
                int ts = 0;
                for (; ts < T; ++ts) {
#pragma unroll
                    for (int v = 0; v < VL; ++v)
                        if (v >= S && v < var_len) tup[v] = nxt[v];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        tg[s] = tgn[s];
                        if (s < S) tup[s] = x[s];
                    }
                    if (ts + 1 < T) load_step(ts + 1);   // in flight while this step is interpreted
                    float xn[NS], sum[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) { xn[s] = 0.0f; sum[s] = 0.0f; }
#pragma unroll 1
                    for (int stage = 0; stage < nstage; ++stage) {
                        float k[NK];
                        const float h = stage == 2 ? p.dt : p.h2;
                        if (nc == 0) {
                            if constexpr (DEEP) {
                                float kt[NK][NT];
                                interpret_dual(tup, mS, 0, k, kt);
                            } else {
                                interpret(tup, k);
                            }
                        } else {
                            const float *src = rk4 && stage > 0 ? mT : mS;
#pragma unroll 1
                            for (int k0 = 0; k0 < nc; k0 += NT) {
                                float kt[NK][NT];
                                interpret_dual(tup, src, k0, k, kt);
                                // ---- the scheme on the tangents of these columns, in the primal's association ----
#pragma unroll
                                for (int i = 0; i < NT; ++i) {
                                    if (k0 + i >= nc) break;
                                    const int col = (k0 + i) * kWave;
                                    if (scheme == EVOGP_SIM_NARX) {
                                        for (int v = S - 1; v >= 1; --v) mS[v * kSensK * kWave + col] = mS[(v - 1) * kSensK * kWave + col];
                                        mS[col] = kt[0][i];
                                        continue;
                                    }
#pragma unroll
                                    for (int s = 0; s < NS; ++s) {
                                        if (s >= S) break;
                                        const int e = s * kSensK * kWave + col;
                                        const float g = kt[s < NK ? s : 0][i];
                                        if (scheme == EVOGP_SIM_MAP) mS[e] = g;
                                        else if (scheme == EVOGP_SIM_EULER) mS[e] = __fadd_rn(mS[e], __fmul_rn(p.dt, g));
                                        else {
                                            const float su = stage == 0 ? g : __fadd_rn(mU[e], stage == 3 ? g : __fmul_rn(2.0f, g));
                                            mU[e] = su;
                                            if (stage < 3) mT[e] = __fadd_rn(mS[e], __fmul_rn(h, g));
                                            else mS[e] = __fadd_rn(mS[e], __fmul_rn(p.h6, su));
                                        }
                                    }
                                }
                            }
                        }
                        // ---- the scheme on the primal: sr_simulate_kernel's lines ----
                        if (scheme == EVOGP_SIM_MAP) {
#pragma unroll
                            for (int s = 0; s < NS; ++s) xn[s] = k[s < NK ? s : 0];
                        } else if (scheme == EVOGP_SIM_EULER) {
#pragma unroll
                            for (int s = 0; s < NS; ++s) xn[s] = __fadd_rn(x[s], __fmul_rn(p.dt, k[s < NK ? s : 0]));
                        } else if (scheme == EVOGP_SIM_NARX) {
                            xn[0] = k[0];
#pragma unroll
                            for (int s = 1; s < NS; ++s) xn[s] = x[s - 1];
                        } else {
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const float ks = k[s < NK ? s : 0];
                                sum[s] = stage == 0 ? ks : __fadd_rn(sum[s], stage == 3 ? ks : __fmul_rn(2.0f, ks));
                                if (stage < 3) { if (s < S) tup[s] = __fadd_rn(x[s], __fmul_rn(h, ks)); }
                                else xn[s] = __fadd_rn(x[s], __fmul_rn(p.h6, sum[s]));
                            }
                        }
                    }
                    bool fin = true;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        if (s < S) fin = fin && finite_f(xn[s]);
                        x[s] = xn[s];
                    }
                    alive = alive && fin;
                    if (!fused) {
                        if (valid) {
                            const size_t at = (((size_t)t * B + (size_t)b) * T + ts) * S;
#pragma unroll
                            for (int s = 0; s < NS; ++s)
                                if (s < S) {
                                    p.states[at + s] = alive ? xn[s] : nan;
                                    for (int k = 0; k < kSensK; ++k)
                                        p.sens[(at + s) * kSensK + k] = !alive ? nan : k < nc ? mS[(s * kSensK + k) * kWave] : 0.0f;
                                }
                        }
                    } else if (alive && valid) {
#pragma unroll
                        for (int s = 0; s < NS; ++s)
                            if (s < SC) {
                                const double d = (double)xn[s] - (double)tg[s];
                                acc[s] += d * d;
                                if (nc > 0) {
                                    const float rf = __fsub_rn(xn[s], tg[s]);
                                    float J[kSensK];
#pragma unroll
                                    for (int i = 0; i < kSensK; ++i) J[i] = i < nc ? mS[(s * kSensK + i) * kWave] : 0.0f;
                                    int kk = 0;
#pragma unroll
                                    for (int i = 0; i < kSensK; ++i) {
                                        const float wJ = __fmul_rn(wgt[s], J[i]);
#pragma unroll
                                        for (int j = i; j < kSensK; ++j, ++kk)
                                            if (j < nc) A[kk] = __fadd_rn(A[kk], __fmul_rn(wJ, J[j]));
                                        if (i < nc) bv[i] = __fadd_rn(bv[i], __fmul_rn(wJ, rf));
                                    }
                                }
                            }
                    }
                    if (!__any(alive)) { ++ts; break; }   // every trajectory of the tile is dead: the result is decided
                }
                if (!fused) {
                    if (valid)
                        for (; ts < T; ++ts) {
                            const size_t at = (((size_t)t * B + (size_t)b) * T + ts) * S;
                            for (int s = 0; s < S; ++s) {
                                p.states[at + s] = nan;
                                for (int k = 0; k < kSensK; ++k) p.sens[(at + s) * kSensK + k] = nan;
                            }
                        }
                } else {
                    const bool dead = __any(!alive) != 0;
#pragma unroll
                    for (int s = 0; s < NS; ++s)
                        if (s < SC) {
                            const double sum_s = wave_sum_d(acc[s]);
                            if (lane == 0) part_d[par][w][s] = sum_s;
                        }
#pragma unroll
                    for (int k = 0; k < kSensTri; ++k) {
                        const float sk = wave_sum(A[k]);
                        if (lane == 0) part_f[par][w][k] = sk;
                    }
#pragma unroll
                    for (int k = 0; k < kSensK; ++k) {
                        const float sk = wave_sum(bv[k]);
                        if (lane == 0) part_f[par][w][kSensTri + k] = sk;
                    }
                    if (lane == 0) dead_s[par][w] = dead ? 1 : 0;
                }
            }
            if (fused) {
                __syncthreads();
                if (threadIdx.x < (unsigned)kWave) {
                    const int left = p.ntiles - r * W;
                    const int nw = left < W ? left : W;
                    for (int i = 0; i < nw; ++i) {
                        if ((int)threadIdx.x < SC) tot += part_d[par][i][threadIdx.x];
                        if (threadIdx.x < (unsigned)kSensWords) totf = __fadd_rn(totf, part_f[par][i][threadIdx.x]);
                        any_dead |= dead_s[par][i];
                    }
                }
            }
        }
        if (fused && w == 0) {
            const double l64 = any_dead ? __builtin_nan("") : tot / ((double)B * (double)T);
            if (lane < SC) p.loss64[(size_t)t * SC + lane] = l64;
            if (lane < kSensWords) p.normal[(size_t)t * kSensWords + lane] = any_dead ? 0.0f : totf / (float)(B * T);
            double ws = 0.0;   // the weighted loss, summed in index order
            for (int s = 0; s < SC; ++s) ws += (double)p.wgt[s] * __shfl(l64, s, kWave);
            if (lane == 0) p.loss32[t] = any_dead ? nan : (float)ws;
        }
        __syncthreads();   // dec_s and the partial sums are rewritten for the next tree
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
struct SensPlan { unsigned blocks, threads, deep_blocks; size_t lds, lds_deep; };

static SensPlan sens_plan(unsigned pop, unsigned B, unsigned S, int scheme) {
    const DeviceInfo &dev = device_info();
    const size_t per_wave = (size_t)sens_wave_words((int)S, scheme) * sizeof(float);   // at most 48 KiB
    const unsigned ntiles = (B + kWave - 1) / kWave;
    unsigned W = (unsigned)((dev.lds_per_cu - kSensStaticLds) / per_wave);             // at least 3
    if (W > (unsigned)kSensWaves) W = kSensWaves;
    if (W > ntiles) W = ntiles;
    long blocks = (long)dev.num_cus * 64;   // (not sized by residency: the hardware keeps as many resident as LDS and registers allow)
    if (blocks > (long)pop) blocks = (long)pop;
    long deep = (long)dev.num_cus;
    if (deep > (long)pop) deep = (long)pop;
    return {(unsigned)blocks, W * 64u, (unsigned)deep, (size_t)W * per_wave, per_wave};
}

template <int VL, int KIND, int BUILD>
static hipError_t launch_sens(const SensParams &p, unsigned blocks, unsigned threads, size_t lds, hipStream_t stream) {
    static LdsGrant grant;   // (one per instantiation)
    std::call_once(grant.once, [&] {
        grant.err = hipFuncSetAttribute((const void *)sr_sim_sens_kernel<VL, KIND, BUILD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        160 * 1024 - kSensStaticLds);
    });
    if (grant.err != hipSuccess) return grant.err;
    hipLaunchKernelGGL((sr_sim_sens_kernel<VL, KIND, BUILD>), dim3(blocks), dim3(threads), lds, stream, p);
    return hipGetLastError();
}

template <int VL, int KIND>
static hipError_t launch_sens_builds(const SensParams &p, const SensPlan &plan, hipStream_t stream) {
    hipError_t e = launch_sens<VL, KIND, 0>(p, plan.blocks, plan.threads, plan.lds, stream);
    if (e != hipSuccess) return e;
    if ((e = launch_sens<VL, KIND, 1>(p, plan.blocks, plan.threads, plan.lds, stream)) != hipSuccess) return e;
    return launch_sens<32, KIND, 2>(p, plan.deep_blocks, 64u, plan.lds_deep, stream);   // (the DEEP build exists at the widest tuple only)
}

template <int VL>
static hipError_t launch_sens_kind(const SensParams &p, const SensPlan &plan, hipStream_t stream) {
    if (p.scheme == EVOGP_SIM_NARX) return launch_sens_builds<VL, 2>(p, plan, stream);
    return p.S > 1 ? launch_sens_builds<VL, 1>(p, plan, stream) : launch_sens_builds<VL, 0>(p, plan, stream);
}

static int sens_check(unsigned pop, unsigned gp_len, unsigned B, unsigned T, unsigned S, unsigned U, int scheme) {
    if (pop == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || B == 0 || T == 0 || T > 65535u || S == 0 || S > (unsigned)kSensS || U > 32u ||
        S + U > 32u || scheme < EVOGP_SIM_MAP || scheme > EVOGP_SIM_NARX || pop > 0x7FFFFFFFu || B > 0x7FFFFFFFu ||
        (unsigned long long)B * T > 0x7FFFFFFFull)
        return EVOGP_E_BADARG;
    return EVOGP_OK;
}

static void sens_workspace(Arena &a, unsigned pop, unsigned gp_len, unsigned B, unsigned T, unsigned S, unsigned U, unsigned SC, int scheme,
                           float **ut, float **tt, int **cls, float **deep) {
    *ut = a.take<float>((size_t)B * T * U);
    *tt = a.take<float>((size_t)B * T * SC);
    *cls = a.take<int>(pop);
    *deep = a.take<float>((size_t)sens_plan(pop, B, S, scheme).deep_blocks * 2 * (gp_len + 2) * kWave);
}

static int sens_run(unsigned pop, unsigned gp_len, unsigned B, unsigned T, unsigned S, unsigned U, int scheme, float dt, float h2, float h6,
                    const float *value, const int16_t *type, const int16_t *size, const float *x0, const float *u, const float *target,
                    const float *weight, float *states, float *sens, double *loss64, float *loss32, float *normal, void *workspace,
                    hipStream_t stream) {
    const unsigned SC = loss64 ? (scheme == EVOGP_SIM_NARX ? 1u : S) : 0u;
    SensParams p{};
    float *ut, *tt;
    Arena a{(char *)workspace};
    sens_workspace(a, pop, gp_len, B, T, S, U, SC, scheme, &ut, &tt, &p.cls, &p.deep);
    hipError_t e;
    p.flags = acquire_counter(stream, &e);
    if (!p.flags) return (int)e;
    p.value = value; p.type = type; p.size = size; p.x0 = x0; p.ut = ut; p.tt = loss64 ? tt : nullptr; p.wgt = weight;
    p.states = states; p.sens = sens; p.loss64 = loss64; p.loss32 = loss32; p.normal = normal;
    p.pop = (int)pop; p.gp_len = (int)gp_len; p.B = (int)B; p.T = (int)T; p.S = (int)S; p.U = (int)U; p.SC = (int)SC;
    p.ntiles = (int)((B + kWave - 1) / kWave); p.scheme = scheme; p.dt = dt; p.h2 = h2; p.h6 = h6;
    const DeviceInfo &dev = device_info();
    const size_t moved = (size_t)B * T * (U + SC);
    if (moved) {
        size_t tb = (moved + 255) / 256;
        if (tb > (size_t)dev.num_cus * 16) tb = (size_t)dev.num_cus * 16;
        hipLaunchKernelGGL(sens_transpose_kernel, dim3((unsigned)tb), dim3(256), 0, stream, u, ut, (int)U, loss64 ? target : nullptr, tt, (int)SC, (int)B, (int)T);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    const SensPlan plan = sens_plan(pop, B, S, scheme);
    const unsigned vl = S + U;
    e = vl <= 9 ? launch_sens_kind<9>(p, plan, stream) : vl <= 16 ? launch_sens_kind<16>(p, plan, stream) : launch_sens_kind<32>(p, plan, stream);
    return (int)e;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_simulation_sens_workspace_bytes(unsigned pop_size, unsigned gp_len, unsigned trajectories, unsigned steps,
                                                            unsigned state_len, unsigned input_len, int scheme, int with_target,
                                                            unsigned long long *bytes) {
    if (!bytes) return EVOGP_E_NULLPTR;
    const int rc = sens_check(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme);
    if (rc != EVOGP_OK) return rc;
    Arena a{nullptr};
    float *ut, *tt, *deep;
    int *cls;
    sens_workspace(a, pop_size, gp_len, trajectories, steps, state_len, input_len, with_target ? (scheme == EVOGP_SIM_NARX ? 1u : state_len) : 0u,
                   scheme, &ut, &tt, &cls, &deep);
    *bytes = a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_simulation_sensitivities(unsigned pop_size, unsigned gp_len, unsigned trajectories, unsigned steps, unsigned state_len,
                                                     unsigned input_len, int scheme, float dt, float h2, float h6, const float *value,
                                                     const int16_t *type, const int16_t *size, const float *x0, const float *u, float *states_out,
                                                     float *sens_out, void *workspace, evogp_stream_t stream) {
    const int rc = sens_check(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme);
    if (rc != EVOGP_OK) return rc;
    if ((unsigned long long)pop_size * trajectories * steps * state_len * kSensK * sizeof(float) > (1ull << 31)) return EVOGP_E_BADARG;
    if (!value || !type || !size || !x0 || (!u && input_len) || !states_out || !sens_out || !workspace) return EVOGP_E_NULLPTR;
    return sens_run(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme, dt, h2, h6, value, type, size, x0, u, nullptr, nullptr,
                    states_out, sens_out, nullptr, nullptr, nullptr, workspace, (hipStream_t)stream);
}

extern "C" int evogp_hip_sr_simulation_normal_eq(unsigned pop_size, unsigned gp_len, unsigned trajectories, unsigned steps, unsigned state_len,
                                                 unsigned input_len, int scheme, float dt, float h2, float h6, const float *value,
                                                 const int16_t *type, const int16_t *size, const float *x0, const float *u, const float *target,
                                                 const float *state_weight, double *loss64_out, float *loss_out, float *normal_out,
                                                 void *workspace, evogp_stream_t stream) {
    const int rc = sens_check(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme);
    if (rc != EVOGP_OK) return rc;
    if (!value || !type || !size || !x0 || (!u && input_len) || !target || !state_weight || !loss64_out || !loss_out || !normal_out || !workspace)
        return EVOGP_E_NULLPTR;
    return sens_run(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme, dt, h2, h6, value, type, size, x0, u, target, state_weight,
                    nullptr, nullptr, loss64_out, loss_out, normal_out, workspace, (hipStream_t)stream);
}
