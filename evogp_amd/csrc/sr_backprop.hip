// sr_backprop.hip — semantic backpropagation (Pawlak, Wieloch & Krawiec 2015) over single-output trees on the rows of the dataset: the
// DESIRED VALUE of the subtree at node pos[t] of tree t on every row, and the match of those values against the semantics of a library
// of subtrees without writing a (pop, D) array (gfx950).  DESIGN.md section 3.24; tests/backprop_ref.py restates the rule.
//
//   (target, state) at the root = (y[d], REQUIRED); one step per function node on the path root -> pos inverts that node in the operand
//   the path takes, with the other operands' values read from the tape.  FREE (any value reproduces the label) and IMPOSSIBLE (none does)
//   are absorbing.  Every rule is ONE float32 operation (the unit is built with -ffp-contract=off):
//       ADD  d = t - s          SUB  k=0: d = t + s   k=1: d = s - t
//       MUL  s != 0: d = t / s; s == 0: t == 0 ? FREE : IMPOSSIBLE
//       DIV  k=0: s == 0 ? IMPOSSIBLE : d = t * s;   k=1: t != 0 && s != 0: d = s / t; t == 0 && s == 0: FREE; else IMPOSSIBLE
//       MAX  t >= s: d = t, else IMPOSSIBLE           MIN  t <= s: d = t, else IMPOSSIBLE
//       NEG  d = -t    INV  t != 0: d = 1 / t    SQRT  t >= 0: d = t * t    ABS  t >= 0: d = c < 0 ? -t : t, c the child's value
//       EXP  t > 0: d = logf(t)    LOG  d = expf(t)
//       IF   k=0: blocked; k=1: condition > 0 ? d = t : OTHER; k=2: condition > 0 ? OTHER : d = t     (a NaN condition is not > 0)
//            OTHER: the tree returns the branch it took, whose value is b: t == b ? FREE : IMPOSSIBLE
//   A NaN t, a NaN sibling s of a binary function, or a d that is not finite: IMPOSSIBLE.  Any other function on the path: the tree is
//   BLOCKED (status 3) and nothing is inverted.
//
// The decomposition is that of the tape kernels (sr_forward.hpp): one workgroup per tree, wave 0 classifies it and builds the operand
// table, the W waves of plan_tape_launch split the 64-row tiles, the value tape in LDS (rows of at most kTapeLdsLen nodes) or in the
// per-stream global workspace.  Wave 0 also finds the PATH: it turns the operand table round into a parent table (in the words of the
// stack the table was built with) and climbs from pos to the root, leaving per step one word (rule, tape indices of the operands the rule
// reads) in LDS; the ancestors are those the subtree sizes of a well-formed row give, taken from the table so that no size word behind
// the root's is trusted.  Per tile a wave walks the tree forward onto the tape and then the path downward with (t, state) in registers.
//
// FUSED == false materialises desired f32[pop][D] (NaN where the state is not REQUIRED), state u8[pop][D] and status.
// FUSED == true  reads the library semantics TRANSPOSED, lib_t f32[D][K], and writes dist f64[pop][K], best, const, const_dist, counts and
//   status only.  Lane j owns the entries j, j + 64, ... (at most 16 float64 sums in registers); the REQUIRED rows of a tile are taken
//   in row order, the row's desired value broadcast by v_readlane (no LDS round trip), the 64 lanes read 64 consecutive words of lib_t.
//   The waves' sums meet in one LDS row in wave order; the constant's moments are float64 sums SHIFTED by the wave's first REQUIRED value
//   (the pilot, as sr_genes.hip), merged in wave order by the pairwise update of Chan, Golub & LeVeque.
// No float atomics, nothing synchronises with the host: the same inputs give the same bits.
//
// MID == true (approximately geometric semantic crossover; tests/agx_ref.py restates it) takes the root target
// from a MATE instead of the labels: tree t is paired with row mate[t] of a second forest of the same row width, and on row d the target
// is mid = 0.5f * T_t(x_d) + 0.5f * T_mate(x_d), REQUIRED where mid is finite and IMPOSSIBLE from the start where it is not.  Wave 0
// classifies the mate as well and builds its operand table first (its build stack is the words that then hold the parent table); per
// tile a wave walks the mate forward onto the value tape, keeps its root value in a register and walks the recipient over the same
// tape.  Status 4: mate[t] is outside [0, n_mates) or the mate's row is malformed.  y is not read.
#include "sr_forward.hpp"
#include "sr_moments.hpp"

#include <type_traits>

namespace evogp {

constexpr int kBackpropMaxLib = EVOGP_BACKPROP_MAX_LIB;
constexpr int kBackpropAcc = kBackpropMaxLib / kWave;   // float64 sums per lane
static_assert(kBackpropAcc * kWave == kBackpropMaxLib && kBackpropAcc == 16, "lane j owns the entries j, j + 64, ...: 16 of them at most");

enum : int { BP_REQUIRED = 0, BP_FREE = 1, BP_IMPOSSIBLE = 2 };
enum : int { BP_OK = 0, BP_MALFORMED = 1, BP_POSITION = 2, BP_BLOCKED = 3, BP_MATE = 4 };
// the rules, the operand the path takes folded in; up to R_MIN the word's index is the SIBLING's (a NaN there: IMPOSSIBLE)
enum : uint32_t { R_ADD = 0, R_SUB0, R_SUB1, R_MUL, R_DIV0, R_DIV1, R_MAX, R_MIN, R_NEG, R_INV, R_SQRT, R_ABS, R_EXP, R_LOG, R_IF1, R_IF2, R_NONE };

struct BackpropParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;       // [D][var_len]
    const float *y;       // [D]
    const int *pos;       // [pop]
    const float *lib_t;   // [D][K]         (fused)
    float *desired;       // [pop][D]       (materialising)
    uint8_t *state;       // [pop][D]       (materialising)
    double *dist;         // [pop][K]       (fused)
    int *best;            // [pop]          (fused)
    float *cnst;          // [pop]          (fused)
    double *const_dist;   // [pop]          (fused)
    int *counts;          // [pop][3]       (fused)
    int *status;          // [pop]
    float *tape;          // global tapes (rows longer than kTapeLdsLen): [blocks * W][2][gp_len][64]; nullptr: the tapes are in LDS
    int pop, D, gp_len, var_len, K, KB;   // KB: the bucket of K the LDS row of sums is sized for (0: materialising)
};
// the MID builds' arguments: the labelled builds keep their own struct, and with it their kernel-argument layout
struct BackpropMidParams : BackpropParams {
    const float *mvalue;  // the mates: a forest of n_mates rows of gp_len words
    const int16_t *mtype;
    const int16_t *msize;
    const int *mate;      // [pop]          the mate's row of every tree
    int n_mates;
};

// Dynamic LDS of one workgroup in front of the tapes: sums[KB] mom[W][2] (double), op[L] kid[L] pay[L] parent[L] path[L] (u32),
// cnt[W][4] (REQUIRED, FREE, IMPOSSIBLE, the pilot's bits), meta[4] (class, length, status, steps)
template <int KB>
__host__ __device__ inline size_t backprop_lds_head_words(int L, int W) {
    return (((size_t)2 * KB + (size_t)4 * W + (size_t)5 * L + (size_t)4 * W + 4) + 3) & ~(size_t)3;
}
__device__ inline size_t backprop_head_words(int KB, int L, int W) {
    return (((size_t)2 * KB + (size_t)4 * W + (size_t)5 * L + (size_t)4 * W + 4) + 3) & ~(size_t)3;
}
// The MID builds: behind meta the mate's operand table mop[L] mkid[L] mpay[L] and its length mmeta[4]
template <int KB>
__host__ __device__ inline size_t backprop_mid_lds_head_words(int L, int W) {
    return (((size_t)2 * KB + (size_t)4 * W + (size_t)8 * L + (size_t)4 * W + 8) + 3) & ~(size_t)3;
}
__device__ inline size_t backprop_mid_head_words(int KB, int L, int W) {
    return (((size_t)2 * KB + (size_t)4 * W + (size_t)8 * L + (size_t)4 * W + 8) + 3) & ~(size_t)3;
}

// one forward walk of a tree of `len` nodes in execution order: every node's value of this lane's row on the tape
__device__ inline void backprop_forward(const uint32_t *s_op, const uint32_t *s_kid, const uint32_t *s_pay, int len, const float *xr,
                                        float *val, int lane) {
    for (int i = len - 1; i >= 0; --i) {
        const uint32_t op = (uint32_t)uni((int)s_op[i]) & kOpMask;
        float v;
        if (op < H_ADD) {
            const uint32_t pay = (uint32_t)uni((int)s_pay[i]);
            v = op == H_CONST ? bits2f(pay) : xr[pay];
        } else {
            const uint32_t kid = (uint32_t)uni((int)s_kid[i]);
            const float a = val[(kid & 1023u) * kWave + lane];
            if (op < H_UN) {
                v = binary_value(op, a, val[((kid >> 10) & 1023u) * kWave + lane]);
            } else if (op < H_IF) {
                v = op_unary<false>(op, a);
            } else {
                const float b = val[((kid >> 10) & 1023u) * kWave + lane], c = val[(kid >> 20) * kWave + lane];
                v = a > 0.0f ? b : c;
            }
        }
        val[i * kWave + lane] = v;
    }
}

// the rule of function node `op` in operand k, and which of its operands the rule reads: one index in bits 0..9, an IF's other branch
// in bits 10..19
__device__ inline uint32_t backprop_rule(uint32_t op, uint32_t kid, int k, uint32_t *index) {
    const uint32_t k0 = kid & 1023u, k1 = (kid >> 10) & 1023u, k2 = kid >> 20;
    *index = k == 0 ? k1 : k0;   // a binary function's sibling
    switch (op) {
    case H_ADD: return R_ADD;
    case H_SUB: return k == 0 ? R_SUB0 : R_SUB1;
    case H_MUL: return R_MUL;
    case H_DIV: return k == 0 ? R_DIV0 : R_DIV1;
    case H_BIN_OTHER + (F_MAX - F_LOOSE_DIV): return R_MAX;
    case H_BIN_OTHER + (F_MIN - F_LOOSE_DIV): return R_MIN;
    default: break;
    }
    *index = k0;   // a unary function's child (ABS reads it), an IF's condition
    switch (op) {
    case H_UN + (F_NEG - F_SIN): return R_NEG;
    case H_UN + (F_INV - F_SIN): return R_INV;
    case H_UN + (F_SQRT - F_SIN): return R_SQRT;
    case H_UN + (F_ABS - F_SIN): return R_ABS;
    case H_UN + (F_EXP - F_SIN): return R_EXP;
    case H_UN + (F_LOG - F_SIN): return R_LOG;
    case H_IF: *index = k0 | ((k == 1 ? k2 : k1) << 10); return k == 1 ? R_IF1 : k == 2 ? R_IF2 : R_NONE;
    default: return R_NONE;
    }
}

// one step down the path: (t, state) of the parent -> of the child; s is the value the rule's word names, b an IF's other branch
__device__ inline void backprop_step(uint32_t rule, float s, float b, float &t, int &state) {
    float d = t;
    int ns = BP_REQUIRED;
    switch (rule) {   // (wave-uniform)
    case R_ADD: d = t - s; break;
    case R_SUB0: d = t + s; break;
    case R_SUB1: d = s - t; break;
    case R_MUL: if (s != 0.0f) d = t / s; else ns = t == 0.0f ? BP_FREE : BP_IMPOSSIBLE; break;
    case R_DIV0: if (s == 0.0f) ns = BP_IMPOSSIBLE; else d = t * s; break;
    case R_DIV1: if (t != 0.0f && s != 0.0f) d = s / t; else ns = (t == 0.0f && s == 0.0f) ? BP_FREE : BP_IMPOSSIBLE; break;
    case R_MAX: if (!(t >= s)) ns = BP_IMPOSSIBLE; break;
    case R_MIN: if (!(t <= s)) ns = BP_IMPOSSIBLE; break;
    case R_NEG: d = -t; break;
    case R_INV: if (t != 0.0f) d = 1.0f / t; else ns = BP_IMPOSSIBLE; break;
    case R_SQRT: if (t >= 0.0f) d = t * t; else ns = BP_IMPOSSIBLE; break;
    case R_ABS: if (t >= 0.0f) d = s < 0.0f ? -t : t; else ns = BP_IMPOSSIBLE; break;
    case R_EXP: if (t > 0.0f) d = logf(t); else ns = BP_IMPOSSIBLE; break;
    case R_LOG: d = expf(t); break;
    case R_IF1: if (!(s > 0.0f)) ns = t == b ? BP_FREE : BP_IMPOSSIBLE; break;
    default: if (s > 0.0f) ns = t == b ? BP_FREE : BP_IMPOSSIBLE; break;   // R_IF2
    }
    if (t != t || (rule <= R_MIN && s != s)) ns = BP_IMPOSSIBLE;
    if (ns == BP_REQUIRED && !finite_f(d)) ns = BP_IMPOSSIBLE;
    if (state == BP_REQUIRED) { state = ns; t = d; }
}

template <bool FUSED, bool MID = false>
__global__ __launch_bounds__(kTapeMaxWaves * 64) void sr_backprop_kernel(std::conditional_t<MID, BackpropMidParams, BackpropParams> p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bp_lds[];
    const int L = p.gp_len;
    const int K = p.K;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    double *s_sum = (double *)bp_lds;
    double *s_mom = s_sum + p.KB;
    uint32_t *s_op = (uint32_t *)(s_mom + 2 * W), *s_kid = s_op + L, *s_pay = s_kid + L;
    int *s_par = (int *)(s_pay + L);
    uint32_t *s_path = (uint32_t *)(s_par + L);
    int *s_cnt = (int *)(s_path + L);
    int *s_meta = s_cnt + 4 * W;
    uint32_t *s_mop = (uint32_t *)(s_meta + 4), *s_mkid = s_mop + L, *s_mpay = s_mkid + L;   // (MID) the mate's table and length
    int *s_mmeta = (int *)(s_mpay + L);
    float *val = p.tape ? p.tape + ((size_t)blockIdx.x * W + w) * 2 * L * kWave
                        : (float *)(bp_lds + (MID ? backprop_mid_head_words(p.KB, L, W) : backprop_head_words(p.KB, L, W))) +
                              (size_t)w * 2 * L * kWave;
    const int ntiles = (p.D + kWave - 1) / kWave;
    const float nanf_ = __builtin_nanf("");

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        const size_t row = (size_t)t * L;
        // ---- wave 0: classify, decode, operand table, the path ----
        if (w == 0) {
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > L ? L : len);
            const int cls = uni(classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, kMaxStack));
            const int at = uni(p.pos[t]);
            int status = cls != TREE_OK ? BP_MALFORMED : (at < 0 || at >= len) ? BP_POSITION : BP_OK;
            int steps = 0;
            if constexpr (MID) if (status == BP_OK) {
                // the mate: its row in range, well-formed; its table first, built with the words that then hold the parent table
                const int m = uni(p.mate[t]);
                status = BP_MATE;
                if (m >= 0 && m < p.n_mates) {
                    const size_t mrow = (size_t)m * L;
                    int mlen = uni((int)p.msize[mrow]);
                    mlen = mlen < 0 ? 0 : (mlen > L ? L : mlen);
                    if (uni(classify_tree(p.mtype + mrow, p.mvalue + mrow, mlen, false, p.var_len, 1, kMaxStack)) == TREE_OK) {
                        build_operand_table<false>(p.mtype, p.mvalue, mrow, mlen, p.var_len, 1, s_mop, s_mkid, s_mpay, s_par);
                        if (lane == 0) s_mmeta[0] = mlen;
                        status = BP_OK;
                    }
                }
            }
            if (status == BP_OK) {
                build_operand_table<false>(p.type, p.value, row, len, p.var_len, 1, s_op, s_kid, s_pay, s_par);
                // the parent of every node: index | operand << 10 (the root's word stays 0)
                for (int i = lane; i < len; i += kWave) s_par[i] = 0;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int i = lane; i < len; i += kWave) {
                    const uint32_t op = s_op[i] & kOpMask;
                    const int arity = op < H_ADD ? 0 : op < H_UN ? 2 : op < H_IF ? 1 : 3;
                    const uint32_t kid = s_kid[i];
                    for (int k = 0; k < arity; ++k) s_par[(kid >> (10 * k)) & 1023u] = i | (k << 10);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                // climb: step j of the list is the j-th ancestor from pos upward (a parent lies in front of its child: at most len steps)
                int node = at;
                while (node > 0 && steps < len) {
                    const int par = uni(s_par[node]);
                    const int i = par & 1023, k = par >> 10;
                    uint32_t index;
                    const uint32_t rule = backprop_rule((uint32_t)uni((int)s_op[i]) & kOpMask, (uint32_t)uni((int)s_kid[i]), k, &index);
                    if (rule == R_NONE) { status = BP_BLOCKED; break; }
                    if (lane == 0) s_path[steps] = index | (rule << 20);
                    ++steps;
                    node = i;
                }
            }
            if (lane == 0) { s_meta[0] = cls; s_meta[1] = len; s_meta[2] = status; s_meta[3] = steps; }
        }
        __syncthreads();
        const int len = uni(s_meta[1]);
        const int status = uni(s_meta[2]);
        const int steps = uni(s_meta[3]);
        if (threadIdx.x == 0) p.status[t] = status;
        if (status != BP_OK) {  // nothing is inverted: every row IMPOSSIBLE
            if (FUSED) {
                for (int k = threadIdx.x; k < K; k += blockDim.x) p.dist[(size_t)t * K + k] = 0.0;
                if (threadIdx.x == 0) {
                    p.best[t] = -1;
                    p.cnst[t] = nanf_;
                    p.const_dist[t] = __builtin_nan("");
                    p.counts[(size_t)t * 3 + 0] = 0; p.counts[(size_t)t * 3 + 1] = 0; p.counts[(size_t)t * 3 + 2] = p.D;
                }
            } else {
                for (int d = threadIdx.x; d < p.D; d += blockDim.x) {
                    p.desired[(size_t)t * p.D + d] = nanf_;
                    p.state[(size_t)t * p.D + d] = (uint8_t)BP_IMPOSSIBLE;
                }
            }
            __syncthreads();
            continue;
        }

        double acc[kBackpropAcc];   // (fused) lane j: the sums of the entries j, j + 64, ...; every index is a constant after unrolling
#pragma unroll
        for (int c = 0; c < kBackpropAcc; ++c) acc[c] = 0.0;
        int n_req = 0, n_free = 0, n_imp = 0;   // (fused, wave-uniform)
        bool have_pilot = false;                // (fused, wave-uniform)
        float pilot = 0.0f;
        double m1 = 0.0, m2 = 0.0;              // (fused) the lane's shifted sums

        for (int tile = w; tile < ntiles; tile += W) {
            const int d = tile * kWave + lane;
            const bool valid = d < p.D;
            const int dc = valid ? d : p.D - 1;
            const float *xr = p.X + (size_t)dc * p.var_len;
            // ---- forward: execution order, every node's value on the tape (MID: the mate first, its root value kept) ----
            float mroot = 0.0f;
            if constexpr (MID) {
                backprop_forward(s_mop, s_mkid, s_mpay, uni(s_mmeta[0]), xr, val, lane);
                mroot = val[lane];
            }
            backprop_forward(s_op, s_kid, s_pay, len, xr, val, lane);
            // ---- downward: from the root's step to the step above pos ----
            float tgt;
            int st = BP_REQUIRED;
            if (MID) {   // the midpoint of the two roots: two scalings and one addition; not finite: IMPOSSIBLE from the start
                tgt = 0.5f * val[lane] + 0.5f * mroot;
                if (!finite_f(tgt)) st = BP_IMPOSSIBLE;
            } else {
                tgt = p.y[dc];
            }
            for (int j = steps - 1; j >= 0; --j) {
                const uint32_t word = (uint32_t)uni((int)s_path[j]);
                backprop_step(word >> 20, val[(word & 1023u) * kWave + lane], val[((word >> 10) & 1023u) * kWave + lane], tgt, st);
            }
            if (!FUSED) {
                if (valid) {
                    p.desired[(size_t)t * p.D + d] = st == BP_REQUIRED ? tgt : nanf_;
                    p.state[(size_t)t * p.D + d] = (uint8_t)st;
                }
                continue;
            }
            // ---- match: the REQUIRED rows of the tile in row order against the library ----
            const bool req = valid && st == BP_REQUIRED;
            unsigned long long mask = __ballot(req);
            n_req += __popcll(mask);
            n_free += __popcll(__ballot(valid && st == BP_FREE));
            n_imp += __popcll(__ballot(valid && st == BP_IMPOSSIBLE));
            if (!have_pilot && mask != 0ull) {
                pilot = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(tgt), (int)__builtin_ctzll(mask)));
                have_pilot = true;
            }
            if (req) {
                const double x = (double)tgt - (double)pilot;
                m1 += x;
                m2 += x * x;
            }
            const float *lib_tile = p.lib_t + (size_t)tile * kWave * K;
            while (mask != 0ull) {
                const int r = (int)__builtin_ctzll(mask);
                mask &= mask - 1ull;
                const double dv = (double)bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(tgt), r));
                const float *lr = lib_tile + (size_t)r * K;
#pragma unroll
                for (int c = 0; c < kBackpropAcc; ++c) {
                    if (c * kWave < K) {   // (wave-uniform)
                        const int k = c * kWave + lane;
                        if (k < K) {
                            const double e = dv - (double)lr[k];
                            acc[c] += e * e;
                        }
                    }
                }
            }
        }

        if (FUSED) {
            // ---- reduce: the waves' sums in wave order through one LDS row; counts and moments parked per wave ----
            const double w1 = wave_sum_d(m1), w2 = wave_sum_d(m2);
            if (lane == 0) {
                s_mom[2 * w] = w1; s_mom[2 * w + 1] = w2;
                s_cnt[4 * w] = n_req; s_cnt[4 * w + 1] = n_free; s_cnt[4 * w + 2] = n_imp; s_cnt[4 * w + 3] = (int)f2bits(pilot);
            }
            for (int q = 0; q < W; ++q) {
                if (w == q) {
#pragma unroll
                    for (int c = 0; c < kBackpropAcc; ++c) {
                        const int k = c * kWave + lane;
                        if (k < K) s_sum[k] = q == 0 ? acc[c] : s_sum[k] + acc[c];
                    }
                }
                __syncthreads();
            }
            // a sum that is not finite met a library value that is not (finite rows cannot overflow float64): +inf
            for (int k = threadIdx.x; k < K; k += blockDim.x) {
                double v = s_sum[k];
                if (!__builtin_isfinite(v)) v = __builtin_inf();
                s_sum[k] = v;
                p.dist[(size_t)t * K + k] = v;
            }
            __syncthreads();
            if (w == 0) {
                // the least distance, the smallest entry on ties; +inf is never taken
                double bv = __builtin_inf();
                int bk = 0x7FFFFFFF;
                for (int k = lane; k < K; k += kWave) {
                    const double v = s_sum[k];
                    if (v < bv) { bv = v; bk = k; }
                }
                for (int off = 1; off < kWave; off <<= 1) {
                    const double ov = __hiloint2double(__shfl_xor(__double2hiint(bv), off), __shfl_xor(__double2loint(bv), off));
                    const int ok = __shfl_xor(bk, off);
                    if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
                }
                if (lane == 0) {
                    int cr = 0, cf = 0, ci = 0;
                    double n = 0.0, p0 = 0.0, ms = 0.0, M2 = 0.0;
                    for (int q = 0; q < W; ++q) {
                        cr += s_cnt[4 * q]; cf += s_cnt[4 * q + 1]; ci += s_cnt[4 * q + 2];
                        const double nb = (double)s_cnt[4 * q];
                        if (nb == 0.0) continue;
                        const double a = (double)bits2f((uint32_t)s_cnt[4 * q + 3]), s1 = s_mom[2 * q], s2 = s_mom[2 * q + 1];
                        if (n == 0.0) p0 = a;
                        const double nn = n + nb;
                        const double dm = ((a - p0) + s1 / nb) - ms;   // the unit's mean against the merged one, both as offsets from p0
                        M2 = (M2 + (s2 - s1 * s1 / nb)) + dm * dm * (n * nb / nn);
                        ms += dm * (nb / nn);
                        n = nn;
                    }
                    p.counts[(size_t)t * 3 + 0] = cr; p.counts[(size_t)t * 3 + 1] = cf; p.counts[(size_t)t * 3 + 2] = ci;
                    p.best[t] = cr == 0 || bk == 0x7FFFFFFF ? -1 : bk;
                    p.cnst[t] = cr == 0 ? nanf_ : (float)(p0 + ms);
                    p.const_dist[t] = cr == 0 ? __builtin_nan("") : (M2 < 0.0 ? 0.0 : M2);
                }
            }
        }
        __syncthreads();  // the tables are rebuilt for the next tree
    }
}

}  // namespace evogp

using namespace evogp;

// the checks both entry points share, in the order of evogp_hip_sr_input_gradient: bad argument, null pointer, out_len
static int backprop_check(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    return 0;
}

template <bool FUSED, int KB, bool MID = false>
static int backprop_launch(std::conditional_t<MID, BackpropMidParams, BackpropParams> &p, hipStream_t stream) {
    p.KB = KB;
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, MID ? backprop_mid_lds_head_words<KB> : backprop_lds_head_words<KB>, &plan))
        return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if (const hipError_t e = grant_tape_lds(grant, {(const void *)sr_backprop_kernel<FUSED, MID>})) return (int)e;
    hipLaunchKernelGGL((sr_backprop_kernel<FUSED, MID>), dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_desired(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                    const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                    const float *labels, const int *pos, float *desired, unsigned char *state, int *status,
                                    evogp_stream_t stream_) {
    if (const int rc = backprop_check(pop_size, data_points, gp_len, var_len, out_len)) return rc;
    if (!value || !type || !size || !variables || !labels || !pos || !desired || !state || !status) return EVOGP_E_NULLPTR;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    BackpropParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.pos = pos;
    p.desired = desired; p.state = state; p.status = status;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    return backprop_launch<false, 0>(p, (hipStream_t)stream_);
}

extern "C" int evogp_hip_sr_backprop_match(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                           const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                           const float *labels, const int *pos, unsigned n_lib, const float *lib_t, double *dist, int *best,
                                           float *cnst, double *const_dist, int *counts, int *status, evogp_stream_t stream_) {
    if (const int rc = backprop_check(pop_size, data_points, gp_len, var_len, out_len)) return rc;
    if (n_lib == 0 || n_lib > (unsigned)kBackpropMaxLib) return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !labels || !pos || !lib_t || !dist || !best || !cnst || !const_dist || !counts || !status)
        return EVOGP_E_NULLPTR;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    BackpropParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.pos = pos; p.lib_t = lib_t;
    p.dist = dist; p.best = best; p.cnst = cnst; p.const_dist = const_dist; p.counts = counts; p.status = status;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.K = (int)n_lib;
    const hipStream_t stream = (hipStream_t)stream_;
    // the LDS row of sums is sized by a bucket of K, so that a small library leaves the tapes their room
    if (n_lib <= 64) return backprop_launch<true, 64>(p, stream);
    if (n_lib <= 256) return backprop_launch<true, 256>(p, stream);
    return backprop_launch<true, kBackpropMaxLib>(p, stream);
}

// ---- the midpoint builds: the root target from a mate (n_mates rows of the same width, mate i32[pop]) instead of the labels ----
extern "C" int evogp_hip_sr_desired_mid(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                        const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                        unsigned n_mates, const float *mvalue, const int16_t *mtype, const int16_t *msize, const int *mate,
                                        const int *pos, float *desired, unsigned char *state, int *status, evogp_stream_t stream_) {
    if (const int rc = backprop_check(pop_size, data_points, gp_len, var_len, out_len)) return rc;
    if (n_mates == 0 || n_mates > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !mvalue || !mtype || !msize || !mate || !pos || !desired || !state || !status)
        return EVOGP_E_NULLPTR;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    BackpropMidParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.pos = pos;
    p.mvalue = mvalue; p.mtype = mtype; p.msize = msize; p.mate = mate; p.n_mates = (int)n_mates;
    p.desired = desired; p.state = state; p.status = status;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    return backprop_launch<false, 0, true>(p, (hipStream_t)stream_);
}

extern "C" int evogp_hip_sr_agx_match(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                      const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                      unsigned n_mates, const float *mvalue, const int16_t *mtype, const int16_t *msize, const int *mate,
                                      const int *pos, unsigned n_lib, const float *lib_t, double *dist, int *best, float *cnst,
                                      double *const_dist, int *counts, int *status, evogp_stream_t stream_) {
    if (const int rc = backprop_check(pop_size, data_points, gp_len, var_len, out_len)) return rc;
    if (n_mates == 0 || n_mates > 0x7FFFFFFFu || n_lib == 0 || n_lib > (unsigned)kBackpropMaxLib) return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !mvalue || !mtype || !msize || !mate || !pos || !lib_t || !dist || !best || !cnst ||
        !const_dist || !counts || !status)
        return EVOGP_E_NULLPTR;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    BackpropMidParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.pos = pos; p.lib_t = lib_t;
    p.mvalue = mvalue; p.mtype = mtype; p.msize = msize; p.mate = mate; p.n_mates = (int)n_mates;
    p.dist = dist; p.best = best; p.cnst = cnst; p.const_dist = const_dist; p.counts = counts; p.status = status;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.K = (int)n_lib;
    const hipStream_t stream = (hipStream_t)stream_;
    if (n_lib <= 64) return backprop_launch<true, 64, true>(p, stream);
    if (n_lib <= 256) return backprop_launch<true, 256, true>(p, stream);
    return backprop_launch<true, kBackpropMaxLib, true>(p, stream);
}
