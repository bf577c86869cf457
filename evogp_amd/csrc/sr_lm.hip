// sr_lm.hip — Levenberg-Marquardt optimisation of the constants of single-output trees under the MSE loss (gfx950): the per-tree
// Gauss-Newton normal equations (evogp_hip_sr_normal_eq) and one damped step on them (evogp_hip_sr_lm_step).
//
//   J_j[d]    = d tree_t(X[d]) / d c_j       c_j: the j-th CONST node of the live prefix in prefix order, j < K = kLmMaxConsts (the
//                                            OPTIMISED constants; a tree's further constants are held fixed)
//   r[d]      = tree_t(X[d]) - y[d]
//   loss[t]   = (1/D) sum_d r[d]^2           (what sr_grad.hip returns, summed in the same order)
//   normal[t] = A_ij = (1/D) sum_d J_i J_j  (i <= j < K, 36 words row-major), then b_i = (1/D) sum_d J_i r (8 words)
//
// The normal-equation kernel is sr_grad_kernel<false>'s walk (one workgroup per tree, wave 0 builds the operand table, W waves share the
// 64-row tiles, forward tape then reverse walk over a [node][lane] tape) with two differences: the reverse walk is seeded with 1
// instead of d loss / d pred, so the adjoint slot of a CONST node holds the lane's J_j; and those slots are STORED per tile (a CONST
// leaf has one parent, so one store per tile defines it) and folded into 45 register accumulators per lane after each tile's walk.
// Lanes are reduced by the fixed DPP butterfly (wave_sum), waves in wave order through LDS: no float atomics, bit-identical from run
// to run.  Tapes live in LDS for rows of at most kTapeLdsLen nodes and in the tape kernels' per-stream global workspace for longer rows;
// the launch is the plan the three tape passes share (sr_forward.hpp plan_tape_launch), which is why the loss is sr_grad.hip's bit for bit.
//
// The WEIGHTED build (WL, evogp_hip_sr_weighted_normal_eq) differs as sr_grad.hip's does: the row's weight is read next to y, `valid`
// also asks for w != 0 (a tile without a weighted row is skipped whole), A and b are sums of w J_i J_j and w J_i r over Wsum, the loss
// is sum w r^2 in float64 (sr_grad.hip's weighted loss for mse, bit for bit), and a non-finite prediction on a weighted row makes the
// tree NaN.
#include <type_traits>

#include "sr_adjoint.hpp"
#include "sr_moments.hpp"

namespace evogp {

constexpr int kLmTri = kLmMaxConsts * (kLmMaxConsts + 1) / 2;   // 36: upper triangle of A
constexpr int kLmWords = kLmTri + kLmMaxConsts;                 // 44: a row of `normal`
constexpr int kLmPart = 48;         // words of one wave's partial sums in LDS: 44 of `normal`, the sum of r^2, padding
constexpr int kLmPartBad = 45, kLmPartLoss = 46;   // weighted build: "met a non-finite prediction", and the float64 sum of w r^2 (2 words)
static_assert(kLmWords == EVOGP_LM_NORMAL_WORDS && kLmWords + 1 <= kLmPart, "layout of a normal-equation row");

struct NormalEqParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;  // [D][var_len]
    const float *y;  // [D]
    float *loss;     // [pop]
    float *normal;   // [pop][kLmWords]
    float *tape;     // global tapes (rows longer than kTapeLdsLen): [blocks * W][2][gp_len][64]; nullptr: the tapes are in LDS
    int pop, D, gp_len, var_len;
};

struct WNormalEqParams : NormalEqParams {   // the weighted build's
    const float *w;           // [D], or nullptr: every weight is 1
    const WeightStat *stat;   // the weight row's sum and whether it may be used (weight_stats_kernel); nullptr without w
};

// The optimised constants of a single-output row: the node indices of its first kLmMaxConsts CONST nodes inside [0, len), in prefix
// order, written to cidx[0 .. nc) by lane 0 (the rest of cidx is set to -1); returns nc.  Called by every lane of one wave; cidx is
// that wave's own LDS.
__device__ inline int find_optimised_consts(const int16_t *type_row, int len, int *cidx) {
    const int lane = threadIdx.x & 63;
    int nc = 0;
    for (int base = 0; base < len && nc < kLmMaxConsts; base += kWave) {
        const int i = base + lane;
        unsigned long long m = __ballot(i < len && type_row[i] == T_CONST);
        while (m != 0 && nc < kLmMaxConsts) {
            const int bit = __ffsll((long long)m) - 1;
            if (lane == 0) cidx[nc] = base + bit;
            m &= m - 1;
            ++nc;
        }
    }
    if (lane == 0)
        for (int j = nc; j < kLmMaxConsts; ++j) cidx[j] = -1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return nc;
}

// Dynamic LDS of one workgroup (16-byte aligned carve): op[L] kids[L] pay[L] stack[L] (u32), part[W][kLmPart], cidx[K], cls / len / nc
// (3 words, padded to 4), then, for LDS tapes, W x 2 x L x 64 floats.
__host__ __device__ inline size_t lm_lds_head_words(int L, int W) {
    return (((size_t)4 * L + (size_t)W * kLmPart + kLmMaxConsts + 4) + 3) & ~(size_t)3;
}

template <bool WL = false>
__global__ __launch_bounds__(kTapeMaxWaves * 64) void sr_normal_eq_kernel(std::conditional_t<WL, WNormalEqParams, NormalEqParams> p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lm_lds[];
    const int L = p.gp_len;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    uint32_t *s_op = lm_lds, *s_kid = s_op + L, *s_pay = s_kid + L;
    int *s_stk = (int *)(s_pay + L);
    float *s_part = (float *)(s_stk + L);
    int *s_cidx = (int *)(s_part + (size_t)W * kLmPart);
    int *s_meta = s_cidx + kLmMaxConsts;
    float *tape = p.tape ? p.tape + ((size_t)blockIdx.x * W + w) * 2 * L * kWave
                         : (float *)(lm_lds + lm_lds_head_words(L, W)) + (size_t)w * 2 * L * kWave;
    float *val = tape, *adj = tape + (size_t)L * kWave;
    const int ntiles = (p.D + kWave - 1) / kWave;
    double wsum = (double)p.D;
    bool usable = true;
    if constexpr (WL) {
        if (p.w) { wsum = p.stat->sum; usable = p.stat->usable != 0; }
    }

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        const size_t row = (size_t)t * L;
        if (WL && !usable) {  // a weight row that may not be used: NaN loss, zero row, for every tree
            for (int i = threadIdx.x; i < kLmWords; i += blockDim.x) p.normal[(size_t)t * kLmWords + i] = 0.0f;
            if (threadIdx.x == 0) p.loss[t] = __builtin_nanf("");
            continue;
        }
        // ---- wave 0: classify, decode, operand table, the optimised constants ----
        if (w == 0) {
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > L ? L : len);
            const int cls = uni(classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, kMaxStack));
            int nc = 0;
            if (cls == TREE_OK) {
                build_operand_table<false>(p.type, p.value, row, len, p.var_len, 1, s_op, s_kid, s_pay, s_stk);
                nc = find_optimised_consts(p.type + row, len, s_cidx);
            }
            if (lane == 0) { s_meta[0] = cls; s_meta[1] = len; s_meta[2] = nc; }
        }
        __syncthreads();
        const int cls = uni(s_meta[0]);
        const int len = uni(s_meta[1]);
        const int nc = uni(s_meta[2]);
        if (cls != TREE_OK) {  // malformed: NaN loss, zero row
            for (int i = threadIdx.x; i < kLmWords; i += blockDim.x) p.normal[(size_t)t * kLmWords + i] = 0.0f;
            if (threadIdx.x == 0) p.loss[t] = __builtin_nanf("");
            __syncthreads();
            continue;
        }
        int cidx[kLmMaxConsts];  // (wave-uniform: scalar registers)
#pragma unroll
        for (int j = 0; j < kLmMaxConsts; ++j) cidx[j] = uni(s_cidx[j]);

        float A[kLmTri], b[kLmMaxConsts], r2 = 0.0f;
#pragma unroll
        for (int k = 0; k < kLmTri; ++k) A[k] = 0.0f;
#pragma unroll
        for (int k = 0; k < kLmMaxConsts; ++k) b[k] = 0.0f;

        double dacc = 0.0;   // (weighted build)
        int bad = 0;
        for (int tile = w; tile < ntiles; tile += W) {
            const int d = tile * kWave + lane;
            bool valid = d < p.D;
            const int dc = valid ? d : p.D - 1;
            float wv = 1.0f;
            if constexpr (WL) {
                if (p.w) wv = p.w[dc];
                valid = valid && wv != 0.0f;   // a row without weight is not looked at
                if (!__any(valid)) continue;   // (wave-uniform) nor is a tile of them
            }
            const float *xr = p.X + (size_t)dc * p.var_len;
            // ---- forward: execution order, every node's value on the tape ----
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
                        const float bb = val[((kid >> 10) & 1023u) * kWave + lane], c = val[(kid >> 20) * kWave + lane];
                        v = a > 0.0f ? bb : c;
                    }
                }
                val[i * kWave + lane] = v;
            }
            const float r = val[lane] - p.y[dc];
            // ---- reverse: prefix order, parents before children, d pred / d node; every operand's slot is stored ----
            adj[lane] = 1.0f;
            for (int i = 0; i < len; ++i) {
                const uint32_t op = (uint32_t)uni((int)s_op[i]) & kOpMask;
                if (op < H_ADD) continue;
                const uint32_t kid = (uint32_t)uni((int)s_kid[i]);
                const float g = adj[i * kWave + lane];
                const float a = val[(kid & 1023u) * kWave + lane];
                if (op < H_UN) {
                    const float bb = val[((kid >> 10) & 1023u) * kWave + lane];
                    float da, db;
                    binary_adjoint(op, a, bb, val[i * kWave + lane], g, da, db);
                    adj[(kid & 1023u) * kWave + lane] = da;
                    adj[((kid >> 10) & 1023u) * kWave + lane] = db;
                } else if (op < H_IF) {
                    adj[(kid & 1023u) * kWave + lane] = unary_adjoint(op, a, val[i * kWave + lane], g);
                } else {
                    const bool take_b = a > 0.0f;
                    adj[(kid & 1023u) * kWave + lane] = 0.0f;
                    adj[((kid >> 10) & 1023u) * kWave + lane] = take_b ? g : 0.0f;
                    adj[(kid >> 20) * kWave + lane] = take_b ? 0.0f : g;
                }
            }
            // ---- this tile's row of the normal equations (rows past D add nothing; absent constants are never touched) ----
            float J[kLmMaxConsts];
#pragma unroll
            for (int j = 0; j < kLmMaxConsts; ++j) {
                J[j] = 0.0f;
                if (j < nc) {
                    const float x = adj[cidx[j] * kWave + lane];
                    J[j] = valid ? x : 0.0f;
                }
            }
            const float rv = valid ? r : 0.0f;
            if (WL) {
                const float pred = val[lane];
                const double rd = (double)pred - (double)p.y[dc];
                const double term = valid ? (double)wv * wloss_rho<false>(EVOGP_LOSS_MSE, 0.0, rd) : 0.0;
                dacc += term;
                bad |= valid && !finite_f(pred);
            } else {
                r2 += rv * rv;
            }
            int k = 0;
#pragma unroll
            for (int i = 0; i < kLmMaxConsts; ++i) {
                const float wJ = WL ? wv * J[i] : J[i];
#pragma unroll
                for (int j = i; j < kLmMaxConsts; ++j, ++k)
                    if (j < nc) A[k] += wJ * J[j];
                if (i < nc) b[i] += wJ * rv;
            }
        }

        // ---- reduce: lanes by the fixed butterfly, waves in wave order ----
        float *part = s_part + (size_t)w * kLmPart;
#pragma unroll
        for (int k = 0; k < kLmTri; ++k) {
            const float s = wave_sum(A[k]);
            if (lane == 0) part[k] = s;
        }
#pragma unroll
        for (int k = 0; k < kLmMaxConsts; ++k) {
            const float s = wave_sum(b[k]);
            if (lane == 0) part[kLmTri + k] = s;
        }
        if (WL) {
            const double s = wave_sum_d(dacc);
            const int wbad = __any(bad) ? 1 : 0;
            if (lane == 0) { *(double *)(part + kLmPartLoss) = s; ((int *)part)[kLmPartBad] = wbad; }
        } else {
            const float s = wave_sum(r2);
            if (lane == 0) part[kLmWords] = s;
        }
        __syncthreads();
        if (WL) {
            if (threadIdx.x <= kLmWords) {
                bool ok = true;   // no weighted row with a non-finite prediction
                for (int k = 0; k < W; ++k) ok = ok && ((const int *)s_part)[(size_t)k * kLmPart + kLmPartBad] == 0;
                if (threadIdx.x < kLmWords) {
                    float s = 0.0f;
                    for (int k = 0; k < W; ++k) s += s_part[(size_t)k * kLmPart + threadIdx.x];
                    p.normal[(size_t)t * kLmWords + threadIdx.x] = ok ? (float)((double)s / wsum) : 0.0f;
                } else {
                    double s = 0.0;
                    for (int k = 0; k < W; ++k) s += *(const double *)(s_part + (size_t)k * kLmPart + kLmPartLoss);
                    p.loss[t] = ok ? (float)(s / wsum) : __builtin_nanf("");
                }
            }
        } else if (threadIdx.x <= kLmWords) {
            float s = 0.0f;
            for (int k = 0; k < W; ++k) s += s_part[(size_t)k * kLmPart + threadIdx.x];
            s = s / (float)p.D;
            if (threadIdx.x < kLmWords) p.normal[(size_t)t * kLmWords + threadIdx.x] = s;
            else p.loss[t] = s;
        }
        __syncthreads();  // the tables are rebuilt for the next tree
    }
}

// ---- one iteration of the damped Gauss-Newton iteration (evogp_hip_sr_lm_step) ----------------------------------------------------
struct LmStepParams {
    float *value;              // [pop][gp_len] current constants (only the optimised constants are written)
    const int16_t *type;
    const int16_t *size;
    float *cand;               // [pop][gp_len] candidate forest (every word written when proposing)
    float *loss;               // [pop] loss of the current forest
    float *normal;             // [pop][kLmWords] its normal equations
    const float *loss_cand;    // [pop] loss of the candidate forest (accepting)
    const float *normal_cand;  // [pop][kLmWords] its normal equations
    float *damping;            // [pop] lambda_t
    int pop, gp_len, phase;
};

constexpr float kLmDampMin = 1e-10f, kLmDampMax = 1e10f;

// One wave per tree.  The solve is ~100 float64 operations on wave-uniform data: every lane does it (no divergence, no broadcast).
__global__ __launch_bounds__(256) void sr_lm_step_kernel(LmStepParams q) {
    __shared__ int s_cidx_all[4][kLmMaxConsts];
    constexpr int K = kLmMaxConsts;
    const int lane = threadIdx.x & 63;
    const int wv = uni((int)(threadIdx.x >> 6));
    const int t = uni((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (t >= q.pop) return;
    int *s_cidx = s_cidx_all[wv];
    const size_t row = (size_t)t * q.gp_len;
    int len = uni((int)q.size[row]);
    len = len < 0 ? 0 : (len > q.gp_len ? q.gp_len : len);
    const int nc = find_optimised_consts(q.type + row, len, s_cidx);
    int cidx[K];
#pragma unroll
    for (int j = 0; j < K; ++j) cidx[j] = uni(s_cidx[j]);
    float *nrm = q.normal + (size_t)t * kLmWords;

    if (q.phase & 1) {  // accept or reject the candidate whose normal-equation pass ran last
        const float lc = q.loss_cand[t];
        const float lam = q.damping[t];
        if (lc < q.loss[t]) {  // (NaN never accepts)
            if (lane < K && lane < nc) {
                const int c = s_cidx[lane];
                q.value[row + c] = q.cand[row + c];
            }
            if (lane < kLmWords) nrm[lane] = q.normal_cand[(size_t)t * kLmWords + lane];
            if (lane == 0) { q.loss[t] = lc; q.damping[t] = fmaxf(lam / 10.0f, kLmDampMin); }
        } else if (lane == 0) {
            q.damping[t] = fminf(10.0f * lam, kLmDampMax);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (q.phase & 2) {  // propose c + delta, (A + lambda diag A) delta = -b over the constants that influence the prediction
        const float l = q.loss[t];
        const double lam = (double)q.damping[t];
        double M[K][K], rhs[K];
        bool act[K];
        bool move = __builtin_isfinite(l) && l != 0.0f;
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < K; ++i) {
#pragma unroll
                for (int j = i; j < K; ++j, ++k) M[i][j] = (double)nrm[k];
                rhs[i] = -(double)nrm[kLmTri + i];
            }
        }
#pragma unroll
        for (int i = 0; i < K; ++i) act[i] = i < nc && M[i][i] != 0.0;   // (a NaN diagonal is "active" and stops the tree below)
        bool any = false;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            any = any || act[i];
#pragma unroll
            for (int j = i; j < K; ++j) {
                const bool used = act[i] && act[j];
                if (used && !__builtin_isfinite(M[i][j])) move = false;
                if (!used) M[i][j] = i == j ? 1.0 : 0.0;   // a dropped constant: an identity row, delta = 0
            }
            if (act[i] && !__builtin_isfinite(rhs[i])) move = false;
            if (!act[i]) rhs[i] = 0.0;
            if (act[i]) M[i][i] += lam * M[i][i];
        }
        move = move && any;
        // Cholesky M = U^T U on the upper triangle, in place
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double piv = M[i][i];
#pragma unroll
            for (int k = 0; k < i; ++k) piv -= M[k][i] * M[k][i];
            if (!(piv > 0.0)) move = false;
            const double u = sqrt(piv);
            M[i][i] = u;
#pragma unroll
            for (int j = i + 1; j < K; ++j) {
                double s = M[i][j];
#pragma unroll
                for (int k = 0; k < i; ++k) s -= M[k][i] * M[k][j];
                M[i][j] = s / u;
            }
        }
#pragma unroll
        for (int i = 0; i < K; ++i) {   // U^T z = rhs
            double s = rhs[i];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= M[k][i] * rhs[k];
            rhs[i] = s / M[i][i];
        }
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {   // U delta = z
            double s = rhs[i];
#pragma unroll
            for (int k = i + 1; k < K; ++k) s -= M[i][k] * rhs[k];
            rhs[i] = s / M[i][i];
        }
        float nv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            nv[j] = 0.0f;
            if (j < nc) {
                const float c = q.value[row + cidx[j]];
                nv[j] = act[j] ? (float)((double)c + rhs[j]) : c;
                if (!__builtin_isfinite(nv[j]) && act[j]) move = false;
            }
        }
        for (int i = lane; i < q.gp_len; i += kWave) {
            float v = q.value[row + i];
            if (move) {
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (i == cidx[j]) v = nv[j];
            }
            q.cand[row + i] = v;
        }
    }
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_normal_eq(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                      const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                      const float *labels, float *loss, float *normal, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len != 1 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !labels || !loss || !normal) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    NormalEqParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.loss = loss; p.normal = normal;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, lm_lds_head_words, &plan)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if (const hipError_t e = grant_tape_lds(grant, {(const void *)sr_normal_eq_kernel<>})) return (int)e;
    hipLaunchKernelGGL(sr_normal_eq_kernel<>, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_weighted_normal_eq(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                               const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                               const float *labels, const float *weights, float *loss, float *normal,
                                               evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    if (!value || !type || !size || !variables || !labels || !loss || !normal) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    WNormalEqParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.loss = loss; p.normal = normal;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    p.w = weights;
    hipError_t e;
    if (weights) {   // the row's sum and whether it may be used stay on the device (sr_wloss.hip's rule and kernel)
        WeightStatOut out{};
        out.slot[0] = (WeightStat *)acquire_counter(stream, &e);
        if (!out.slot[0]) return (int)e;
        p.stat = out.slot[0];
        hipLaunchKernelGGL(weight_stats_kernel, dim3(1), dim3(kStatsThreads), 0, stream, weights, p.D, 1, out);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, lm_lds_head_words, &plan)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if ((e = grant_tape_lds(grant, {(const void *)sr_normal_eq_kernel<true>})) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sr_normal_eq_kernel<true>, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_lm_step(unsigned pop_size, unsigned gp_len, unsigned out_len, int phase, float *value, const int16_t *type,
                                    const int16_t *size, float *value_cand, float *loss, float *normal, const float *loss_cand,
                                    const float *normal_cand, float *damping, evogp_stream_t stream_) {
    if (pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || out_len != 1 || pop_size > 0x7FFFFFFFu || phase < 1 || phase > 3)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !value_cand || !loss || !normal || !damping) return EVOGP_E_NULLPTR;
    if ((phase & 1) && (!loss_cand || !normal_cand)) return EVOGP_E_NULLPTR;
    LmStepParams q{};
    q.value = value; q.type = type; q.size = size; q.cand = value_cand; q.loss = loss; q.normal = normal;
    q.loss_cand = loss_cand; q.normal_cand = normal_cand; q.damping = damping;
    q.pop = (int)pop_size; q.gp_len = (int)gp_len; q.phase = phase;
    const unsigned blocks = (pop_size + 3) / 4;
    hipLaunchKernelGGL(sr_lm_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, q);
    return (int)hipGetLastError();
}
