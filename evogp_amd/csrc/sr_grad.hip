// sr_grad.hip — reverse-mode (adjoint) gradient of the symbolic-regression loss with respect to every constant node, and one
// iteration of the per-tree constant descent that uses it (gfx950).
//
//   loss[t]    = (1/D) * sum_d sum_o err(y[d][o] - tree_t(X[d])_o)          err = square | abs  (what sr_fitness.hip returns)
//   grad[t][i] = d loss[t] / d value[t][i]   for every CONST node i; exactly 0 at every other node and on the tail [len, gp_len)
//
// The forward semantics are run_general's (interp.hpp), both output modes; the derivative table is DESIGN.md's "Constant gradients".
//
// Work decomposition:
//   * one workgroup owns one tree at a time (grid-stride over the population); wave 0 classifies it (classify_tree) and builds its
//     OPERAND TABLE in LDS: for every function node the indices of the nodes whose pushed values it pops (a stack of node indices,
//     walked once per tree in execution order -- the tree's structure is wave-uniform, so nothing of it is per row);
//   * the W waves of the workgroup share the row tiles (64 rows each: wave w takes tiles w, w + W, ...).  Per tile a wave walks the
//     tree in execution order (reverse prefix) writing every node's pushed value into a TAPE [node][lane], then in prefix order
//     (parents before children) writing each operand's adjoint into a second [node][lane] array.  The adjoint slot of a CONST node
//     is an accumulator instead (zeroed once per tree, only valid rows added), so after the last tile it holds the lane's sum over
//     the wave's rows;
//   * every CONST slot is reduced over the lanes with the fixed DPP butterfly (wave_sum), the waves' partials are added in wave
//     order by one thread per node: no float atomics, bit-identical from run to run.
//
// The tapes live in LDS for rows of at most kTapeLdsLen nodes (2 x 64 x 256 B = 32 KiB per wave) and in the per-stream global
// workspace of the tape kernels for longer rows, one slice of 2 x gp_len x 256 B per resident wave.  Every access is a [node][lane]
// column: 64 consecutive floats, one per lane, conflict-free in LDS and one coalesced 256-byte line in memory.  Waves, workgroups, LDS
// bytes and the workspace come from the plan the three tape passes share (sr_forward.hpp plan_tape_launch).
//
// The WEIGHTED build (WL, evogp_hip_sr_weighted_gradient: single-output trees) is the same walk with another epilogue: the row's
// weight is read next to y and `valid` also asks for w != 0 (a tile without a weighted row is skipped whole), the loss is
// sum w rho(r) in float64 per lane (wave_sum_d, then the waves in wave order) over Wsum, the reverse walk is seeded with
// w rho'(r) / Wsum, and a non-finite prediction on a weighted row makes the tree NaN (sr_wloss.hip's rule).
#include <type_traits>

#include "sr_adjoint.hpp"
#include "sr_moments.hpp"

namespace evogp {

struct GradParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;  // [D][var_len]
    const float *y;  // [D][out_len]
    float *loss;     // [pop]
    float *grad;     // [pop][gp_len]
    float *tape;     // global tapes (rows longer than kTapeLdsLen): [blocks * W][2][gp_len][64]; nullptr: the tapes are in LDS
    int pop, D, gp_len, var_len, out_len, use_mse;
};

struct WGradParams : GradParams {   // the weighted build's
    const float *w;           // [D], or nullptr: every weight is 1
    const WeightStat *stat;   // the weight row's sum and whether it may be used (weight_stats_kernel); nullptr without w
    double prm;               // delta (huber) or tau (pinball)
    int kind;
};

// Dynamic LDS of one workgroup (16-byte aligned carve): op[L] kids[L] pay[L] stack[L] (u32), part[W][L], lpart[W], cls/len (2 words,
// padded to 4), then, for LDS tapes, W x 2 x L x 64 floats.
__host__ __device__ inline size_t grad_lds_head_words(int L, int W) { return (((size_t)4 * L + (size_t)W * L + W + 4) + 3) & ~(size_t)3; }

// the weighted build's head: lpart is W doubles on an 8-byte boundary, followed by the waves' "met a non-finite prediction" words
__host__ __device__ inline size_t wgrad_lpart_word(int L, int W) { return (((size_t)4 * L + (size_t)W * L) + 1) & ~(size_t)1; }
__host__ __device__ inline size_t wgrad_lds_head_words(int L, int W) { return ((wgrad_lpart_word(L, W) + (size_t)3 * W + 4) + 3) & ~(size_t)3; }

template <bool MO, bool WL = false>
__global__ __launch_bounds__(kTapeMaxWaves * 64) void sr_grad_kernel(std::conditional_t<WL, WGradParams, GradParams> p) {
    static_assert(!(MO && WL), "the weighted build takes single-output trees");
    extern __shared__ __attribute__((aligned(16))) uint32_t grad_lds[];
    const int L = p.gp_len;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    uint32_t *s_op = grad_lds, *s_kid = s_op + L, *s_pay = s_kid + L;
    int *s_stk = (int *)(s_pay + L);
    float *s_part = (float *)(s_stk + L);
    float *s_lpart = s_part + (size_t)W * L;
    double *s_dpart = (double *)(grad_lds + wgrad_lpart_word(L, W));   // (weighted build)
    int *s_bad = (int *)(s_dpart + W);
    int *s_meta = WL ? s_bad + W : (int *)(s_lpart + W);
    float *tape = p.tape ? p.tape + ((size_t)blockIdx.x * W + w) * 2 * L * kWave
                         : (float *)(grad_lds + (WL ? wgrad_lds_head_words(L, W) : grad_lds_head_words(L, W))) + (size_t)w * 2 * L * kWave;
    float *val = tape, *adj = tape + (size_t)L * kWave;
    const int ntiles = (p.D + kWave - 1) / kWave;
    const float inv_d = 1.0f / (float)p.D;
    double wsum = (double)p.D;
    bool usable = true;
    if constexpr (WL) {
        if (p.w) { wsum = p.stat->sum; usable = p.stat->usable != 0; }
    }

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        const size_t row = (size_t)t * L;
        if (WL && !usable) {  // a weight row that may not be used: NaN loss, zero row, for every tree
            for (int i = threadIdx.x; i < L; i += blockDim.x) p.grad[row + i] = 0.0f;
            if (threadIdx.x == 0) p.loss[t] = __builtin_nanf("");
            continue;
        }
        // ---- wave 0: classify, decode, operand table ----
        if (w == 0) {
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > L ? L : len);
            const int cls = uni(classify_tree(p.type + row, p.value + row, len, MO, p.var_len, p.out_len, kMaxStack));
            if (cls == TREE_OK) build_operand_table<MO>(p.type, p.value, row, len, p.var_len, p.out_len, s_op, s_kid, s_pay, s_stk);
            if (lane == 0) { s_meta[0] = cls; s_meta[1] = len; }
        }
        __syncthreads();
        const int cls = uni(s_meta[0]);
        const int len = uni(s_meta[1]);
        if (cls != TREE_OK) {  // malformed: NaN loss, zero row
            for (int i = threadIdx.x; i < L; i += blockDim.x) p.grad[row + i] = 0.0f;
            if (threadIdx.x == 0) p.loss[t] = __builtin_nanf("");
            __syncthreads();
            continue;
        }
        for (int i = 0; i < len; ++i)
            if ((uni((int)s_op[i]) & kOpMask) == H_CONST) adj[i * kWave + lane] = 0.0f;

        // adjoint of operand k of a node whose word is `opw`: stored, or added for a CONST operand (valid rows only)
        auto put = [&](uint32_t opw, uint32_t kid, int k, float x, bool valid) {
            const int c = (int)((kid >> (10 * k)) & 1023u);
            float *q = adj + c * kWave + lane;
            if (opw & (1u << (8 + k))) *q += valid ? x : 0.0f;
            else *q = x;
        };

        float acc = 0.0f;
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
            v16f outs, gout;
            if (MO) {
#pragma unroll
                for (int o = 0; o < kMaxOutRegs; ++o) outs[o] = 0.0f;
            }
            // ---- forward: execution order, every node's pushed value on the tape ----
            for (int i = len - 1; i >= 0; --i) {
                const uint32_t op = (uint32_t)uni((int)s_op[i]) & kOpMask;
                float v;
                if (op < H_ADD) {
                    const uint32_t pay = (uint32_t)uni((int)s_pay[i]);
                    v = op == H_CONST ? bits2f(pay) : xr[pay];
                } else {
                    const uint32_t kid = (uint32_t)uni((int)s_kid[i]);
                    const float a = val[(kid & 1023u) * kWave + lane];
                    float r, last;
                    if (op < H_UN) {
                        const float b = val[((kid >> 10) & 1023u) * kWave + lane];
                        r = binary_value(op, a, b);
                        last = b;
                    } else if (op < H_IF) {
                        r = op_unary<false>(op, a);
                        last = a;
                    } else {
                        const float b = val[((kid >> 10) & 1023u) * kWave + lane], c = val[(kid >> 20) * kWave + lane];
                        r = a > 0.0f ? b : c;
                        last = c;
                    }
                    if (MO) {
                        const uint32_t pay = (uint32_t)uni((int)s_pay[i]);
                        if (pay != kNoOut) outs[pay] += r;
                        v = last;
                    } else {
                        v = r;
                    }
                }
                val[i * kWave + lane] = v;
            }
            // ---- loss and the adjoints of the outputs ----
            float e = 0.0f, g0 = 0.0f;
            if constexpr (WL) {
                const float pred = val[lane];
                const double r = (double)pred - (double)p.y[dc];
                const bool lc = p.kind == EVOGP_LOSS_LOGCOSH;   // (wave-uniform)
                const double term = valid ? (double)wv * (lc ? wloss_rho<true>(p.kind, p.prm, r) : wloss_rho<false>(p.kind, p.prm, r)) : 0.0;
                dacc += term;
                bad |= valid && !finite_f(pred);
                const double dr = lc ? wloss_drho<true>(p.kind, p.prm, r) : wloss_drho<false>(p.kind, p.prm, r);
                g0 = valid ? (float)((double)wv * dr / wsum) : 0.0f;
            } else if (!MO) {
                const float pred = val[lane], yv = p.y[dc];
                e = grad_err(yv - pred, p.use_mse);
                const float diff = pred - yv;
                g0 = valid ? (p.use_mse ? 2.0f * diff * inv_d : sign_of(diff) * inv_d) : 0.0f;
            } else {
                const float *yr = p.y + (size_t)dc * p.out_len;
#pragma unroll
                for (int o = 0; o < kMaxOutRegs; ++o) {
                    gout[o] = 0.0f;
                    if (o < p.out_len) {
                        e += grad_err(yr[o] - outs[o], p.use_mse);
                        const float diff = outs[o] - yr[o];
                        gout[o] = valid ? (p.use_mse ? 2.0f * diff * inv_d : sign_of(diff) * inv_d) : 0.0f;
                    }
                }
            }
            acc += valid ? e : 0.0f;
            // ---- reverse: prefix order, parents before children ----
            {   // the root's pushed value: the prediction (single output) or nothing (multi-output: the outputs are the sums)
                const uint32_t op0 = (uint32_t)uni((int)s_op[0]) & kOpMask;
                const float x = MO ? 0.0f : g0;
                if (op0 == H_CONST) adj[lane] += valid ? x : 0.0f;
                else adj[lane] = x;
            }
            for (int i = 0; i < len; ++i) {
                const uint32_t opw = (uint32_t)uni((int)s_op[i]);
                const uint32_t op = opw & kOpMask;
                if (op < H_ADD) continue;
                const uint32_t kid = (uint32_t)uni((int)s_kid[i]);
                const float g = adj[i * kWave + lane];
                const float a = val[(kid & 1023u) * kWave + lane];
                uint32_t pay = kNoOut;
                if (MO) pay = (uint32_t)uni((int)s_pay[i]);
                const bool through = !MO || pay != kNoOut;  // does the node's result r reach the loss?
                float gr = g;
                if (MO) gr = through ? gout[pay] : 0.0f;
                if (op < H_UN) {
                    const float b = val[((kid >> 10) & 1023u) * kWave + lane];
                    float da = 0.0f, db = 0.0f;
                    if (through) {
                        const float r = MO ? binary_value(op, a, b) : val[i * kWave + lane];
                        binary_adjoint(op, a, b, r, gr, da, db);
                    }
                    if (MO) db += g;  // the passed operand
                    put(opw, kid, 0, da, valid);
                    put(opw, kid, 1, db, valid);
                } else if (op < H_IF) {
                    float da = 0.0f;
                    if (through) {
                        const float r = MO ? op_unary<false>(op, a) : val[i * kWave + lane];
                        da = unary_adjoint(op, a, r, gr);
                    }
                    if (MO) da += g;
                    put(opw, kid, 0, da, valid);
                } else {
                    const bool take_b = a > 0.0f;
                    float db = through && take_b ? gr : 0.0f, dcv = through && !take_b ? gr : 0.0f;
                    if (MO) dcv += g;
                    put(opw, kid, 0, 0.0f, valid);
                    put(opw, kid, 1, db, valid);
                    put(opw, kid, 2, dcv, valid);
                }
            }
        }

        // ---- reduce: lanes by the fixed butterfly, waves in wave order ----
        for (int i = 0; i < len; ++i) {
            if ((uni((int)s_op[i]) & kOpMask) != H_CONST) continue;
            const float s = wave_sum(adj[i * kWave + lane]);
            if (lane == 0) s_part[(size_t)w * L + i] = s;
        }
        if (WL) {
            const double s = wave_sum_d(dacc);
            const int wbad = __any(bad) ? 1 : 0;
            if (lane == 0) { s_dpart[w] = s; s_bad[w] = wbad; }
        } else {
            const float s = wave_sum(acc);
            if (lane == 0) s_lpart[w] = s;
        }
        __syncthreads();
        bool ok = true;   // (weighted build) no weighted row with a non-finite prediction
        if (WL)
            for (int k = 0; k < W; ++k) ok = ok && s_bad[k] == 0;
        for (int i = threadIdx.x; i < L; i += blockDim.x) {
            float s = 0.0f;
            if (i < len && (s_op[i] & kOpMask) == H_CONST)
                for (int k = 0; k < W; ++k) s += s_part[(size_t)k * L + i];
            p.grad[row + i] = ok ? s : 0.0f;
        }
        if (threadIdx.x == 0) {
            if (WL) {
                double s = 0.0;
                for (int k = 0; k < W; ++k) s += s_dpart[k];
                p.loss[t] = ok ? (float)(s / wsum) : __builtin_nanf("");
            } else {
                float s = 0.0f;
                for (int k = 0; k < W; ++k) s += s_lpart[k];
                p.loss[t] = s / (float)p.D;
            }
        }
        __syncthreads();  // the tables are rebuilt for the next tree
    }
}

// ---- one iteration of the per-tree descent (evogp_hip_sr_const_step) ----------------------------------------------------------
struct StepParams {
    float *value;            // [pop][gp_len] current constants (only CONST words of the live prefix are written)
    const int16_t *type;
    const int16_t *size;
    float *cand;             // [pop][gp_len] candidate forest (every word written when proposing)
    float *loss;             // [pop] loss of the current forest
    float *grad;             // [pop][gp_len] its gradient
    const float *loss_cand;  // [pop] loss of the candidate forest (accepting)
    const float *grad_cand;  // [pop][gp_len] its gradient
    float *step;             // [pop] step length h_t
    int pop, gp_len, multi, phase;
};

__device__ inline bool is_const_node(int type, bool multi) { return (multi ? (type & T_MASK) : type) == T_CONST; }

__global__ __launch_bounds__(256) void sr_const_step_kernel(StepParams q) {
    const int lane = threadIdx.x & 63;
    const int t = uni((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (t >= q.pop) return;
    const size_t row = (size_t)t * q.gp_len;
    int len = uni((int)q.size[row]);
    len = len < 0 ? 0 : (len > q.gp_len ? q.gp_len : len);
    const bool multi = q.multi != 0;
    if (q.phase & 1) {  // accept or reject the candidate whose gradient pass ran last
        const float lc = q.loss_cand[t];
        if (lc < q.loss[t]) {  // (NaN never accepts)
            for (int i = lane; i < q.gp_len; i += kWave) {
                if (i < len && is_const_node(q.type[row + i], multi)) q.value[row + i] = q.cand[row + i];
                q.grad[row + i] = q.grad_cand[row + i];
            }
            if (lane == 0) { q.loss[t] = lc; q.step[t] = 2.0f * q.step[t]; }
        } else if (lane == 0) {
            q.step[t] = 0.5f * q.step[t];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (q.phase & 2) {  // propose c - h * g / |g|
        float s = 0.0f;
        for (int i = lane; i < q.gp_len; i += kWave) { const float g = q.grad[row + i]; s += g * g; }
        const float norm = sqrtf(wave_sum(s));
        const float l = q.loss[t], h = q.step[t];
        const bool move = __builtin_isfinite(l) && l != 0.0f && __builtin_isfinite(norm) && norm != 0.0f;
        for (int i = lane; i < q.gp_len; i += kWave) {
            float v = q.value[row + i];
            if (move && i < len && is_const_node(q.type[row + i], multi)) v = v - h * q.grad[row + i] / norm;
            q.cand[row + i] = v;
        }
    }
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_gradient(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                     int use_mse, const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                     const float *labels, float *loss, float *grad, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !labels || !loss || !grad) return EVOGP_E_NULLPTR;
    if (out_len > (unsigned)kMaxOutRegs) return EVOGP_E_UNSUPPORTED;
    const hipStream_t stream = (hipStream_t)stream_;
    GradParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.loss = loss; p.grad = grad;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.out_len = (int)out_len;
    p.use_mse = use_mse ? 1 : 0;
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, grad_lds_head_words, &plan)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if (const hipError_t e = grant_tape_lds(grant, {(const void *)sr_grad_kernel<true>, (const void *)sr_grad_kernel<false>})) return (int)e;
    if (p.out_len > 1) hipLaunchKernelGGL(sr_grad_kernel<true>, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    else hipLaunchKernelGGL(sr_grad_kernel<false>, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_weighted_gradient(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                              const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                              const float *labels, const float *weights, int loss_kind, double loss_param, float *loss,
                                              float *grad, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (loss_kind < EVOGP_LOSS_MSE || loss_kind > EVOGP_LOSS_LOGCOSH || loss_param != loss_param) return EVOGP_E_BADARG;
    if (loss_kind == EVOGP_LOSS_HUBER && !(loss_param > 0.0 && loss_param < HUGE_VAL)) return EVOGP_E_BADARG;
    if (loss_kind == EVOGP_LOSS_PINBALL && !(loss_param > 0.0 && loss_param < 1.0)) return EVOGP_E_BADARG;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    if (!value || !type || !size || !variables || !labels || !loss || !grad) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    WGradParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.loss = loss; p.grad = grad;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.out_len = 1;
    p.w = weights; p.kind = loss_kind; p.prm = loss_param;
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
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, wgrad_lds_head_words, &plan)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if ((e = grant_tape_lds(grant, {(const void *)sr_grad_kernel<false, true>})) != hipSuccess) return (int)e;
    hipLaunchKernelGGL((sr_grad_kernel<false, true>), dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_const_step(unsigned pop_size, unsigned gp_len, unsigned out_len, int phase, float *value, const int16_t *type,
                                       const int16_t *size, float *value_cand, float *loss, float *grad, const float *loss_cand,
                                       const float *grad_cand, float *step, evogp_stream_t stream_) {
    if (pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || out_len == 0 || pop_size > 0x7FFFFFFFu || phase < 1 || phase > 3)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !value_cand || !loss || !grad || !step) return EVOGP_E_NULLPTR;
    if ((phase & 1) && (!loss_cand || !grad_cand)) return EVOGP_E_NULLPTR;
    StepParams q{};
    q.value = value; q.type = type; q.size = size; q.cand = value_cand; q.loss = loss; q.grad = grad;
    q.loss_cand = loss_cand; q.grad_cand = grad_cand; q.step = step;
    q.pop = (int)pop_size; q.gp_len = (int)gp_len; q.multi = out_len > 1 ? 1 : 0; q.phase = phase;
    const unsigned blocks = (pop_size + 3) / 4;
    hipLaunchKernelGGL(sr_const_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, q);
    return (int)hipGetLastError();
}
