// sr_xgrad.hip — reverse-mode (adjoint) gradient of a single-output tree with respect to its INPUTS on the rows of the dataset, and the
// derivative loss that is computed from it without writing a (pop, D) array (gfx950).  DESIGN.md section 3.23.
//
//   pred[t][d]     = tree_t(X[d])                                     the bits of the tape's forward walk (run_general's semantics)
//   dpred[k][t][d] = d tree_t / d x_{wrt[k]} at X[d]                  k < V <= kXgradMaxVars requested variables
//
// The walk is sr_grad.hip's, specialised: single output, the reverse walk seeded with 1.0f at the root, every adjoint a plain store (there
// is no accumulator slot: nothing is summed over the rows).  After the reverse walk the adjoint slot of a VAR node holds the adjoint of
// that OCCURRENCE of the variable; the derivative in variable wrt[k] is the float32 sum, from +0.0f, of the slots of the VAR nodes whose
// decoded index is wrt[k], in prefix order.  The walk visits a node after its parent, so a VAR node's slot is final when the walk reaches
// it and the sum is taken there.  A variable the tree does not hold has +0.0f exactly, a root that is a VAR 1.0f.
//
// NaN rules: they are the constant gradient's (sr_adjoint.hpp), unrepaired.  An adjoint is a product of the parent's adjoint and a local
// partial, and 0 * NaN is NaN: an IF passes 0 to its untaken branch, max / min pass 0 to the operand that lost, and a NaN or infinite
// VALUE inside that branch can make the local partials below it NaN.  A derivative may therefore be NaN on a row whose prediction is
// finite.  Such a row counts as a violation and makes its loss column NaN (below).
//
// Which running sum a VAR node adds to is wave-uniform: wave 0 writes the column of the variable (1 + k, 0: not requested) into the top
// four bits of the node's payload word when it builds the operand table, and the walk selects the sum by a uniform switch over named
// registers (no dynamically indexed register array, no var_len-sized table, no scratch).
//
// FUSED == false materialises pred [pop][D] and dpred [V][pop][D]: a lane stores its row, 64 consecutive floats per wave and array.  A
// malformed tree's rows are NaN in both.
// FUSED == true writes loss [pop][1 + V] and viol [pop][V] only:
//   loss[t][0]     = (float)( sum_d r_d^2 / D ),  r_d = (double)pred - (double)y[d]: per-lane float64 in ascending tile order, wave_sum_d,
//                    the waves in wave order -- the association of the weighted build of sr_grad_kernel, whose MSE without weights it
//                    equals bit for bit (same plan, same forward walk);
//   loss[t][1 + k] = (float)( sum_d ((double)g_k - (double)dy[d][k])^2 / D ), the same way; dy == nullptr: labels of zero;
//   a column is NaN exactly when one of its row terms is not finite (a flag per column and wave);
//   viol[t][k]     = number of rows with !(dmin[k] <= g_k && g_k <= dmax[k]) (a NaN derivative counts; nullptr bounds: -inf / +inf):
//                    ballot and popcount per tile, integer sums per wave, the waves in wave order;
//   a malformed tree has every column NaN and viol = D.
// No float atomics, nothing synchronises with the host: the same inputs give the same bits.
#include "sr_adjoint.hpp"
#include "sr_moments.hpp"

namespace evogp {

constexpr int kXgradMaxVars = EVOGP_XGRAD_MAX_VARS;
constexpr uint32_t kXgradVarMask = 0x0FFFFFFFu;   // payload of a VAR node: the variable in bits 0..27, its column + 1 in bits 28..31

struct XgradParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;      // [D][var_len]
    const float *y;      // [D]            (fused)
    const float *dy;     // [D][V] or nullptr: zeros (fused)
    const float *dmin;   // [V] or nullptr: -inf (fused)
    const float *dmax;   // [V] or nullptr: +inf (fused)
    float *pred;         // [pop][D]       (materialising)
    float *dpred;        // [V][pop][D]    (materialising)
    float *loss;         // [pop][1 + V]   (fused)
    int *viol;           // [pop][V]       (fused)
    float *tape;         // global tapes (rows longer than kTapeLdsLen): [blocks * W][2][gp_len][64]; nullptr: the tapes are in LDS
    int wrt[kXgradMaxVars];
    int pop, D, gp_len, var_len, V;
};

// Dynamic LDS of one workgroup in front of the tapes, sized for V = 8: op[L] kids[L] pay[L] stack[L] (u32), dpart[W][9] (double, on an
// 8-byte boundary: 4 L is even), bad[W], viol[W][8], cls / len.
constexpr int kXgradCols = 1 + kXgradMaxVars;
__host__ __device__ inline size_t xgrad_lds_head_words(int L, int W) {
    return (((size_t)4 * L + (size_t)W * (2 * kXgradCols + 1 + kXgradMaxVars) + 2) + 3) & ~(size_t)3;
}

template <bool FUSED>
__global__ __launch_bounds__(kTapeMaxWaves * 64) void sr_xgrad_kernel(XgradParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t xgrad_lds[];
    const int L = p.gp_len;
    const int V = p.V;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    uint32_t *s_op = xgrad_lds, *s_kid = s_op + L, *s_pay = s_kid + L;
    int *s_stk = (int *)(s_pay + L);
    double *s_dpart = (double *)(s_stk + L);
    int *s_bad = (int *)(s_dpart + (size_t)W * kXgradCols);
    int *s_viol = s_bad + W;
    int *s_meta = s_viol + W * kXgradMaxVars;
    float *tape = p.tape ? p.tape + ((size_t)blockIdx.x * W + w) * 2 * L * kWave
                         : (float *)(xgrad_lds + xgrad_lds_head_words(L, W)) + (size_t)w * 2 * L * kWave;
    float *val = tape, *adj = tape + (size_t)L * kWave;
    const int ntiles = (p.D + kWave - 1) / kWave;
    const float nanf_ = __builtin_nanf("");

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        const size_t row = (size_t)t * L;
        // ---- wave 0: classify, decode, operand table, the columns of the VAR nodes ----
        if (w == 0) {
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > L ? L : len);
            const int cls = uni(classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, kMaxStack));
            if (cls == TREE_OK) {
                build_operand_table<false>(p.type, p.value, row, len, p.var_len, 1, s_op, s_kid, s_pay, s_stk);
                for (int i = lane; i < len; i += kWave) {
                    if ((s_op[i] & kOpMask) != H_VAR) continue;
                    const uint32_t v = s_pay[i] & kXgradVarMask;
                    uint32_t col = 0;
#pragma unroll
                    for (int k = 0; k < kXgradMaxVars; ++k)
                        if (k < V && v == (uint32_t)p.wrt[k]) col = (uint32_t)k + 1u;
                    s_pay[i] = v | (col << 28);
                }
            }
            if (lane == 0) { s_meta[0] = cls; s_meta[1] = len; }
        }
        __syncthreads();
        const int cls = uni(s_meta[0]);
        const int len = uni(s_meta[1]);
        if (cls != TREE_OK) {  // malformed: NaN rows (materialising); NaN columns and D violations (fused)
            if (FUSED) {
                if ((int)threadIdx.x <= V) p.loss[(size_t)t * (1 + V) + threadIdx.x] = nanf_;
                if ((int)threadIdx.x < V) p.viol[(size_t)t * V + threadIdx.x] = p.D;
            } else {
                for (int d = threadIdx.x; d < p.D; d += blockDim.x) {
                    p.pred[(size_t)t * p.D + d] = nanf_;
                    for (int k = 0; k < V; ++k) p.dpred[((size_t)k * p.pop + t) * p.D + d] = nanf_;
                }
            }
            __syncthreads();
            continue;
        }

        double dacc[kXgradCols];   // (fused) the lane's float64 sums, one per column; every index below is a constant after unrolling
        int vcnt[kXgradMaxVars];   // (fused, wave-uniform) violating rows of the wave's tiles
        int bad = 0;               // (fused) bit c: a row term of column c was not finite
#pragma unroll
        for (int c = 0; c < kXgradCols; ++c) dacc[c] = 0.0;
#pragma unroll
        for (int k = 0; k < kXgradMaxVars; ++k) vcnt[k] = 0;

        for (int tile = w; tile < ntiles; tile += W) {
            const int d = tile * kWave + lane;
            const bool valid = d < p.D;
            const int dc = valid ? d : p.D - 1;
            const float *xr = p.X + (size_t)dc * p.var_len;
            // ---- forward: execution order, every node's value on the tape ----
            for (int i = len - 1; i >= 0; --i) {
                const uint32_t op = (uint32_t)uni((int)s_op[i]) & kOpMask;
                float v;
                if (op < H_ADD) {
                    const uint32_t pay = (uint32_t)uni((int)s_pay[i]);
                    v = op == H_CONST ? bits2f(pay) : xr[pay & kXgradVarMask];
                } else {
                    const uint32_t kid = (uint32_t)uni((int)s_kid[i]);
                    const float a = val[(kid & 1023u) * kWave + lane];
                    if (op < H_UN) {
                        const float b = val[((kid >> 10) & 1023u) * kWave + lane];
                        v = binary_value(op, a, b);
                    } else if (op < H_IF) {
                        v = op_unary<false>(op, a);
                    } else {
                        const float b = val[((kid >> 10) & 1023u) * kWave + lane], c = val[(kid >> 20) * kWave + lane];
                        v = a > 0.0f ? b : c;
                    }
                }
                val[i * kWave + lane] = v;
            }
            // ---- reverse: prefix order, parents before children; a VAR node's slot is final when the walk reaches it ----
            float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f, g4 = 0.0f, g5 = 0.0f, g6 = 0.0f, g7 = 0.0f;
            adj[lane] = 1.0f;
            for (int i = 0; i < len; ++i) {
                const uint32_t op = (uint32_t)uni((int)s_op[i]) & kOpMask;
                if (op < H_ADD) {
                    if (op == H_VAR) {
                        const uint32_t col = (uint32_t)uni((int)s_pay[i]) >> 28;
                        if (col != 0) {
                            const float x = adj[i * kWave + lane];
                            switch (col) {   // (wave-uniform)
                            case 1: g0 += x; break;
                            case 2: g1 += x; break;
                            case 3: g2 += x; break;
                            case 4: g3 += x; break;
                            case 5: g4 += x; break;
                            case 6: g5 += x; break;
                            case 7: g6 += x; break;
                            default: g7 += x; break;
                            }
                        }
                    }
                    continue;
                }
                const uint32_t kid = (uint32_t)uni((int)s_kid[i]);
                const float g = adj[i * kWave + lane];
                const float a = val[(kid & 1023u) * kWave + lane];
                if (op < H_UN) {
                    const float b = val[((kid >> 10) & 1023u) * kWave + lane];
                    float da, db;
                    binary_adjoint(op, a, b, val[i * kWave + lane], g, da, db);
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
            const float gs[kXgradMaxVars] = {g0, g1, g2, g3, g4, g5, g6, g7};
            const float pred = val[lane];
            if (FUSED) {
                const double r = (double)pred - (double)p.y[dc];
                const double t0 = r * r;
                dacc[0] += valid ? t0 : 0.0;
                bad |= valid && !__builtin_isfinite(t0) ? 1 : 0;
#pragma unroll
                for (int k = 0; k < kXgradMaxVars; ++k) {
                    if (k < V) {   // (wave-uniform)
                        const float label = p.dy ? p.dy[(size_t)dc * V + k] : 0.0f;
                        const double e = (double)gs[k] - (double)label;
                        const double tk = e * e;
                        dacc[1 + k] += valid ? tk : 0.0;
                        bad |= valid && !__builtin_isfinite(tk) ? 2 << k : 0;
                        const float lo = p.dmin ? p.dmin[k] : -__builtin_inff(), hi = p.dmax ? p.dmax[k] : __builtin_inff();
                        vcnt[k] += __popcll(__ballot(valid && !(lo <= gs[k] && gs[k] <= hi)));
                    }
                }
            } else if (valid) {
                p.pred[(size_t)t * p.D + d] = pred;
#pragma unroll
                for (int k = 0; k < kXgradMaxVars; ++k)
                    if (k < V) p.dpred[((size_t)k * p.pop + t) * p.D + d] = gs[k];
            }
        }

        if (FUSED) {
            // ---- reduce: lanes by the fixed butterfly, waves in wave order ----
            int wbad = 0;
#pragma unroll
            for (int c = 0; c < kXgradCols; ++c) {
                if (c <= V) {
                    const double s = wave_sum_d(dacc[c]);
                    if (lane == 0) s_dpart[w * kXgradCols + c] = s;
                    if (__any((bad >> c) & 1)) wbad |= 1 << c;
                }
            }
            if (lane == 0) {
                s_bad[w] = wbad;
#pragma unroll
                for (int k = 0; k < kXgradMaxVars; ++k)
                    if (k < V) s_viol[w * kXgradMaxVars + k] = vcnt[k];
            }
            __syncthreads();
            const int c = (int)threadIdx.x;
            if (c <= V) {
                double s = 0.0;
                int anybad = 0;
                for (int k = 0; k < W; ++k) { s += s_dpart[k * kXgradCols + c]; anybad |= s_bad[k]; }
                p.loss[(size_t)t * (1 + V) + c] = (anybad >> c) & 1 ? nanf_ : (float)(s / (double)p.D);
            }
            if (c < V) {
                int n = 0;
                for (int k = 0; k < W; ++k) n += s_viol[k * kXgradMaxVars + c];
                p.viol[(size_t)t * V + c] = n;
            }
        }
        __syncthreads();  // the tables are rebuilt for the next tree
    }
}

}  // namespace evogp

using namespace evogp;

// the checks both entry points share, in the order of evogp_hip_sr_gradient: bad argument, null pointer, out_len
static int xgrad_check(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len, unsigned n_wrt,
                       const int *wrt) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || var_len > kXgradVarMask ||
        out_len == 0 || pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu || n_wrt == 0 || n_wrt > (unsigned)kXgradMaxVars)
        return EVOGP_E_BADARG;
    if (!wrt) return EVOGP_E_NULLPTR;
    for (unsigned k = 0; k < n_wrt; ++k) {
        if (wrt[k] < 0 || (unsigned)wrt[k] >= var_len) return EVOGP_E_BADARG;
        for (unsigned j = 0; j < k; ++j)
            if (wrt[j] == wrt[k]) return EVOGP_E_BADARG;
    }
    return 0;
}

template <bool FUSED>
static int xgrad_launch(XgradParams &p, unsigned n_wrt, const int *wrt, hipStream_t stream) {
    p.V = (int)n_wrt;
    for (int k = 0; k < kXgradMaxVars; ++k) p.wrt[k] = k < p.V ? wrt[k] : -1;
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, xgrad_lds_head_words, &plan)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if (const hipError_t e = grant_tape_lds(grant, {(const void *)sr_xgrad_kernel<FUSED>})) return (int)e;
    hipLaunchKernelGGL(sr_xgrad_kernel<FUSED>, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_input_gradient(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                           const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                           unsigned n_wrt, const int *wrt, float *pred, float *dpred, evogp_stream_t stream_) {
    if (const int rc = xgrad_check(pop_size, data_points, gp_len, var_len, out_len, n_wrt, wrt)) return rc;
    if (!value || !type || !size || !variables || !pred || !dpred) return EVOGP_E_NULLPTR;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    XgradParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.pred = pred; p.dpred = dpred;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    return xgrad_launch<false>(p, n_wrt, wrt, (hipStream_t)stream_);
}

extern "C" int evogp_hip_sr_derivative_loss(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                            const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                            const float *labels, const float *dlabels, unsigned n_wrt, const int *wrt, const float *dmin,
                                            const float *dmax, float *loss, int *violations, evogp_stream_t stream_) {
    if (const int rc = xgrad_check(pop_size, data_points, gp_len, var_len, out_len, n_wrt, wrt)) return rc;
    if (!value || !type || !size || !variables || !labels || !loss || !violations) return EVOGP_E_NULLPTR;
    if (out_len != 1) return EVOGP_E_UNSUPPORTED;
    XgradParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.dy = dlabels; p.dmin = dmin; p.dmax = dmax;
    p.loss = loss; p.viol = violations;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    return xgrad_launch<true>(p, n_wrt, wrt, (hipStream_t)stream_);
}
