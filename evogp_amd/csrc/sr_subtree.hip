// sr_subtree.hip — the loss of EVERY SUBTREE of every single-output tree as a model of its own, whether the subtree is constant over
// the dataset, and the rewrite that uses both: hoist the best subtree to the root, replace row-constant subtrees by CONST nodes (gfx950).
//
//   node_err[t][i]   = (1/D) * sum_d err(y[d] - v_i(X[d]))        v_i = the value of the subtree rooted at node i, err = square | abs
//   node_const[t][i] = c  when v_i(X[d]) has the bit pattern of c on every row d and c is not a NaN; NaN otherwise
//   both NaN on the tail [len, gp_len) and on every entry of a malformed tree (classify_tree != TREE_OK)
//
// sr_subtree_kernel is the forward half of sr_grad_kernel (sr_grad.hip, single-output mode, where the tape holds the value of every
// subtree on every row) with the same work decomposition: one workgroup owns a tree, wave 0 classifies it and builds the operand
// table, the W waves split the 64-row tiles.  Per tile a wave walks the tree in execution order writing v_i into the TAPE [node][lane]
// and adding the row's error into an ACCUMULATOR [node][lane] (valid rows only), the way the gradient kernel keeps its CONST adjoints.
// After the last tile every accumulator column is reduced over the lanes with the fixed DPP butterfly (wave_sum) and the waves'
// partials are added in wave order by one thread per node: no float atomics, bit-identical from run to run, and node_err[t][0] is
// the loss evogp_hip_sr_gradient returns, bit for bit.
// Constancy needs no per-lane storage: per wave and node the bit pattern the wave's first row gave (FIRST) and a flag "some lane of some
// tile of mine differed from it" (BAD), both in LDS; the last tile's lanes past D repeat row D - 1, so they cannot break it.  A node
// is constant when no wave saw a difference and the waves' FIRSTs are one pattern.
//
// Tape and accumulator live in LDS for rows of at most kTapeLdsLen nodes (2 x 64 x 256 B = 32 KiB per wave) and in the per-stream
// global workspace of the tape kernels (launches on one stream never overlap) for longer rows.  The launch is the plan the three tape
// passes share (sr_forward.hpp plan_tape_launch): the same rows meet the same order of summation as in the gradient pass.
//
// prune_rows_kernel: one wave per tree, the rule of include/evogp_hip.h evogp_hip_prune_rows (tests/subtree_ref.py restates it).
#include "sr_forward.hpp"

namespace evogp {

struct SubtreeParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;     // [D][var_len]
    const float *y;     // [D]
    float *node_err;    // [pop][gp_len]
    float *node_const;  // [pop][gp_len]
    float *tape;        // global tapes (rows longer than kTapeLdsLen): [blocks * W][2][gp_len][64]; nullptr: they are in LDS
    int pop, D, gp_len, var_len, use_mse;
};

// Dynamic LDS of one workgroup (16-byte aligned carve): op[L] kids[L] pay[L] stack[L] (u32), part[W][L] (float), first[W][L] bad[W][L]
// (u32), cls/len (2 words, padded to 4), then, for LDS tapes, W x 2 x L x 64 floats.
__host__ __device__ inline size_t subtree_lds_head_words(int L, int W) { return (((size_t)4 * L + (size_t)3 * W * L + 4) + 3) & ~(size_t)3; }

__global__ __launch_bounds__(kTapeMaxWaves * 64) void sr_subtree_kernel(SubtreeParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sub_lds[];
    const int L = p.gp_len;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    uint32_t *s_op = sub_lds, *s_kid = s_op + L, *s_pay = s_kid + L;
    int *s_stk = (int *)(s_pay + L);
    float *s_part = (float *)(s_stk + L);
    uint32_t *s_first = (uint32_t *)(s_part + (size_t)W * L);
    uint32_t *s_bad = s_first + (size_t)W * L;
    int *s_meta = (int *)(s_bad + (size_t)W * L);
    float *tape = p.tape ? p.tape + ((size_t)blockIdx.x * W + w) * 2 * L * kWave
                         : (float *)(sub_lds + subtree_lds_head_words(L, W)) + (size_t)w * 2 * L * kWave;
    float *val = tape, *acc = tape + (size_t)L * kWave;
    uint32_t *my_first = s_first + (size_t)w * L, *my_bad = s_bad + (size_t)w * L;
    const int ntiles = (p.D + kWave - 1) / kWave;
    const float nan = __builtin_nanf("");

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        const size_t row = (size_t)t * L;
        // ---- wave 0: classify, decode, operand table ----
        if (w == 0) {
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > L ? L : len);
            const int cls = uni(classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, kMaxStack));
            if (cls == TREE_OK) build_operand_table<false>(p.type, p.value, row, len, p.var_len, 1, s_op, s_kid, s_pay, s_stk);
            if (lane == 0) { s_meta[0] = cls; s_meta[1] = len; }
        }
        __syncthreads();
        const int cls = uni(s_meta[0]);
        const int len = uni(s_meta[1]);
        if (cls != TREE_OK) {  // malformed: NaN rows
            for (int i = threadIdx.x; i < L; i += blockDim.x) { p.node_err[row + i] = nan; p.node_const[row + i] = nan; }
            __syncthreads();
            continue;
        }
        for (int i = 0; i < len; ++i) acc[i * kWave + lane] = 0.0f;
        for (int i = lane; i < len; i += kWave) my_bad[i] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();

        for (int tile = w; tile < ntiles; tile += W) {
            const int d = tile * kWave + lane;
            const bool valid = d < p.D;
            const int dc = valid ? d : p.D - 1;
            const float *xr = p.X + (size_t)dc * p.var_len;
            const float yv = p.y[dc];
            const bool first_tile = tile == w;
            // ---- forward: execution order, every subtree's value on the tape, its error into the accumulator ----
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
                const float e = grad_err(yv - v, p.use_mse);
                acc[i * kWave + lane] += valid ? e : 0.0f;
                const uint32_t vb = f2bits(v);
                uint32_t ref;
                if (first_tile) {
                    ref = uni(vb);
                    if (lane == 0) my_first[i] = ref;
                } else {
                    ref = uni(my_first[i]);
                }
                if (vb != ref) my_bad[i] = 1u;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }

        // ---- reduce: lanes by the fixed butterfly, waves in wave order ----
        for (int i = 0; i < len; ++i) {
            const float s = wave_sum(acc[i * kWave + lane]);
            if (lane == 0) s_part[(size_t)w * L + i] = s;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < L; i += blockDim.x) {
            float e = nan, c = nan;
            if (i < len) {
                float s = 0.0f;
                for (int k = 0; k < W; ++k) s += s_part[(size_t)k * L + i];
                e = s / (float)p.D;
                const uint32_t f0 = s_first[i];
                bool same = true;
                for (int k = 0; k < W; ++k) same = same && s_bad[(size_t)k * L + i] == 0u && s_first[(size_t)k * L + i] == f0;
                const float fv = bits2f(f0);
                if (same && fv == fv) c = fv;
            }
            p.node_err[row + i] = e;
            p.node_const[row + i] = c;
        }
        __syncthreads();  // the tables are rebuilt for the next tree
    }
}

// ---- the rewrite -----------------------------------------------------------------------------------------------------------------
struct PruneParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *node_err;
    const float *node_const;
    float *out_value;
    int16_t *out_type;
    int16_t *out_size;
    int *root_pos;
    float *loss;
    int pop, gp_len, hoist, fold;
};

// inclusive running maximum over the 64 lanes (values >= 0)
__device__ inline int wave_scan_max_incl(int v) {
    v = max(v, dpp_move<kDppRowShr | 1, 0xf>(0, v));
    v = max(v, dpp_move<kDppRowShr | 2, 0xf>(0, v));
    v = max(v, dpp_move<kDppRowShr | 4, 0xf>(0, v));
    v = max(v, dpp_move<kDppRowShr | 8, 0xf>(0, v));
    v = max(v, dpp_move<kDppBcast15, 0xa>(0, v));
    v = max(v, dpp_move<kDppBcast31, 0xc>(0, v));
    return v;
}

// subtree size of node j as the row states it, kept inside the live prefix (a well-formed tree's sizes already are)
__device__ inline int node_span(const int16_t *size, size_t row, int j, int len) {
    const int s = (int)size[row + j];
    return s < 1 ? 1 : (s > len - j ? len - j : s);
}

constexpr int kPruneWaves = 4;

__global__ __launch_bounds__(kPruneWaves * 64) void prune_rows_kernel(PruneParams q) {
    __shared__ uint16_t s_cnt_all[kPruneWaves][kMaxStack + 2];  // kept nodes in front of node r + k of the chosen subtree
    const int lane = threadIdx.x & 63;
    const int wv = uni((int)(threadIdx.x >> 6));
    const int t = uni((int)(blockIdx.x * kPruneWaves) + wv);
    if (t >= q.pop) return;
    uint16_t *s_cnt = s_cnt_all[wv];
    const int L = q.gp_len;
    const size_t row = (size_t)t * L;
    int len = uni((int)q.size[row]);
    len = len < 0 ? 0 : (len > L ? L : len);
    const int cls = uni(classify_tree(q.type + row, q.value + row, len, false, 1, 1, kMaxStack));
    if (cls != TREE_OK) {  // malformed: the row as it is
        for (int i = lane; i < L; i += kWave) {
            q.out_value[row + i] = q.value[row + i];
            q.out_type[row + i] = q.type[row + i];
            q.out_size[row + i] = q.size[row + i];
        }
        if (lane == 0) { q.root_pos[t] = 0; q.loss[t] = __builtin_nanf(""); }
        return;
    }
    // ---- hoist: the node of least finite error, then least size, then least index ----
    int r0 = 0;
    if (q.hoist) {
        float be = 0.0f;
        int bs = 0, bi = 0x7FFFFFFF;  // (no candidate yet)
        auto better = [](float e, int s, int i, float be, int bs, int bi) {
            if (i == 0x7FFFFFFF) return false;
            if (bi == 0x7FFFFFFF) return true;
            return e < be || (e == be && (s < bs || (s == bs && i < bi)));
        };
        for (int i = lane; i < len; i += kWave) {
            const float e = q.node_err[row + i];
            if (!finite_f(e)) continue;
            const int s = node_span(q.size, row, i, len);
            if (better(e, s, i, be, bs, bi)) { be = e; bs = s; bi = i; }
        }
        for (int off = 1; off < kWave; off <<= 1) {
            const float oe = __shfl_xor(be, off);
            const int os = __shfl_xor(bs, off), oi = __shfl_xor(bi, off);
            if (better(oe, os, oi, be, bs, bi)) { be = oe; bs = os; bi = oi; }
        }
        bi = uni(bi);
        r0 = bi == 0x7FFFFFFF ? 0 : bi;
    }
    const int r1 = r0 + node_span(q.size, row, r0, len);

    auto fold_end = [&](int j) {  // end of the span node j folds away (0: it does not fold)
        if (!q.fold) return 0;
        const int ty = (int)q.type[row + j];
        if (ty == T_VAR || ty == T_CONST || !finite_f(q.node_const[row + j])) return 0;
        return j + node_span(q.size, row, j, len);
    };

    // ---- pass 1: which nodes of [r0, r1) stay (not inside a folding node), and how many stay in front of each ----
    int cover = 0, cnt = 0;
    for (int base = r0; base < r1; base += kWave) {
        const int j = base + lane;
        const bool in = j < r1;
        const int end = in ? fold_end(j) : 0;
        int before = __shfl_up(end, 1);
        if (lane == 0) before = 0;
        const int m = max(cover, wave_scan_max_incl(before));  // the furthest end of a folding node in front of j
        const int keep = in && m <= j ? 1 : 0;
        cover = max(cover, wave_max(end));
        const int incl = wave_scan_incl(keep);
        if (in) s_cnt[j - r0] = (uint16_t)(cnt + incl - keep);
        cnt += __builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) s_cnt[r1 - r0] = (uint16_t)cnt;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- pass 2: the kept nodes in order from position 0, a folding node as one CONST ----
    for (int base = r0; base < r1; base += kWave) {
        const int j = base + lane;
        if (j >= r1) continue;
        const int at = (int)s_cnt[j - r0];
        if ((int)s_cnt[j - r0 + 1] == at) continue;  // dropped
        if (fold_end(j) != 0) {
            q.out_value[row + at] = q.node_const[row + j];
            q.out_type[row + at] = (int16_t)T_CONST;
            q.out_size[row + at] = 1;
        } else {
            const int e = min(j + node_span(q.size, row, j, len), r1);
            q.out_value[row + at] = q.value[row + j];
            q.out_type[row + at] = q.type[row + j];
            q.out_size[row + at] = (int16_t)((int)s_cnt[e - r0] - at);
        }
    }
    for (int i = cnt + lane; i < L; i += kWave) {
        q.out_value[row + i] = 0.0f;
        q.out_type[row + i] = 0;
        q.out_size[row + i] = 0;
    }
    if (lane == 0) { q.root_pos[t] = r0; q.loss[t] = q.node_err[row + r0]; }
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_subtree_errors(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                           int use_mse, const float *value, const int16_t *type, const int16_t *size,
                                           const float *variables, const float *labels, float *node_err, float *node_const,
                                           evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len != 1 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !labels || !node_err || !node_const) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    SubtreeParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.node_err = node_err; p.node_const = node_const;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.use_mse = use_mse ? 1 : 0;
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, subtree_lds_head_words, &plan)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if (const hipError_t e = grant_tape_lds(grant, {(const void *)sr_subtree_kernel})) return (int)e;
    hipLaunchKernelGGL(sr_subtree_kernel, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_prune_rows(unsigned pop_size, unsigned gp_len, unsigned out_len, int hoist, int fold, const float *value,
                                    const int16_t *type, const int16_t *size, const float *node_err, const float *node_const,
                                    float *out_value, int16_t *out_type, int16_t *out_size, int *root_pos, float *loss,
                                    evogp_stream_t stream_) {
    if (pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || out_len != 1 || pop_size > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!value || !type || !size || !node_err || !node_const || !out_value || !out_type || !out_size || !root_pos || !loss)
        return EVOGP_E_NULLPTR;
    if (out_value == value || out_type == type || out_size == size) return EVOGP_E_BADARG;  // not in place
    PruneParams q{};
    q.value = value; q.type = type; q.size = size; q.node_err = node_err; q.node_const = node_const;
    q.out_value = out_value; q.out_type = out_type; q.out_size = out_size; q.root_pos = root_pos; q.loss = loss;
    q.pop = (int)pop_size; q.gp_len = (int)gp_len; q.hoist = hoist ? 1 : 0; q.fold = fold ? 1 : 0;
    const unsigned blocks = (pop_size + kPruneWaves - 1) / kPruneWaves;
    hipLaunchKernelGGL(prune_rows_kernel, dim3(blocks), dim3(kPruneWaves * 64), 0, (hipStream_t)stream_, q);
    return (int)hipGetLastError();
}
