// sr_introns.hip — exact semantic intron removal for single-output trees: a node whose subtree takes, on every data row, the value of
// one of its own descendants is replaced by that descendant (x + 0, 1 * x, max(x, x), neg(neg(x)), IF(c, a, a), ...; gfx950; no
// counterpart in the reference).  include/evogp_hip.h has the contracts, DESIGN 3.28 the reasoning, tests/intron_ref.py the restatement.
//
//   E(a, b)       two float32 values are EQUAL when they have one bit pattern or are both NaN (+0 and -0 are not: 1/x tells them apart)
//   span(i)       size[t][i] kept inside [1, n - i], n the live length (prune_rows_kernel's reading of a row)
//   cand(i)       sig[t][i] != 0: the j in (i, i + span(i)) with sig[t][j] == sig[t][i] of smallest (span(j), j); none, or sig 0: i
//   rep[t][i]     cand(i) when cand(i) != i and E(v_i(X[d]), v_cand(i)(X[d])) on EVERY row d < D; else i.  i on tails and malformed rows
//
// SIGNATURES PROPOSE, THE TAPE VERIFIES: whatever `sig` holds, rep names only descendants that are equal on every row, and every
// function of the interpreter decides by comparison or propagates NaN, so E-equal operands give E-equal results all the way up.
//
// sr_intron_kernel has sr_subtree_sig_kernel's decomposition (sr_subtree_sig.hip): one workgroup owns a tree, wave 0 classifies it and
// builds the operand table while every thread stages the tree's signature row and clamped spans in LDS; then the threads share the candidate scan (a
// thread per node i over its span: sum of spans compares, at most L^2 / 2), the W waves split the 64-row tiles and walk the tree in
// execution order with the value of every subtree on a TAPE [node][lane], one 32-bit word per node and lane.  A node with a candidate
// compares its fresh value with the candidate's tape word (a descendant: already written) and, on a mismatch, stores 1 into the wave's
// BAD[node] word -- the divergent store of a constant sr_subtree_kernel's constancy test uses.  Lanes past D repeat row D - 1 and so
// cannot raise a mismatch.  After the last tile one thread per node ORs the waves' words.  A tree with no candidate at all writes the
// identity and walks nothing.  No atomics, no float reductions, nothing synchronises with the host.
//
// intron_rewrite_kernel: one wave per tree on prune_rows_kernel's skeleton.  R(i) emits node rep[i] and then R(c) for each child c of
// rep[i]; a lane decides node k by walking from the root (cur = 0: r = rep[cur]; k outside r's span: dropped; k == r: kept; else cur =
// the child of r whose span holds k), so a dropped node's own rep deletes nothing.  Prefix counts of the kept flags place the nodes.
#include "sem_key.hpp"
#include "sr_forward.hpp"

namespace evogp {

struct IntronParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;                   // [D][var_len]
    const unsigned long long *sig;    // [pop][gp_len]
    int16_t *rep;                     // [pop][gp_len]
    float *tape;                      // global tapes (rows longer than kTapeLdsLen): [blocks * W][gp_len][64]; nullptr: they are in LDS
    int pop, D, gp_len, var_len;
};

// Dynamic LDS of one workgroup (16-byte aligned carve): op[L] kids[L] pay[L] stack[L] (u32), bad[W][L] (u32), cls / - / any (3 words,
// padded to 4); the candidate of node i rides in bits 16..25 of op[i] (the walk reads that word anyway).  Behind them the staged
// signature row (u64[L]) and the spans (u16[L]) -- which lie IN the tapes when they are in LDS (the scan is over before the first tile
// writes them: W x L x 64 floats >= 2.5 L words), and are part of the head when they are not.
__host__ __device__ inline size_t intron_lds_base_words(int L, int W) { return (((size_t)4 * L + (size_t)W * L + 4) + 3) & ~(size_t)3; }
__host__ __device__ inline size_t intron_lds_head_words(int L, int W) {
    return intron_lds_base_words(L, W) + (L > kTapeLdsLen ? (((size_t)2 * L + ((size_t)L + 1) / 2 + 3) & ~(size_t)3) : 0);
}

// subtree size of node j as the row states it, kept inside the live prefix (sr_subtree.hip node_span)
__device__ inline int intron_span(const int16_t *size, size_t row, int j, int len) {
    const int s = (int)size[row + j];
    return s < 1 ? 1 : (s > len - j ? len - j : s);
}

constexpr int kCandShift = 16;   // operand-table word: handler 0..7, CONST flags 8..10, the candidate 16..25

__global__ __launch_bounds__(kTapeMaxWaves * 64) void sr_intron_kernel(IntronParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t intron_lds[];
    const int L = p.gp_len;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    uint32_t *s_op = intron_lds, *s_kid = s_op + L, *s_pay = s_kid + L;
    int *s_stk = (int *)(s_pay + L);
    uint32_t *s_bad = (uint32_t *)(s_stk + L);
    int *s_meta = (int *)(s_bad + (size_t)W * L);
    unsigned long long *s_sig = (unsigned long long *)(intron_lds + intron_lds_base_words(L, W));
    uint16_t *s_span = (uint16_t *)(s_sig + L);
    float *val = p.tape ? p.tape + ((size_t)blockIdx.x * W + w) * L * kWave
                        : (float *)(intron_lds + intron_lds_head_words(L, W)) + (size_t)w * L * kWave;
    uint32_t *my_bad = s_bad + (size_t)w * L;
    const int ntiles = (p.D + kWave - 1) / kWave;

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        const size_t row = (size_t)t * L;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > L ? L : len);
        // ---- every thread: the signature row and the spans into LDS; wave 0: classify, decode, operand table ----
        for (int i = threadIdx.x; i < len; i += blockDim.x) {
            s_sig[i] = p.sig[row + i];
            s_span[i] = (uint16_t)intron_span(p.size, row, i, len);
        }
        if (w == 0) {
            const int cls = uni(classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, kMaxStack));
            if (cls == TREE_OK) build_operand_table<false>(p.type, p.value, row, len, p.var_len, 1, s_op, s_kid, s_pay, s_stk);
            if (lane == 0) { s_meta[0] = cls; s_meta[2] = 0; }
        }
        __syncthreads();
        const int cls = uni(s_meta[0]);
        if (cls != TREE_OK) {  // malformed: the identity
            for (int i = threadIdx.x; i < L; i += blockDim.x) p.rep[row + i] = (int16_t)i;
            __syncthreads();
            continue;
        }
        // ---- candidates: a thread per node over its span ----
        for (int i = threadIdx.x; i < len; i += blockDim.x) {
            const unsigned long long s = s_sig[i];
            int best = i;
            if (s != 0ull) {
                const int end = i + (int)s_span[i];
                int best_span = 0x7FFFFFFF;
                for (int j = i + 1; j < end; ++j) {
                    if (s_sig[j] != s) continue;
                    const int sj = (int)s_span[j];
                    if (sj < best_span) { best_span = sj; best = j; }   // (j ascends: the first of a size wins)
                }
            }
            s_op[i] |= (uint32_t)best << kCandShift;   // (wave 0 finished the table before the barrier)
            if (best != i) s_meta[2] = 1;
            for (int k = 0; k < W; ++k) s_bad[(size_t)k * L + i] = 0u;
        }
        __syncthreads();
        if (uni(s_meta[2]) == 0) {  // nothing to verify: the identity, no walk
            for (int i = threadIdx.x; i < L; i += blockDim.x) p.rep[row + i] = (int16_t)i;
            __syncthreads();
            continue;
        }

        for (int tile = w; tile < ntiles; tile += W) {
            const long long d = (long long)tile * kWave + lane;   // (64 bits: D may lie within a tile of INT_MAX)
            const int dc = d < p.D ? (int)d : p.D - 1;
            const float *xr = p.X + (size_t)dc * p.var_len;
            // ---- forward: execution order, every subtree's value on the tape, compared with its candidate's ----
            for (int i = len - 1; i >= 0; --i) {
                const uint32_t opw = (uint32_t)uni((int)s_op[i]);
                const uint32_t op = opw & kOpMask;
                const int cd = (int)(opw >> kCandShift);
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
                if (cd != i) {   // (cd > i: written earlier in this walk)
                    const float o = val[cd * kWave + lane];
                    if (f2bits(v) != f2bits(o) && !(v != v && o != o)) my_bad[i] = 1u;
                }
                val[i * kWave + lane] = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();

        // ---- verdict: the waves' words, one thread per node ----
        for (int i = threadIdx.x; i < L; i += blockDim.x) {
            int r = i;
            if (i < len) {
                uint32_t bad = 0u;
                for (int k = 0; k < W; ++k) bad |= s_bad[(size_t)k * L + i];
                if (bad == 0u) r = (int)(s_op[i] >> kCandShift);
            }
            p.rep[row + i] = (int16_t)r;
        }
        __syncthreads();  // the tables are rebuilt for the next tree
    }
}

// ---- the rewrite -----------------------------------------------------------------------------------------------------------------
struct IntronRewriteParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const int16_t *rep;
    float *out_value;
    int16_t *out_type;
    int16_t *out_size;
    int *removed;
    int pop, gp_len;
};

constexpr int kIntronWaves = 4;

__global__ __launch_bounds__(kIntronWaves * 64) void intron_rewrite_kernel(IntronRewriteParams q) {
    __shared__ uint16_t s_cnt_all[kIntronWaves][kMaxStack + 2];   // kept nodes in front of node k
    __shared__ uint16_t s_span_all[kIntronWaves][kMaxStack];      // span(k)
    __shared__ uint16_t s_rep_all[kIntronWaves][kMaxStack];       // rep[k], an entry outside (k, k + span(k)) read as k
    const int lane = threadIdx.x & 63;
    const int wv = uni((int)(threadIdx.x >> 6));
    const int t = uni((int)(blockIdx.x * kIntronWaves) + wv);
    if (t >= q.pop) return;
    uint16_t *s_cnt = s_cnt_all[wv], *s_span = s_span_all[wv], *s_rep = s_rep_all[wv];
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
        if (lane == 0) q.removed[t] = 0;
        return;
    }
    for (int i = lane; i < len; i += kWave) {
        const int s = intron_span(q.size, row, i, len);
        const int r = (int)q.rep[row + i];
        s_span[i] = (uint16_t)s;
        s_rep[i] = (uint16_t)((r > i && r < i + s) ? r : i);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- pass 1: which nodes stay (the walk from the root), and how many stay in front of each ----
    int cnt = 0;
    for (int base = 0; base < len; base += kWave) {
        const int k = base + lane;
        int keep = 0;
        if (k < len) {
            int cur = 0;
            for (;;) {   // cur <= k and k lies in cur's span; cur grows with every round
                const int r = (int)s_rep[cur];
                if (k < r || k >= r + (int)s_span[r]) break;
                if (k == r) { keep = 1; break; }
                int c = r + 1;   // the child of r whose span holds k (c <= k throughout)
                while (k >= c + (int)s_span[c]) c += (int)s_span[c];
                cur = c;
            }
        }
        const int incl = wave_scan_incl(keep);
        if (k < len) s_cnt[k] = (uint16_t)(cnt + incl - keep);
        cnt += __builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) s_cnt[len] = (uint16_t)cnt;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- pass 2: the kept nodes in order from position 0, each with the kept nodes of its span as its size ----
    for (int k = lane; k < len; k += kWave) {
        const int at = (int)s_cnt[k];
        if ((int)s_cnt[k + 1] == at) continue;  // dropped
        q.out_value[row + at] = q.value[row + k];
        q.out_type[row + at] = q.type[row + k];
        q.out_size[row + at] = (int16_t)((int)s_cnt[k + (int)s_span[k]] - at);
    }
    for (int i = cnt + lane; i < L; i += kWave) {
        q.out_value[row + i] = 0.0f;
        q.out_type[row + i] = 0;
        q.out_size[row + i] = 0;
    }
    if (lane == 0) q.removed[t] = len - cnt;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_subtree_introns(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                            const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                            const unsigned long long *sig, int16_t *rep_out, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len != 1 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !sig || !rep_out) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    IntronParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.sig = sig; p.rep = rep_out;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, intron_lds_head_words, &plan, 1)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if (const hipError_t e = grant_tape_lds(grant, {(const void *)sr_intron_kernel})) return (int)e;
    hipLaunchKernelGGL(sr_intron_kernel, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_remove_introns(unsigned pop_size, unsigned gp_len, const float *value, const int16_t *type, const int16_t *size,
                                        const int16_t *rep, float *out_value, int16_t *out_type, int16_t *out_size, int *removed_out,
                                        evogp_stream_t stream_) {
    if (pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || pop_size > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!value || !type || !size || !rep || !out_value || !out_type || !out_size || !removed_out) return EVOGP_E_NULLPTR;
    if (out_value == value || out_type == type || out_size == size) return EVOGP_E_BADARG;  // not in place
    IntronRewriteParams q{};
    q.value = value; q.type = type; q.size = size; q.rep = rep;
    q.out_value = out_value; q.out_type = out_type; q.out_size = out_size; q.removed = removed_out;
    q.pop = (int)pop_size; q.gp_len = (int)gp_len;
    const unsigned blocks = (pop_size + kIntronWaves - 1) / kIntronWaves;
    hipLaunchKernelGGL(intron_rewrite_kernel, dim3(blocks), dim3(kIntronWaves * 64), 0, (hipStream_t)stream_, q);
    return (int)hipGetLastError();
}
