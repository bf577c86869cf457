// sr_subtree_sig.hip — the semantic signature of EVERY SUBTREE of every single-output tree, and the choice of a library of semantically
// distinct subtrees from those signatures (gfx950; no counterpart in the reference).  include/evogp_hip.h has the contracts, DESIGN 3.27
// the reasoning.
//
//   sig[t][i] = sem_finish( sum_{d<D} sem_term(v_i(X[d]), d), D )     v_i = the float32 value of the subtree rooted at node i
//   0 on the tail [len, gp_len) and on every entry of a malformed tree (classify_tree != TREE_OK)
//
// sem_term / sem_finish are sem_key.hpp's, the ones sr_semantic.hip uses for whole trees, and the tape's values are run_general's, so
// sig[t][0] is evogp_hip_sr_semantic_hash's word of tree t and sig[t][i] that of the row holding nodes [i, i + size[t][i]) alone.
//
// sr_subtree_sig_kernel has sr_subtree_kernel's decomposition (sr_subtree.hip): one workgroup owns a tree, wave 0 classifies it and
// builds the operand table, the W waves split the 64-row tiles and walk the tree in execution order with the value of every subtree
// on a TAPE [node][lane].  The epilogue of a node is integer: the lane's term (0 past D) is added over the 64 lanes by a DPP butterfly
// and the total goes into the wave's accumulator [node] (u64, LDS).  There is NO per-lane accumulator tape: a wave keeps one 32-bit
// word per node and lane (16 KiB at gp_len 64, against 48 KiB with a [node][lane] u64 next to the values), which is what decides how
// many waves a CU holds; DESIGN 3.27 has the cost model.  After the last tile one thread per node adds the waves' accumulators and
// finishes the signature.  The sum is modular, so no order matters; there are no atomics and nothing synchronises with the host.
//
// evogp_hip_subtree_library_select: the classes of equal signature among the eligible nodes, the (size, flat index)-smallest member of
// each, and the k classes of largest count.  Two stable sorts (group_sort.hpp) with a few kernels around them:
//   1. pairs   key[f] = sig[f] for an eligible node, 0 for every other word (0 is never eligible), val[f] = f
//   2. sort    by key: the dead words in front, every class a run behind them, flat indices ascending within a run
//   3. runs    run starts (head marks + inclusive maximum scan); the last entry of a run writes its length, every entry offers
//              size << 32 | f to a 64-bit atomic minimum at the run's start (after a plain read that spares most of them)
//   4. order   key2 = (2^32 - 1 - count) << 32 | representative at a run start, ~0 elsewhere; val2 = count; a second sort
//   5. emit    the first min(k, n_classes) entries
// The sorts run over all pop * gp_len words: the number of eligible nodes is known on the device only and the op may not wait for it,
// so the compaction is "to the back of one sort", not a shorter sort.
#include "group_sort.hpp"
#include "sem_key.hpp"
#include "sr_forward.hpp"

namespace evogp {

struct SubtreeSigParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;              // [D][var_len]
    unsigned long long *sig;     // [pop][gp_len]
    float *tape;                 // global tapes (rows longer than kTapeLdsLen): [blocks * W][gp_len][64]; nullptr: they are in LDS
    int pop, D, gp_len, var_len;
};

// Dynamic LDS of one workgroup (16-byte aligned carve): op[L] kids[L] pay[L] stack[L] (u32), acc[W][L] (u64, 8-byte aligned behind
// 4 L words), cls/len (2 words, padded to 4), then, for LDS tapes, W x L x 64 floats.
__host__ __device__ inline size_t subtree_sig_lds_head_words(int L, int W) { return (((size_t)4 * L + (size_t)2 * W * L + 4) + 3) & ~(size_t)3; }

// sum of the 64 lanes mod 2^64 on the DPP path (evogp_defs.hpp wave_sum's sequence on both halves), valid in lane 63
__device__ inline unsigned long long wave_sum_u64_last(unsigned long long v) {
#define EVOGP_SIG_STEP(CTRL, MASK)                                                                            \
    v += ((unsigned long long)(uint32_t)dpp_move<CTRL, MASK>(0, (int)(uint32_t)(v >> 32)) << 32) |            \
         (unsigned long long)(uint32_t)dpp_move<CTRL, MASK>(0, (int)(uint32_t)v)
    EVOGP_SIG_STEP(kDppRowShr | 1, 0xf);
    EVOGP_SIG_STEP(kDppRowShr | 2, 0xf);
    EVOGP_SIG_STEP(kDppRowShr | 4, 0xf);
    EVOGP_SIG_STEP(kDppRowShr | 8, 0xf);
    EVOGP_SIG_STEP(kDppBcast15, 0xa);
    EVOGP_SIG_STEP(kDppBcast31, 0xc);
#undef EVOGP_SIG_STEP
    return v;
}

__global__ __launch_bounds__(kTapeMaxWaves * 64) void sr_subtree_sig_kernel(SubtreeSigParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sig_lds[];
    const int L = p.gp_len;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    uint32_t *s_op = sig_lds, *s_kid = s_op + L, *s_pay = s_kid + L;
    int *s_stk = (int *)(s_pay + L);
    unsigned long long *s_acc = (unsigned long long *)(s_stk + L);
    int *s_meta = (int *)(s_acc + (size_t)W * L);
    float *val = p.tape ? p.tape + ((size_t)blockIdx.x * W + w) * L * kWave
                        : (float *)(sig_lds + subtree_sig_lds_head_words(L, W)) + (size_t)w * L * kWave;
    unsigned long long *my_acc = s_acc + (size_t)w * L;
    const int ntiles = (p.D + kWave - 1) / kWave;

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
        if (cls != TREE_OK) {  // malformed: a row of zeros
            for (int i = threadIdx.x; i < L; i += blockDim.x) p.sig[row + i] = 0ull;
            __syncthreads();
            continue;
        }
        for (int i = lane; i < len; i += kWave) my_acc[i] = 0ull;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();

        for (int tile = w; tile < ntiles; tile += W) {
            const long long d = (long long)tile * kWave + lane;   // (64 bits: D may lie within a tile of INT_MAX)
            const bool valid = d < p.D;
            const int dc = valid ? (int)d : p.D - 1;
            const float *xr = p.X + (size_t)dc * p.var_len;
            // ---- forward: execution order, every subtree's value on the tape, its term into the wave's accumulator ----
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
                const unsigned long long term = sem_term(v, (unsigned long long)(unsigned)dc);
                const unsigned long long tot = wave_sum_u64_last(valid ? term : 0ull);
                if (lane == kWave - 1) my_acc[i] += tot;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();

        // ---- finish: the waves' accumulators, one thread per node ----
        for (int i = threadIdx.x; i < L; i += blockDim.x) {
            unsigned long long s = 0ull;
            if (i < len) {
                for (int k = 0; k < W; ++k) s += s_acc[(size_t)k * L + i];
                s = sem_finish(s, p.D);
            }
            p.sig[row + i] = s;
        }
        __syncthreads();  // the tables are rebuilt for the next tree
    }
}

// ---- the library's choice ---------------------------------------------------------------------------------------------------------
constexpr unsigned long long kNoRep = ~0ull;

__global__ __launch_bounds__(256) void sublib_pairs_kernel(const unsigned long long *sig, const int16_t *size, unsigned n, int min_size,
                                                           int max_size, unsigned long long *key, unsigned *idx, unsigned long long *rep,
                                                           unsigned *n_classes) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f == 0u) *n_classes = 0u;
    if (f >= n) return;
    const unsigned long long s = sig[f];
    const int sz = (int)size[f];
    key[f] = (s != 0ull && sz >= min_size && sz <= max_size) ? s : 0ull;
    idx[f] = f;
    rep[f] = kNoRep;
}

__global__ __launch_bounds__(256) void sublib_heads_kernel(const unsigned long long *key, unsigned n, unsigned *head_pos) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    head_pos[s] = (s == 0u || key[s] != key[s - 1u]) ? s : 0u;
}

// cnt may be the array the head marks were in: the scan that read them is done, and only a run start's word is ever read again
__global__ __launch_bounds__(256) void sublib_runs_kernel(const unsigned long long *key, const unsigned *members, const unsigned *seg,
                                                          const int16_t *size, unsigned n, unsigned long long *rep, unsigned *cnt) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const unsigned long long k = key[s];
    if (k == 0ull) return;
    const unsigned st = seg[s], f = members[s];
    const unsigned long long mine = ((unsigned long long)(unsigned)(int)size[f] << 32) | f;
    if (mine < __atomic_load_n(&rep[st], __ATOMIC_RELAXED)) atomicMin(&rep[st], mine);   // (rep only falls: a stale read costs an atomic, no more)
    if (s == n - 1u || key[s + 1u] != k) cnt[st] = s - st + 1u;
}

__global__ __launch_bounds__(256) void sublib_order_kernel(const unsigned long long *key, const unsigned *seg, const unsigned long long *rep,
                                                           const unsigned *cnt, unsigned n, unsigned long long *key2, unsigned *val2,
                                                           unsigned *n_classes) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const bool head = key[s] != 0ull && seg[s] == s;
    const unsigned c = head ? cnt[s] : 0u;
    key2[s] = head ? ((unsigned long long)(0xFFFFFFFFu - c) << 32) | (rep[s] & 0xFFFFFFFFull) : kNoRep;   // (c >= 1: never kNoRep)
    val2[s] = c;
    if (head) atomicAdd(n_classes, 1u);
}

__global__ __launch_bounds__(256) void sublib_emit_kernel(const unsigned long long *key2, const unsigned *val2, const unsigned *n_classes,
                                                          unsigned n, int k, int *member, int *count, int *n_out) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    const unsigned nc = *n_classes;
    if (j == 0) *n_out = (int)nc;
    if (j >= k) return;
    const bool live = (unsigned)j < nc && (unsigned)j < n;
    member[j] = live ? (int)(unsigned)(key2[j] & 0xFFFFFFFFull) : -1;
    count[j] = live ? (int)val2[j] : 0;
}

struct SublibWorkspace {
    unsigned long long *keys_a, *keys_b, *rep;
    unsigned *vals_a, *vals_b, *head_pos, *seg, *n_classes;
    void *temp;
    size_t temp_bytes;
};

static hipError_t sublib_workspace(unsigned n, Arena &a, SublibWorkspace *w) {
    hipError_t e;
    w->temp_bytes = 0;
    if ((e = sort_buffers_temp(n, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = scan_max_temp(n, &w->temp_bytes)) != hipSuccess) return e;
    w->keys_a = a.take<unsigned long long>(n); w->keys_b = a.take<unsigned long long>(n); w->rep = a.take<unsigned long long>(n);
    w->vals_a = a.take<unsigned>(n); w->vals_b = a.take<unsigned>(n);
    w->head_pos = a.take<unsigned>(n); w->seg = a.take<unsigned>(n);
    w->n_classes = a.take<unsigned>(1);
    w->temp = a.take_bytes(w->temp_bytes);
    return hipSuccess;
}

static int sublib_badarg(unsigned pop_size, unsigned gp_len) {
    return pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || (unsigned long long)pop_size * gp_len > 0x7FFFFFFFull;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_subtree_signatures(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                               const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                               unsigned long long *sig_out, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len != 1 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !sig_out) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    SubtreeSigParams p{};
    p.value = value; p.type = type; p.size = size; p.X = variables; p.sig = sig_out;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    TapePlan plan;
    if (const int rc = plan_tape_launch(p.pop, p.D, p.gp_len, stream, subtree_sig_lds_head_words, &plan, 1)) return rc;
    p.tape = plan.tape;
    static LdsGrant grant;
    if (const hipError_t e = grant_tape_lds(grant, {(const void *)sr_subtree_sig_kernel})) return (int)e;
    hipLaunchKernelGGL(sr_subtree_sig_kernel, dim3((unsigned)plan.blocks), dim3(plan.W * 64), plan.lds, stream, p);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_subtree_library_select_workspace_bytes(unsigned pop_size, unsigned gp_len, unsigned long long *bytes) {
    if (sublib_badarg(pop_size, gp_len)) return EVOGP_E_BADARG;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    SublibWorkspace w;
    const hipError_t e = sublib_workspace(pop_size * gp_len, a, &w);
    if (e != hipSuccess) return (int)e;
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_subtree_library_select(unsigned pop_size, unsigned gp_len, const unsigned long long *sig, const int16_t *size,
                                                int min_size, int max_size, int k, int *member_out, int *count_out, int *n_classes_out,
                                                void *workspace, evogp_stream_t stream_) {
    if (sublib_badarg(pop_size, gp_len) || min_size < 1 || max_size < min_size || k < 1 || k > EVOGP_BACKPROP_MAX_LIB) return EVOGP_E_BADARG;
    if (!sig || !size || !member_out || !count_out || !n_classes_out || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const unsigned n = pop_size * gp_len;
    Arena a{(char *)workspace};
    SublibWorkspace w;
    hipError_t e = sublib_workspace(n, a, &w);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((n + 255u) / 256u), block(256);
    hipLaunchKernelGGL(sublib_pairs_kernel, grid, block, 0, stream, sig, size, n, min_size, max_size, w.keys_a, w.vals_a, w.rep, w.n_classes);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    bool in_b;
    if ((e = sort_buffers(w.temp, w.temp_bytes, w.keys_a, w.keys_b, w.vals_a, w.vals_b, n, &in_b, stream)) != hipSuccess) return (int)e;
    unsigned long long *key = in_b ? w.keys_b : w.keys_a, *key2 = in_b ? w.keys_a : w.keys_b;   // the other side is free for the second sort
    unsigned *members = in_b ? w.vals_b : w.vals_a, *val2 = in_b ? w.vals_a : w.vals_b;
    hipLaunchKernelGGL(sublib_heads_kernel, grid, block, 0, stream, key, n, w.head_pos);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = scan_max(w.temp, w.temp_bytes, w.head_pos, w.seg, n, stream)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sublib_runs_kernel, grid, block, 0, stream, key, members, w.seg, size, n, w.rep, w.head_pos);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sublib_order_kernel, grid, block, 0, stream, key, w.seg, w.rep, w.head_pos, n, key2, val2, w.n_classes);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    bool in_second;
    if ((e = sort_buffers(w.temp, w.temp_bytes, key2, key, val2, members, n, &in_second, stream)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sublib_emit_kernel, dim3(((unsigned)k + 255u) / 256u), block, 0, stream, in_second ? key : key2, in_second ? members : val2,
                       w.n_classes, n, k, member_out, count_out, n_classes_out);
    return (int)hipGetLastError();
}
