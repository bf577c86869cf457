// sr_structure.hip — structural constraints over SR trees (gfx950; no counterpart in the reference): for every node of the live prefix of
// every single-output tree a weighted complexity, a height, a depth, R nesting counters and a flag byte, and per tree the number of
// violations of the depth limit, the complexity limit, the operand limits and the nesting rules.  The definition -- symbols, both
// passes, the flags -- is the integer restatement tests/structure_ref.py; this file follows it rule by rule and, all arithmetic being
// integer, gives the same words.
//
// ONE LANE PER TREE, BOTH PASSES IN ONE LAUNCH, the walk of sr_interval_rules.hpp and sr_dims.hip.  The pass up goes from the last live
// node to node 0: child 1 of node i is i + 1 (its complexity, height, counters and verified size are still in registers), child 2 is
// i + 1 + size[i + 1] and child 3 follows it: theirs are read back from the lane's own output rows, which are products, not scratch.
// Size words are verified before a parent uses them and the stack discipline is checked on the way, so no child index leaves the live
// prefix; a row that fails is rewritten as MALFORMED.  The pass down runs for a well-formed row: node 0 to the last live node, every
// node writes depth + 1 into its children's slots of the depth row (child 1's stays in a register), where a child finds it when the walk
// arrives (same lane, program order).
//
// R IS A TEMPLATE PARAMETER, one instantiation per R = 0 .. 8, as K is in sr_dims.hip: the counters a step holds (child 1's, the
// node's, those of children 2 and 3 as they are read) are registers only when every index is a constant, R = 0 pays for none, and
// for R = 2, 4, 8 the counters of a node are one 2-, 4- or 8-byte access of the nest row instead of R byte accesses.  The
// compiler's report is in DESIGN.md section 3.19.  The three tables -- cost[32], operand_limit[32][3], the rules -- go into LDS once
// per workgroup (the index is the lane's own symbol, so the scalar path does not apply).  The words past the live prefix are zeroed by
// the workgroup, one row after the other with the lanes along the row.  No dataset, no atomics, no host synchronisation, no workspace;
// inputs are only read.
#include "sr_interval_rules.hpp"

using namespace evogp;

namespace {

constexpr int kSymVar = 29, kSymConst = 30, kSymUnknown = 31;
constexpr int kTableWords = 32 + 96;   // cost, operand_limit; then 3 R words of rules

template <int R> struct Nest { int c[R > 0 ? R : 1]; };

// the R counters of one node are R consecutive bytes of the nest row: one access where R is 2, 4 or 8 (the row is 8-byte aligned)
template <int R> __device__ inline void nest_max(const unsigned char *p, Nest<R> &below) {
    unsigned w[2] = {0u, 0u};
    if (R == 8) { const uint2 q = *reinterpret_cast<const uint2 *>(p); w[0] = q.x; w[1] = q.y; }
    else if (R == 4) w[0] = *reinterpret_cast<const unsigned *>(p);
    else if (R == 2) w[0] = *reinterpret_cast<const unsigned short *>(p);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int b = (R == 8 || R == 4 || R == 2) ? (int)((w[r >> 2] >> (8 * (r & 3))) & 0xFFu) : (int)p[r];
        below.c[r] = b > below.c[r] ? b : below.c[r];
    }
}
template <int R> __device__ inline void nest_store(unsigned char *p, const Nest<R> &v) {
    if (R == 8 || R == 4 || R == 2) {
        unsigned w[2] = {0u, 0u};
#pragma unroll
        for (int r = 0; r < R; ++r) w[r >> 2] |= (unsigned)v.c[r] << (8 * (r & 3));
        if (R == 8) *reinterpret_cast<uint2 *>(p) = make_uint2(w[0], w[1]);
        else if (R == 4) *reinterpret_cast<unsigned *>(p) = w[0];
        else *reinterpret_cast<unsigned short *>(p) = (unsigned short)w[0];
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) p[r] = (unsigned char)v.c[r];
    }
}

// the symbol of a decoded node
__device__ inline int structure_symbol(const Decoded &d) {
    if (d.op == H_CONST) return kSymConst;
    if (d.op == H_VAR) return kSymVar;
    if (d.op == H_IF) return 0;
    const int f = itv_func_of(d.op);
    return f < 0 ? kSymUnknown : f;
}

template <int R>
__global__ __launch_bounds__(kWave) void tree_structure_kernel(const float *__restrict__ value, const int16_t *__restrict__ type,
                                                               const int16_t *__restrict__ size, const int *__restrict__ cost,
                                                               const int *__restrict__ operand_limit, const int *__restrict__ rule_outer,
                                                               const int *__restrict__ rule_inner, const int *__restrict__ rule_limit,
                                                               int max_depth, int max_complexity, unsigned pop, unsigned gp_len,
                                                               int *complexity, int16_t *height, int16_t *depth, unsigned char *nest,
                                                               unsigned char *flags, int *__restrict__ violations) {
    __shared__ int s_table[kTableWords + 3 * (R > 0 ? R : 1)];
    const unsigned lane = threadIdx.x;
    for (unsigned j = lane; j < 32u; j += (unsigned)kWave) s_table[j] = cost[j];
    for (unsigned j = lane; j < 96u; j += (unsigned)kWave) s_table[32 + j] = operand_limit[j];
    if (R > 0 && lane < (unsigned)R) {
        s_table[kTableWords + lane] = rule_outer[lane];
        s_table[kTableWords + R + lane] = rule_inner[lane];
        s_table[kTableWords + 2 * R + lane] = rule_limit[lane];
    }
    __syncthreads();
    const int *s_cost = s_table, *s_oplim = s_table + 32, *s_outer = s_table + kTableWords, *s_inner = s_outer + R, *s_limit = s_inner + R;

    const unsigned t = blockIdx.x * (unsigned)kWave + lane;
    const bool live = t < pop;
    const size_t row = (size_t)(live ? t : 0u) * gp_len;
    int n = 0;
    if (live) {
        n = (int)size[row];
        n = n < 0 ? 0 : (n > (int)gp_len ? (int)gp_len : n);
    }

    // the dead words of the workgroup's rows: one row after the other, the lanes along the row
    const unsigned rows_here = min((unsigned)kWave, pop - blockIdx.x * (unsigned)kWave);
    for (unsigned r = 0; r < rows_here; ++r) {
        const int nr = __builtin_amdgcn_readlane(n, (int)r);
        const size_t at = ((size_t)blockIdx.x * kWave + r) * gp_len;
        const unsigned first = (unsigned)(nr > 0 ? nr : 1);
        for (unsigned j = first + lane; j < gp_len; j += (unsigned)kWave) {
            complexity[at + j] = 0;
            height[at + j] = 0;
            depth[at + j] = 0;
            flags[at + j] = 0;
        }
        if (R > 0)
            for (unsigned j = first * (unsigned)R + lane; j < gp_len * (unsigned)R; j += (unsigned)kWave) nest[at * R + j] = 0;
    }
    if (!live) return;

    // ---- the pass up: last live node to node 0 ----
    bool ok = n > 0;
    int h = 0;               // operand-stack height after the nodes walked so far
    int count = 0;
    int prev_cx = 0, prev_ht = 0, prev_size = 0;   // node i + 1: its complexity, height, (verified) size and counters
    Nest<R> prev;
#pragma unroll
    for (int r = 0; r < R; ++r) prev.c[r] = 0;
    int ty = 0, sz = 0;
    float v = 0.0f;
    if (ok) { ty = type[row + n - 1]; v = value[row + n - 1]; sz = size[row + n - 1]; }
    for (int i = n - 1; i >= 0; --i) {
        const int ty_i = ty, sz_i = sz;
        const float v_i = v;
        if (i > 0) { ty = type[row + i - 1]; v = value[row + i - 1]; sz = size[row + i - 1]; }   // the next node's words
        const Decoded d = decode_node(ty_i, v_i, false, 1, 1);
        const int arity = 1 - d.delta;
        if (h < arity) { ok = false; break; }
        h += d.delta;
        const int s = structure_symbol(d);
        int cx = s_cost[s], ht = 0, span = 1;
        bool operand = false;
        Nest<R> below;
#pragma unroll
        for (int r = 0; r < R; ++r) below.c[r] = 0;
        if (arity >= 1) {
            const int lim1 = s_oplim[3 * s];
            operand = lim1 >= 0 && prev_cx > lim1;
            cx += prev_cx;
            ht = prev_ht;
            span += prev_size;
            below = prev;
        }
        if (arity >= 2) {
            const size_t c2 = row + i + 1 + prev_size;
            const int cx2 = complexity[c2], ht2 = height[c2], size2 = size[c2], lim2 = s_oplim[3 * s + 1];
            operand = operand || (lim2 >= 0 && cx2 > lim2);
            cx += cx2;
            ht = ht2 > ht ? ht2 : ht;
            span += size2;
            nest_max<R>(nest + c2 * R, below);
            if (arity == 3) {
                const size_t c3 = c2 + size2;
                const int cx3 = complexity[c3], ht3 = height[c3], lim3 = s_oplim[3 * s + 2];
                operand = operand || (lim3 >= 0 && cx3 > lim3);
                cx += cx3;
                ht = ht3 > ht ? ht3 : ht;
                span += (int)size[c3];
                nest_max<R>(nest + c3 * R, below);
            }
        }
        if (sz_i != span) { ok = false; break; }
        ht += 1;
        bool nested = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            nested = nested || ((((unsigned)s_outer[r] >> s) & 1u) != 0u && below.c[r] > s_limit[r]);
            const int c = below.c[r] + (int)(((unsigned)s_inner[r] >> s) & 1u);
            prev.c[r] = c > 255 ? 255 : c;
        }
        if (R > 0) nest_store<R>(nest + (row + i) * R, prev);
        complexity[row + i] = cx;
        height[row + i] = (int16_t)ht;
        flags[row + i] = (unsigned char)((nested ? EVOGP_STRUCT_NEST : 0) | (operand ? EVOGP_STRUCT_OPERAND : 0));
        count += (nested || operand) ? 1 : 0;
        prev_cx = cx;
        prev_ht = ht;
        prev_size = span;
    }
    if (!ok || h != 1) {
        const int m = n > 0 ? n : 1;   // (an empty row marks word 0)
        for (int i = 0; i < m; ++i) {
            complexity[row + i] = 0;
            height[row + i] = 0;
            depth[row + i] = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) nest[(row + i) * R + r] = 0;
            flags[row + i] = (unsigned char)EVOGP_STRUCT_MALFORMED;
        }
        violations[t] = -1;
        return;
    }
    // the root (prev_* is node 0 now)
    unsigned root = 0;
    if (max_depth >= 0 && prev_ht > max_depth) root |= EVOGP_STRUCT_DEPTH;
    if (max_complexity >= 0 && prev_cx > max_complexity) root |= EVOGP_STRUCT_COMPLEXITY;
    if (root) {
        flags[row] = (unsigned char)(flags[row] | root);
        count += (root & EVOGP_STRUCT_DEPTH ? 1 : 0) + (root & EVOGP_STRUCT_COMPLEXITY ? 1 : 0);
    }
    violations[t] = count;

    // ---- the pass down: node 0 to the last live node ----
    depth[row] = 0;
    int dp = 0;
    bool in_reg = true;   // dp is node i's depth (node 0, or the first child of node i - 1); otherwise it is read from the row
    ty = type[row];
    int ty_next = 0, sz_next = 0;   // the words of node i + 1, fetched one step ahead
    if (n > 1) { ty_next = type[row + 1]; sz_next = size[row + 1]; }
    for (int i = 0; i < n; ++i) {
        const int ty_i = ty, size1 = sz_next;
        ty = ty_next;
        if (i + 2 < n) { ty_next = type[row + i + 2]; sz_next = size[row + i + 2]; }
        if (!in_reg) dp = depth[row + i];
        const int arity = (ty_i == T_CONST || ty_i == T_VAR) ? 0 : ty_i == T_UFUNC ? 1 : ty_i == T_BFUNC ? 2 : 3;
        in_reg = arity > 0;
        if (arity == 0) continue;
        dp += 1;
        const size_t c1 = row + i + 1;
        depth[c1] = (int16_t)dp;
        if (arity >= 2) {
            const size_t c2 = c1 + size1;
            depth[c2] = (int16_t)dp;
            if (arity == 3) depth[c2 + size[c2]] = (int16_t)dp;
        }
    }
}

template <int R>
int launch_structure(unsigned pop, unsigned gp_len, const float *value, const int16_t *type, const int16_t *size, const int *cost,
                     const int *operand_limit, const int *rule_outer, const int *rule_inner, const int *rule_limit, int max_depth,
                     int max_complexity, int *complexity, int16_t *height, int16_t *depth, unsigned char *nest, unsigned char *flags,
                     int *violations, hipStream_t stream) {
    const dim3 grid((pop + (unsigned)kWave - 1u) / (unsigned)kWave), block(kWave);
    hipLaunchKernelGGL((tree_structure_kernel<R>), grid, block, 0, stream, value, type, size, cost, operand_limit, rule_outer, rule_inner,
                       rule_limit, max_depth, max_complexity, pop, gp_len, complexity, height, depth, nest, flags, violations);
    return (int)hipGetLastError();
}

} // namespace

extern "C" int evogp_hip_tree_structure(unsigned pop, unsigned gp_len, unsigned n_rules, const float *value, const int16_t *type,
                                        const int16_t *size, const int *cost, const int *operand_limit, const int *rule_outer,
                                        const int *rule_inner, const int *rule_limit, int max_depth, int max_complexity, int *complexity,
                                        int16_t *height, int16_t *depth, unsigned char *nest, unsigned char *flags, int *violations,
                                        evogp_stream_t stream_) {
    if (pop == 0 || pop > 0x7FFFFFFFu || gp_len == 0 || gp_len > (unsigned)kMaxStack || n_rules > (unsigned)EVOGP_STRUCT_MAX_RULES ||
        max_depth < -1 || max_complexity < -1)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !cost || !operand_limit || !complexity || !height || !depth || !flags || !violations)
        return EVOGP_E_NULLPTR;
    if (n_rules > 0 && (!rule_outer || !rule_inner || !rule_limit || !nest)) return EVOGP_E_NULLPTR;
    if (n_rules > 0 && ((uintptr_t)nest & 7u) != 0) return EVOGP_E_BADARG;   // (the counters of a node are read and written as one word)
    hipStream_t stream = (hipStream_t)stream_;
#define EVOGP_STRUCT_CASE(R_) \
    case R_: return launch_structure<R_>(pop, gp_len, value, type, size, cost, operand_limit, rule_outer, rule_inner, rule_limit, max_depth, \
                                         max_complexity, complexity, height, depth, nest, flags, violations, stream)
    switch (n_rules) {
        EVOGP_STRUCT_CASE(0);
        EVOGP_STRUCT_CASE(1);
        EVOGP_STRUCT_CASE(2);
        EVOGP_STRUCT_CASE(3);
        EVOGP_STRUCT_CASE(4);
        EVOGP_STRUCT_CASE(5);
        EVOGP_STRUCT_CASE(6);
        EVOGP_STRUCT_CASE(7);
        default: EVOGP_STRUCT_CASE(8);
    }
#undef EVOGP_STRUCT_CASE
}
