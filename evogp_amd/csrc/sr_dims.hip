// sr_dims.hip — dimensional analysis over SR trees (gfx950; no counterpart in the reference): for every node of the live prefix of every
// single-output tree a physical unit (K int32 numerators over the denominator EVOGP_DIM_DEN) and a flag byte, and per tree the number of
// nodes at which no unit of the free constants can make the operation consistent.  The definition -- every rule of both passes, the
// claim and its pow gap -- is the integer restatement tests/dimension_ref.py; this file follows it rule by rule and, all arithmetic
// being integer (the one float64 product of pow is exact), gives the same words.
//
// ONE LANE PER TREE, BOTH PASSES IN ONE LAUNCH, the walk of sr_interval_rules.hpp.  Pass 1 goes from the last live node to node 0 and
// gives every node (free?, unit): child 1 of node i is i + 1 (its unit, free mark and verified size are still in registers), child 2
// is i + 1 + size[i + 1] and child 3 follows it: their units are read back from the lane's own units row, which is the product, not
// scratch.  Size words are verified before a parent uses them and the stack discipline is checked on the way, so no child index leaves
// the live prefix; a row that fails is rewritten as MALFORMED.  Pass 2 runs only for a tree without a violation that holds a free node:
// node 0 to the last live node, every node hands its FREE children the unit they must take by writing it into the child's slot of the
// row, where the child finds it when the walk arrives (same lane, program order).
//
// K IS A TEMPLATE PARAMETER, one instantiation per K = 1 .. 8, not a runtime bound over arrays of 8: the four units a step holds (child
// 1, the node, children 2 and 3) are 4 K registers that the compiler can only keep in VGPRs when every index is a constant, a unit is
// one contiguous 4 K-byte access that it merges into dwordx2 / x3 / x4, and K = 1 .. 3 -- what physical problems use -- pay for K
// words, not for 8 predicated ones.  The compiler reports 33 VGPRs for K = 1, 43 for K = 3 and 63 for K = 8 -- the full 8 waves per SIMD
// by registers for every K -- and no scratch.
// var_units is staged in LDS by the wave when it fits kDimLdsWords (16 KiB), and read through the vector cache otherwise (the index is
// the lane's own, so the scalar path does not apply).  The words past the live prefix are zeroed by the workgroup, one row after the
// other with the lanes along the row.  No dataset, no atomics, no host synchronisation, no workspace; inputs are only read.
#include "sr_interval_rules.hpp"

using namespace evogp;

namespace {

constexpr int kDimLim = EVOGP_DIM_MAX_NUM;
constexpr unsigned kDimLdsWords = 4096;

template <int K> struct Unit { int n[K]; };

template <int K> __device__ inline Unit<K> unit_zero() {
    Unit<K> r;
#pragma unroll
    for (int k = 0; k < K; ++k) r.n[k] = 0;
    return r;
}
template <int K> __device__ inline Unit<K> unit_load(const int *p) {
    Unit<K> r;
#pragma unroll
    for (int k = 0; k < K; ++k) r.n[k] = p[k];
    return r;
}
template <int K> __device__ inline void unit_store(int *p, const Unit<K> &u) {
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = u.n[k];
}
template <int K> __device__ inline bool unit_differ(const Unit<K> &a, const Unit<K> &b) {
    int d = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) d |= a.n[k] ^ b.n[k];
    return d != 0;
}
template <int K> __device__ inline bool unit_nonzero(const Unit<K> &a) {
    int d = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) d |= a.n[k];
    return d != 0;
}
// sa * a + sb * b; false when a numerator leaves the range
template <int K> __device__ inline bool unit_combine(int sa, const Unit<K> &a, int sb, const Unit<K> &b, Unit<K> &r) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        r.n[k] = sa * a.n[k] + sb * b.n[k];
        ok = ok && r.n[k] <= kDimLim && r.n[k] >= -kDimLim;
    }
    return ok;
}

struct DimNode {
    bool free, viol;
};

// + - max min, the branches of IF, the operands of a comparison: (free?, unit, violation) of the pair
template <int K> __device__ inline DimNode dim_addlike(bool a_free, const Unit<K> &a, bool b_free, const Unit<K> &b, Unit<K> &r) {
#pragma unroll
    for (int k = 0; k < K; ++k) r.n[k] = a_free ? b.n[k] : a.n[k];   // (a free node's unit is 0 in pass 1)
    DimNode d;
    d.free = a_free && b_free;
    d.viol = !a_free && !b_free && unit_differ<K>(a, b);
    return d;
}

template <int K> __device__ inline DimNode dim_unary(int f, bool a_free, const Unit<K> &a, Unit<K> &r) {
    DimNode d;
    d.free = false;
    d.viol = false;
    r = unit_zero<K>();
    if (f < 0) return d;
    switch (f) {
    case F_NEG:
    case F_ABS: r = a; d.free = a_free; return d;
    case F_INV:
    case F_LOOSE_INV:
#pragma unroll
        for (int k = 0; k < K; ++k) r.n[k] = -a.n[k];
        d.free = a_free;
        return d;
    case F_SQRT:
    case F_LOOSE_SQRT: {
        d.free = a_free;
        int odd = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) { odd |= a.n[k] & 1; r.n[k] = a.n[k] >> 1; }
        if (odd) { d.viol = true; r = unit_zero<K>(); }
        return d;
    }
    default:   // sin .. exp
        d.viol = !a_free && unit_nonzero<K>(a);
        return d;
    }
}

// b_const: child 2 is a CONST leaf, c its value
template <int K> __device__ inline DimNode dim_binary(int f, bool a_free, const Unit<K> &a, bool b_free, const Unit<K> &b, bool b_const, float c,
                                                      Unit<K> &r) {
    DimNode d;
    d.free = false;
    d.viol = false;
    r = unit_zero<K>();
    if (f < 0) return d;
    switch (f) {
    case F_ADD:
    case F_SUB:
    case F_MAX:
    case F_MIN: return dim_addlike<K>(a_free, a, b_free, b, r);
    case F_MUL:
    case F_DIV:
    case F_LOOSE_DIV:
        d.free = a_free || b_free;
        if (!d.free && !unit_combine<K>(1, a, f == F_MUL ? 1 : -1, b, r)) { d.viol = true; r = unit_zero<K>(); }
        return d;
    case F_POW:
    case F_LOOSE_POW: {
        const bool based = !a_free && unit_nonzero<K>(a);
        d.viol = (!b_free && unit_nonzero<K>(b)) || (based && !b_const);
        if (!d.viol && based) {
            bool ok = true;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double p = (double)c * (double)a.n[k];   // exact: 24 x 25 bits
                const bool in = p == rint(p) && fabs(p) <= (double)kDimLim;   // (false for a NaN or infinite c)
                r.n[k] = in ? (int)p : 0;
                ok = ok && in;
            }
            if (!ok) { d.viol = true; r = unit_zero<K>(); }
        }
        return d;
    }
    default: {   // F_LT .. F_GE
        Unit<K> unused;
        d.viol = dim_addlike<K>(a_free, a, b_free, b, unused).viol;
        return d;
    }
    }
}

// pass 2: the free child at word c must take the unit `want`; one out of range becomes 0 and a violation of that child
template <int K> __device__ inline int dim_demand(int *units, unsigned char *flags, size_t c, bool in_range, Unit<K> want) {
    if (!in_range) {
        want = unit_zero<K>();
        flags[c] = (unsigned char)(flags[c] | EVOGP_DIM_VIOLATION);
    }
    unit_store<K>(units + c * K, want);
    return in_range ? 0 : 1;
}

template <int K, bool LDS>
__global__ __launch_bounds__(kWave) void tree_dimensions_kernel(const float *__restrict__ value, const int16_t *__restrict__ type,
                                                                 const int16_t *__restrict__ size, const int *__restrict__ var_units,
                                                                 const int *__restrict__ label_units, int check_root, unsigned pop,
                                                                 unsigned gp_len, unsigned var_len, int *units, unsigned char *flags,
                                                                 int *__restrict__ violations) {
    extern __shared__ int s_var_units[];
    const unsigned lane = threadIdx.x;
    if (LDS) {
        for (unsigned j = lane; j < var_len * (unsigned)K; j += (unsigned)kWave) s_var_units[j] = var_units[j];
        __syncthreads();
    }
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
        for (unsigned j = first + lane; j < gp_len; j += (unsigned)kWave) flags[at + j] = 0;
        for (unsigned j = first * (unsigned)K + lane; j < gp_len * (unsigned)K; j += (unsigned)kWave) units[at * K + j] = 0;
    }
    if (!live) return;

    // ---- pass 1: last live node to node 0 ----
    bool ok = n > 0;
    int h = 0;               // operand-stack height after the nodes walked so far
    int count = 0;
    bool any_free = false;
    Unit<K> prev = unit_zero<K>();   // node i + 1: its unit, is it free, its (verified) size
    bool prev_free = false;
    int prev_size = 0;
    int ty = 0, sz = 0;
    float v = 0.0f;
    if (ok) { ty = type[row + n - 1]; v = value[row + n - 1]; sz = size[row + n - 1]; }
    for (int i = n - 1; i >= 0; --i) {
        const int ty_i = ty, sz_i = sz;
        const float v_i = v;
        if (i > 0) { ty = type[row + i - 1]; v = value[row + i - 1]; sz = size[row + i - 1]; }   // the next node's words
        const Decoded d = decode_node(ty_i, v_i, false, (int)var_len, 1);
        const int arity = 1 - d.delta;
        if (h < arity) { ok = false; break; }
        h += d.delta;
        Unit<K> r = unit_zero<K>();
        DimNode res;
        res.free = false;
        res.viol = false;
        int span = 1;
        if (d.op == H_CONST) {
            res.free = true;
        } else if (d.op == H_VAR) {
            r = LDS ? unit_load<K>(s_var_units + d.pay * K) : unit_load<K>(var_units + (size_t)d.pay * K);
        } else if (arity == 1) {
            span = 1 + prev_size;
            res = dim_unary<K>(itv_func_of(d.op), prev_free, prev, r);
        } else {
            const size_t c2 = row + i + 1 + prev_size;
            const Unit<K> b = unit_load<K>(units + c2 * K);
            const bool b_free = (flags[c2] & EVOGP_DIM_FREE) != 0;
            const int size2 = size[c2];
            if (arity == 2) {
                span = 1 + prev_size + size2;
                res = dim_binary<K>(itv_func_of(d.op), prev_free, prev, b_free, b, type[c2] == T_CONST, value[c2], r);
            } else {
                const size_t c3 = c2 + size2;
                const Unit<K> c = unit_load<K>(units + c3 * K);
                const bool c_free = (flags[c3] & EVOGP_DIM_FREE) != 0;
                span = 1 + prev_size + size2 + (int)size[c3];
                res = dim_addlike<K>(b_free, b, c_free, c, r);   // (the condition is compared with 0: any unit)
            }
        }
        if (sz_i != span) { ok = false; break; }
        unit_store<K>(units + (row + i) * K, r);
        flags[row + i] = (unsigned char)((res.free ? EVOGP_DIM_FREE : 0) | (res.viol ? EVOGP_DIM_VIOLATION : 0));
        count += res.viol ? 1 : 0;
        any_free = any_free || res.free;
        prev = r;
        prev_free = res.free;
        prev_size = span;
    }
    if (!ok || h != 1) {
        const int m = n > 0 ? n : 1;   // (an empty row marks word 0)
        for (int i = 0; i < m; ++i) {
            unit_store<K>(units + (row + i) * K, unit_zero<K>());
            flags[row + i] = (unsigned char)EVOGP_DIM_MALFORMED;
        }
        violations[t] = -1;
        return;
    }
    // the root (prev is node 0 now)
    Unit<K> label = unit_zero<K>();
    if (check_root) label = unit_load<K>(label_units);
    if (check_root && !prev_free && unit_differ<K>(prev, label)) {
        flags[row] = (unsigned char)(flags[row] | EVOGP_DIM_ROOT_MISMATCH);
        ++count;
    }

    // ---- pass 2: node 0 to the last live node, for a consistent tree that holds a free node ----
    if (count == 0 && any_free) {
        if (prev_free) unit_store<K>(units + row * K, label);
        for (int i = 0; i < n; ++i) {
            const Decoded d = decode_node(type[row + i], value[row + i], false, (int)var_len, 1);
            const int arity = 1 - d.delta;
            if (arity == 0) continue;
            const size_t c1 = row + i + 1;
            const bool f1 = (flags[c1] & EVOGP_DIM_FREE) != 0;
            const int *final_unit = units + (row + i) * K;   // D, read only by a node that has a free child
            const Unit<K> zero = unit_zero<K>();
            Unit<K> w;
            if (arity == 1) {
                if (!f1) continue;
                const Unit<K> D = unit_load<K>(final_unit);
                const int f = itv_func_of(d.op);
                const int s = (f == F_NEG || f == F_ABS) ? 1 : (f == F_INV || f == F_LOOSE_INV) ? -1 : (f == F_SQRT || f == F_LOOSE_SQRT) ? 2 : 0;
                const bool in = unit_combine<K>(s, D, 0, zero, w);
                count += dim_demand<K>(units, flags, c1, in, w);
                continue;
            }
            const size_t c2 = c1 + size[c1];
            const bool f2 = (flags[c2] & EVOGP_DIM_FREE) != 0;
            if (arity == 3) {
                const size_t c3 = c2 + size[c2];
                const bool f3 = (flags[c3] & EVOGP_DIM_FREE) != 0;
                if (f1) count += dim_demand<K>(units, flags, c1, true, zero);
                if (f2 || f3) {
                    const Unit<K> D = unit_load<K>(final_unit);
                    if (f2) count += dim_demand<K>(units, flags, c2, true, D);
                    if (f3) count += dim_demand<K>(units, flags, c3, true, D);
                }
                continue;
            }
            if (!f1 && !f2) continue;
            const Unit<K> D = unit_load<K>(final_unit);
            const int f = itv_func_of(d.op);
            const Unit<K> u1 = f1 ? zero : unit_load<K>(units + c1 * K), u2 = f2 ? zero : unit_load<K>(units + c2 * K);
            if (f == F_ADD || f == F_SUB || f == F_MAX || f == F_MIN) {
                if (f1) count += dim_demand<K>(units, flags, c1, true, D);
                if (f2) count += dim_demand<K>(units, flags, c2, true, D);
            } else if (f >= F_LT && f <= F_GE) {   // the fixed sibling's unit (0: a free one's)
                if (f1) count += dim_demand<K>(units, flags, c1, true, u2);
                if (f2) count += dim_demand<K>(units, flags, c2, true, u1);
            } else if (f == F_MUL || f == F_DIV || f == F_LOOSE_DIV) {
                const int sg = f == F_MUL ? -1 : 1;
                if (f1) {   // a * b = D: a = D - u(b);  a / b = D: a = D + u(b)  (both free: u(b) is 0, b takes 0)
                    const bool in = unit_combine<K>(1, D, sg, u2, w);
                    count += dim_demand<K>(units, flags, c1, in, w);
                }
                if (f2) {   // b = D - u(a);  b = u(a) - D
                    const bool in = f1 ? unit_combine<K>(0, D, 0, zero, w) : unit_combine<K>(-sg, D, sg, u1, w);
                    count += dim_demand<K>(units, flags, c2, in, w);
                }
            } else {   // pow, loose_pow, an unknown id
                if (f1) count += dim_demand<K>(units, flags, c1, true, zero);
                if (f2) count += dim_demand<K>(units, flags, c2, true, zero);
            }
        }
    }
    violations[t] = count;
}

template <int K>
int launch_dimensions(unsigned pop, unsigned gp_len, unsigned var_len, const float *value, const int16_t *type, const int16_t *size,
                      const int *var_units, const int *label_units, int check_root, int *units, unsigned char *flags, int *violations,
                      hipStream_t stream) {
    const dim3 grid((pop + (unsigned)kWave - 1u) / (unsigned)kWave), block(kWave);
    const unsigned long long words = (unsigned long long)var_len * K;
    if (words <= kDimLdsWords)
        hipLaunchKernelGGL((tree_dimensions_kernel<K, true>), grid, block, (size_t)words * sizeof(int), stream, value, type, size, var_units,
                           label_units, check_root, pop, gp_len, var_len, units, flags, violations);
    else
        hipLaunchKernelGGL((tree_dimensions_kernel<K, false>), grid, block, 0, stream, value, type, size, var_units, label_units, check_root,
                           pop, gp_len, var_len, units, flags, violations);
    return (int)hipGetLastError();
}

} // namespace

extern "C" int evogp_hip_tree_dimensions(unsigned pop, unsigned gp_len, unsigned var_len, unsigned n_dims, const float *value,
                                         const int16_t *type, const int16_t *size, const int *var_units, const int *label_units,
                                         int check_root, int *units, unsigned char *flags, int *violations, evogp_stream_t stream_) {
    if (pop == 0 || pop > 0x7FFFFFFFu || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || n_dims == 0 ||
        n_dims > (unsigned)EVOGP_DIM_MAX_DIMS)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !var_units || !label_units || !units || !flags || !violations) return EVOGP_E_NULLPTR;
    hipStream_t stream = (hipStream_t)stream_;
#define EVOGP_DIMS_CASE(K_) \
    case K_: return launch_dimensions<K_>(pop, gp_len, var_len, value, type, size, var_units, label_units, check_root, units, flags, violations, stream)
    switch (n_dims) {
        EVOGP_DIMS_CASE(1);
        EVOGP_DIMS_CASE(2);
        EVOGP_DIMS_CASE(3);
        EVOGP_DIMS_CASE(4);
        EVOGP_DIMS_CASE(5);
        EVOGP_DIMS_CASE(6);
        EVOGP_DIMS_CASE(7);
        default: EVOGP_DIMS_CASE(8);
    }
#undef EVOGP_DIMS_CASE
}
