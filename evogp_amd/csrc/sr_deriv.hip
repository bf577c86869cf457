// sr_deriv.hip — interval bounds on the partial derivatives of SR trees (gfx950; no counterpart in the reference; Kronberger et al. 2022,
// shape-constrained symbolic regression).  For every node i of every single-output tree and every requested variable v an interval
// [dlo, dhi] and a flag byte that bound d subtree_i / d x_v on ANY real input of a box lower[v] <= x[v] <= upper[v], and tell whether the
// subtree is known to be continuous in x_v there.  The definition -- every rule, every choice, both claims -- is the numpy restatement
// tests/derivative_ref.py; the functions below follow it name by name, in the same order of float32 operations, operand order included,
// so that every rule without a library call gives the same bits.
//
// TWO LAUNCHES.  (1) tree_intervals_kernel<true> (sr_interval_rules.hpp): the walk of the interval pass with the outward variant of its
// rules writes R = (vlo, vhi, vflags), enclosures of the REAL value of every subtree, and verifies every size word and the stack
// discipline on the way.  (2) tree_derivative_intervals_kernel: one lane per (tree, requested variable), grid ceil(pop / 64) x K.  The
// lane walks from the last live node to node 0; it reads the children's R and the node's own Q from launch 1's rows (read-only, shared
// by the K lanes of a tree), keeps child 1's D and R in registers and reads child 2's and 3's D back from its own output row, which
// is the product, not scratch: there is no operand stack, and a chain 401 deep is no special case.  A tree whose vflags[t][0] carries
// MALFORMED is written as malformed and not walked; for every other tree launch 1 has verified every size word the walk uses (child
// indices are clamped to the live prefix all the same: a caller can not make the walk leave its row).
// No dataset, no workspace, no atomics, no host synchronisation; the result of a row does not depend on the other rows.
#include "sr_interval_rules.hpp"

namespace evogp {

constexpr unsigned kDrvJump = 1u, kDrvMalformed = 2u, kDrvDepends = 4u;
constexpr unsigned kDrvCarry = kDrvJump | kDrvDepends;

// interval + - * / on derivative quantities (derivative_ref.d_add .. d_div): the outward rules, the value-style flags dropped.
// Not inlined: one copy of each in the kernel.
static __device__ __noinline__ Itv drv_add(Itv x, Itv y) {
    const Itv r = itv_binary<true>(F_ADD, itv_make(x.lo, x.hi, 0u), itv_make(y.lo, y.hi, 0u), false, false);
    return itv_make(r.lo, r.hi, 0u);
}
static __device__ __noinline__ Itv drv_sub(Itv x, Itv y) {
    const Itv r = itv_binary<true>(F_SUB, itv_make(x.lo, x.hi, 0u), itv_make(y.lo, y.hi, 0u), false, false);
    return itv_make(r.lo, r.hi, 0u);
}
static __device__ __noinline__ Itv drv_mul(Itv x, Itv y) {
    const Itv r = itv_binary<true>(F_MUL, itv_make(x.lo, x.hi, 0u), itv_make(y.lo, y.hi, 0u), false, false);
    return itv_make(r.lo, r.hi, 0u);
}
static __device__ __noinline__ Itv drv_div(Itv x, Itv y) {   // [-inf, +inf] when y holds 0
    const Itv r = itv_binary<true>(F_DIV, itv_make(x.lo, x.hi, 0u), itv_make(y.lo, y.hi, 0u), false, false);
    return itv_make(r.lo, r.hi, 0u);
}
__device__ inline Itv drv_neg(Itv x) { return itv_make(-x.hi, -x.lo, 0u); }
__device__ inline Itv drv_hull(Itv x, Itv y) { return itv_make(itv_min(x.lo, y.lo), itv_max(x.hi, y.hi), 0u); }
__device__ inline Itv drv_point(float c) { return itv_make(c, c, 0u); }
__device__ inline Itv drv_with(Itv d, unsigned fl) { return itv_make(d.lo, d.hi, fl); }
// the rule of function f (interval_ref.unary, not stepped) applied to R(a), flags dropped
__device__ inline Itv drv_rule(int f, Itv ra) {
    const Itv r = itv_unary<false>(f, itv_make(ra.lo, ra.hi, 0u));
    return itv_make(r.lo, r.hi, 0u);
}

// D and flags of a unary node whose child DEPENDS: ra = R(a), q = R(node), da = the child's D with its flags
__device__ inline Itv drv_unary(int f, Itv ra, Itv q, Itv da) {
    unsigned fl = da.fl & kDrvCarry;
    const Itv d = itv_make(da.lo, da.hi, 0u);
    switch (f) {
    case F_NEG: return drv_with(drv_neg(d), fl);
    case F_ABS:
        if (ra.lo >= 0.0f) return drv_with(d, fl);
        if (ra.hi <= 0.0f) return drv_with(drv_neg(d), fl);
        return drv_with(drv_hull(d, drv_neg(d)), fl);
    case F_SQRT:
        if (ra.lo > 0.0f) return drv_with(drv_div(d, drv_mul(drv_point(2.0f), q)), fl);
        return itv_full(fl);
    case F_LOOSE_SQRT: {
        if (itv_has_zero(ra.lo, ra.hi)) return itv_full(fl);
        const Itv r = drv_div(d, drv_mul(drv_point(2.0f), q));
        return drv_with(ra.lo > 0.0f ? r : drv_neg(r), fl);
    }
    case F_INV:
    case F_LOOSE_INV:
        if (f == F_LOOSE_INV && !(ra.lo > kDelta || ra.hi < -kDelta)) return itv_full(fl | kDrvJump);
        if (itv_has_zero(ra.lo, ra.hi)) return itv_full(fl);
        return drv_with(drv_neg(drv_mul(drv_mul(q, q), d)), fl);
    case F_EXP: return drv_with(drv_mul(q, d), fl);
    case F_LOG:
    case F_LOOSE_LOG:
        if (f == F_LOOSE_LOG && itv_has_zero(ra.lo, ra.hi)) return itv_full(fl | kDrvJump);
        if (ra.lo > 0.0f || (f == F_LOOSE_LOG && ra.hi < 0.0f)) return drv_with(drv_div(d, ra), fl);
        return itv_full(fl);
    case F_SIN: return drv_with(drv_mul(drv_rule(F_COS, ra), d), fl);
    case F_COS: return drv_with(drv_mul(drv_neg(drv_rule(F_SIN, ra)), d), fl);
    case F_TAN:
        if (itv_isinf(q.lo) || itv_isinf(q.hi)) fl |= kDrvJump;
        return drv_with(drv_mul(drv_add(drv_point(1.0f), drv_mul(q, q)), d), fl);
    case F_SINH: return drv_with(drv_mul(d, drv_rule(F_COSH, ra)), fl);
    case F_COSH: return drv_with(drv_mul(d, drv_rule(F_SINH, ra)), fl);
    default: {   // F_TANH
        const Itv s = drv_sub(drv_point(1.0f), drv_mul(q, q));
        return drv_with(drv_mul(itv_make(itv_max(s.lo, 0.0f), itv_min(s.hi, 1.0f), 0u), d), fl);
    }
    }
}

// D and flags of a binary node (the caller applies the independence rule): ra, rb = R of the children with their value flags
__device__ inline Itv drv_binary(int f, Itv ra, Itv rb, Itv q, Itv da, Itv db, bool a_nan_const) {
    const Itv xa = itv_make(da.lo, da.hi, 0u), xb = itv_make(db.lo, db.hi, 0u);
    const unsigned fa = da.fl & kDrvCarry, fb = db.fl & kDrvCarry, both = fa | fb;
    switch (f) {
    case F_ADD: return drv_with(drv_add(xa, xb), both);
    case F_SUB: return drv_with(drv_sub(xa, xb), both);
    case F_MUL: return drv_with(drv_add(drv_mul(xa, rb), drv_mul(ra, xb)), both);
    case F_DIV:
    case F_LOOSE_DIV:
        if (f == F_LOOSE_DIV && !(rb.lo > kDelta || rb.hi < -kDelta)) return itv_full(both | kDrvJump);
        if (itv_has_zero(rb.lo, rb.hi)) return itv_full(both);
        return drv_with(drv_div(drv_sub(xa, drv_mul(q, xb)), rb), both);
    case F_POW:
    case F_LOOSE_POW: return itv_full(both | (itv_has_zero(ra.lo, ra.hi) ? kDrvJump : 0u));
    case F_MAX:
    case F_MIN: {
        if (a_nan_const) return drv_with(xb, fb);
        const bool a_nan = (ra.fl & kItvMayNan) != 0;
        if (!a_nan) {
            const bool a_over_b = ra.lo > rb.hi, b_over_a = ra.hi < rb.lo;
            if (f == F_MAX ? a_over_b : b_over_a) return drv_with(xa, fa);
            if (f == F_MAX ? b_over_a : a_over_b) return drv_with(xb, fb);
        }
        return drv_with(drv_hull(xa, xb), both | ((a_nan && (fa & kDrvDepends)) ? kDrvJump : 0u));
    }
    default:   // F_LT .. F_GE
        return itv_make(0.0f, 0.0f, both | (((both & kDrvDepends) && q.lo != q.hi) ? kDrvJump : 0u));
    }
}

__device__ inline Itv drv_ternary(Itv ra, Itv da, Itv db, Itv dc, bool a_nan_const) {
    if (a_nan_const || ra.hi <= 0.0f) return drv_with(dc, dc.fl & kDrvCarry);
    if (ra.lo > 0.0f && !(ra.fl & kItvMayNan)) return drv_with(db, db.fl & kDrvCarry);
    const unsigned fl = (da.fl | db.fl | dc.fl) & kDrvCarry;
    return drv_with(drv_hull(db, dc), fl | ((da.fl & kDrvDepends) ? kDrvJump : 0u));
}

__global__ __launch_bounds__(kWave) void tree_derivative_intervals_kernel(
    const float *__restrict__ value, const int16_t *__restrict__ type, const int16_t *__restrict__ size, const int *__restrict__ wrt,
    const float *__restrict__ vlo, const float *__restrict__ vhi, const unsigned char *__restrict__ vfl, unsigned pop, unsigned gp_len,
    unsigned var_len, float *dlo_out, float *dhi_out, unsigned char *dfl_out) {
    const unsigned lane = threadIdx.x;
    const unsigned t = blockIdx.x * (unsigned)kWave + lane;
    const bool live = t < pop;
    const size_t row = (size_t)(live ? t : 0u) * gp_len;            // the tree's row of the inputs and of launch 1's outputs
    const size_t plane = (size_t)blockIdx.y * pop * gp_len;          // slice k of the (K, pop, L) outputs
    const size_t out = plane + row;
    const int wv = wrt[blockIdx.y];   // (the caller checks the range; an index outside it matches no variable and addresses nothing)
    int n = 0;
    if (live) {
        n = (int)size[row];
        n = n < 0 ? 0 : (n > (int)gp_len ? (int)gp_len : n);
    }

    // the dead words of the workgroup's rows: one row after the other, the lanes along the row
    const unsigned rows_here = min((unsigned)kWave, pop - blockIdx.x * (unsigned)kWave);
    for (unsigned r = 0; r < rows_here; ++r) {
        const int nr = __builtin_amdgcn_readlane(n, (int)r);
        const size_t at = plane + ((size_t)blockIdx.x * kWave + r) * gp_len;
        for (unsigned j = (unsigned)(nr > 0 ? nr : 1) + lane; j < gp_len; j += (unsigned)kWave) {
            dlo_out[at + j] = 0.0f;
            dhi_out[at + j] = 0.0f;
            dfl_out[at + j] = 0;
        }
    }
    if (!live) return;

    if (vfl[row] & kItvMalformed) {
        const float nan = __builtin_nanf("");
        const int m = n > 0 ? n : 1;
        for (int i = 0; i < m; ++i) {
            dlo_out[out + i] = nan;
            dhi_out[out + i] = nan;
            dfl_out[out + i] = (unsigned char)kDrvMalformed;
        }
        return;
    }

    // node i + 1 (child 1 of a function node i): its D, its R, is it a NaN constant
    Itv prev_d = itv_make(0.0f, 0.0f, 0u), prev_r = itv_make(0.0f, 0.0f, 0u);
    bool prev_nanc = false;
    int ty = 0;
    float v = 0.0f;
    Itv q = itv_make(0.0f, 0.0f, 0u);
    if (n > 0) {
        ty = type[row + n - 1]; v = value[row + n - 1];
        q = itv_make(vlo[row + n - 1], vhi[row + n - 1], vfl[row + n - 1]);
    }
    for (int i = n - 1; i >= 0; --i) {
        const int ty_i = ty;
        const float v_i = v;
        const Itv q_i = q;
        if (i > 0) {   // the next node's words
            ty = type[row + i - 1]; v = value[row + i - 1];
            q = itv_make(vlo[row + i - 1], vhi[row + i - 1], vfl[row + i - 1]);
        }
        const Decoded d = decode_node(ty_i, v_i, false, (int)var_len, 1);
        const int arity = 1 - d.delta;
        Itv r = itv_make(0.0f, 0.0f, 0u);
        bool nanc = false;
        if (d.op == H_CONST) {
            const float c = bits2f(d.pay);
            nanc = c != c;
        } else if (d.op == H_VAR) {
            if ((int)d.pay == wv) r = itv_make(1.0f, 1.0f, kDrvDepends);
        } else if (arity == 1) {
            const int f = itv_func_of(d.op);
            if (f >= 0 && (prev_d.fl & kDrvDepends)) r = drv_unary(f, prev_r, q_i, prev_d);
        } else {
            const int c1 = i + 1 > n - 1 ? n - 1 : i + 1;
            int c2 = c1 + (int)size[row + c1];
            c2 = c2 > n - 1 ? n - 1 : (c2 < 0 ? 0 : c2);
            const Itv rb = itv_make(vlo[row + c2], vhi[row + c2], vfl[row + c2]);
            const Itv db = itv_make(dlo_out[out + c2], dhi_out[out + c2], dfl_out[out + c2]);
            if (arity == 2) {
                const int f = itv_func_of(d.op);
                if (f >= 0) r = drv_binary(f, prev_r, rb, q_i, prev_d, db, prev_nanc);
            } else {
                int c3 = c2 + (int)size[row + c2];
                c3 = c3 > n - 1 ? n - 1 : (c3 < 0 ? 0 : c3);
                const Itv dc = itv_make(dlo_out[out + c3], dhi_out[out + c3], dfl_out[out + c3]);
                r = drv_ternary(prev_r, prev_d, db, dc, prev_nanc);
            }
            if (!(r.fl & kDrvDepends)) r = itv_make(0.0f, 0.0f, 0u);   // independence: no taken child depends on x_v
        }
        dlo_out[out + i] = r.lo;
        dhi_out[out + i] = r.hi;
        dfl_out[out + i] = (unsigned char)r.fl;
        prev_d = r;
        prev_r = q_i;
        prev_nanc = nanc;
    }
}

} // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_tree_derivative_intervals(unsigned pop, unsigned gp_len, unsigned var_len, const float *value, const int16_t *type,
                                                   const int16_t *size, const float *lower, const float *upper, unsigned n_wrt,
                                                   const int *wrt, float *vlo, float *vhi, unsigned char *vflags, float *dlo, float *dhi,
                                                   unsigned char *dflags, evogp_stream_t stream_) {
    if (pop == 0 || pop > 0x7FFFFFFFu || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || n_wrt == 0 || n_wrt > 65535u)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !lower || !upper || !wrt || !vlo || !vhi || !vflags || !dlo || !dhi || !dflags) return EVOGP_E_NULLPTR;
    const unsigned blocks = (pop + (unsigned)kWave - 1u) / (unsigned)kWave;
    hipLaunchKernelGGL(tree_intervals_kernel<true>, dim3(blocks), dim3(kWave), 0, (hipStream_t)stream_, value, type, size, lower, upper, pop,
                       gp_len, var_len, vlo, vhi, vflags);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(tree_derivative_intervals_kernel, dim3(blocks, n_wrt), dim3(kWave), 0, (hipStream_t)stream_, value, type, size, wrt, vlo,
                       vhi, vflags, pop, gp_len, var_len, dlo, dhi, dflags);
    return (int)hipGetLastError();
}
