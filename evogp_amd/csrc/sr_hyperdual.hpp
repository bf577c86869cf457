// sr_hyperdual.hpp — the node rules of second-order forward mode: a tree interpreted on hyper-dual numbers (v, t_a, t_b, t_ab), whose
// root word t_ab is d^2 T / dx_a dx_b (csrc/sr_hessian.hip; DESIGN.md section 3.36 holds the table; tests/hessian_ref.py restates it).
//
// A VAR node x_a is seeded with t_a = 1, x_b with t_b = 1 (both for a == b), everything else with 0.  Every float32 operation is rounded
// on its own (-ffp-contract=off), in the association written here.  The first partials f', g_a, g_b are sr_adjoint.hpp's pinned table
// with g = 1; this file adds the second partials and the way the four words combine:
//   unary f            r_x = f' a_x                      r_ab = (f'' a_a) a_b + f' a_ab
//   binary g           r_x = g_a a_x + g_b b_x           r_ab = (((g_a a_ab + g_b b_ab) + (g_aa a_a) a_b) + g_ab (a_a b_b + a_b b_a)) + (g_bb b_a) b_b
//   + - neg            word by word
//   *                  r_x = a_x b + a b_x               r_ab = ((a_ab b + a b_ab) + a_a b_b) + a_b b_a
//   / , loose /        through r = a / d:  r_x = (a_x - r b_x) / d,  r_ab = (((a_ab - r_a b_b) - r_b b_a) - r b_ab) / d;  a loose divisor
//                      inside the delta band is a constant: r_x = a_x / d, r_ab = a_ab / d
//   IF                 the four words of the branch taken;  max / min: the four words of the operand the first-order table calls the winner
//   comparisons, unknown ids: zeros
//   abs and the kinks of the loose variants: the table's convention for f', and f'' = 0
//   pow / loose_pow    the closed second partials; d / db is 0 where the table says so (a <= 0), so g_ab and g_bb are 0 there; every
//                      second partial is NaN where a first partial of the table is NaN
// The untaken branch of an IF, the loser of a max / min are never multiplied in: a second derivative is NaN only where the path taken
// makes it so (the reverse walk's 0 * NaN does not occur here).
#pragma once
#include "sr_adjoint.hpp"

namespace evogp {

struct HyperDual { float v, ta, tb, tab; };

// f'(a) from the pinned table.  The LEAN build names the operations it can meet, so the table's transcendental rows are not compiled into it.
template <bool LEAN>
__device__ inline float unary_first(uint32_t op, float a, float r) {
    switch (op) {
    case H_UN + (F_INV - F_SIN): return unary_adjoint(H_UN + (F_INV - F_SIN), a, r, 1.0f);
    case H_UN + (F_LOOSE_INV - F_SIN): return unary_adjoint(H_UN + (F_LOOSE_INV - F_SIN), a, r, 1.0f);
    case H_UN + (F_ABS - F_SIN): return unary_adjoint(H_UN + (F_ABS - F_SIN), a, r, 1.0f);
    case H_UN + (F_SQRT - F_SIN): return unary_adjoint(H_UN + (F_SQRT - F_SIN), a, r, 1.0f);
    case H_UN + (F_LOOSE_SQRT - F_SIN): return unary_adjoint(H_UN + (F_LOOSE_SQRT - F_SIN), a, r, 1.0f);
    default: return LEAN ? 0.0f : unary_adjoint(op, a, r, 1.0f);
    }
}

// f''(a); r = f(a)
template <bool LEAN>
__device__ inline float unary_second(uint32_t op, float a, float r) {
    switch (op) {
    case H_UN + (F_INV - F_SIN): return a == 0.0f ? __builtin_nanf("") : 2.0f * r * r * r;
    case H_UN + (F_LOOSE_INV - F_SIN): return fabsf(a) <= kDelta ? 0.0f : 2.0f * r * r * r;
    case H_UN + (F_ABS - F_SIN): return 0.0f;
    case H_UN + (F_SQRT - F_SIN): return -0.25f / (a * r);
    case H_UN + (F_LOOSE_SQRT - F_SIN): return a == 0.0f ? 0.0f : -0.25f / (fabsf(a) * r);
    default: break;
    }
    if (!LEAN) {
        switch (op) {
        case H_UN + (F_SIN - F_SIN): return -r;
        case H_UN + (F_COS - F_SIN): return -r;
        case H_UN + (F_TAN - F_SIN): return 2.0f * r * (1.0f + r * r);
        case H_UN + (F_SINH - F_SIN): return r;
        case H_UN + (F_COSH - F_SIN): return r;
        case H_UN + (F_TANH - F_SIN): return -2.0f * r * (1.0f - r * r);
        case H_UN + (F_LOG - F_SIN): return -1.0f / (a * a);
        case H_UN + (F_LOOSE_LOG - F_SIN): return a == 0.0f ? 0.0f : -1.0f / (a * a);
        case H_UN + (F_EXP - F_SIN): return r;
        default: break;
        }
    }
    return 0.0f;
}

template <bool LEAN>
__device__ inline HyperDual hd_unary(uint32_t op, const HyperDual &A) {
    const float r = op_unary<LEAN>(op, A.v);
    if (op == H_UN + (F_NEG - F_SIN)) return {r, -A.ta, -A.tb, -A.tab};
    if (op == H_UN_ZERO) return {r, 0.0f, 0.0f, 0.0f};
    const float f1 = unary_first<LEAN>(op, A.v, r), f2 = unary_second<LEAN>(op, A.v, r);
    return {r, f1 * A.ta, f1 * A.tb, f2 * A.ta * A.tb + f1 * A.tab};
}

// the second partials of pow / loose_pow; ga, gb are the table's first partials
__device__ inline void pow_second(bool loose, float a, float b, float r, float ga, float gb, float &gaa, float &gab, float &gbb) {
    const float m = loose ? fabsf(a) : a;
    const bool pos = m > 0.0f;
    const float lm = logf(pos ? m : 1.0f);
    gaa = b * (b - 1.0f) * powf(m, b - 2.0f);
    gab = powf(m, b - 1.0f) * (1.0f + b * lm);
    if (loose) {
        gab = gab * sign_of(a);
        if (a == 0.0f) gaa = 0.0f;   // the kink: f'' = 0
    }
    gab = pos ? gab : 0.0f;
    gbb = pos ? r * lm * lm : 0.0f;
    if (ga != ga || gb != gb) gaa = gab = gbb = __builtin_nanf("");
}

template <bool LEAN>
__device__ inline HyperDual hd_binary(uint32_t op, const HyperDual &A, const HyperDual &B) {
    const float a = A.v, b = B.v;
    const float r = op == H_ADD ? a + b : op == H_SUB ? a - b : op == H_MUL ? a * b
                    : op == H_DIV ? (b == 0.0f ? __builtin_nanf("") : a / b) : op_binary_other<LEAN>(op, a, b);
    if (op == H_ADD) return {r, A.ta + B.ta, A.tb + B.tb, A.tab + B.tab};
    if (op == H_SUB) return {r, A.ta - B.ta, A.tb - B.tb, A.tab - B.tab};
    if (op == H_MUL) return {r, A.ta * b + a * B.ta, A.tb * b + a * B.tb, A.tab * b + a * B.tab + A.ta * B.tb + A.tb * B.ta};
    if (op == H_DIV || op == H_BIN_OTHER + (F_LOOSE_DIV - F_LOOSE_DIV)) {
        const bool tiny = op != H_DIV && fabsf(b) <= kDelta;
        const float d = tiny ? copysignf(kDelta, b) : b;
        if (tiny) return {r, A.ta / d, A.tb / d, A.tab / d};
        const float ra = (A.ta - r * B.ta) / d, rb = (A.tb - r * B.tb) / d;
        return {r, ra, rb, (A.tab - ra * B.tb - rb * B.ta - r * B.tab) / d};
    }
    if (op == H_BIN_OTHER + (F_MAX - F_LOOSE_DIV)) return a >= b ? A : B;
    if (op == H_BIN_OTHER + (F_MIN - F_LOOSE_DIV)) return a <= b ? A : B;
    if (LEAN || op >= H_BIN_OTHER + (F_LT - F_LOOSE_DIV)) return {r, 0.0f, 0.0f, 0.0f};   // the comparisons, an unknown id
    float ga, gb, gaa, gab, gbb;   // pow, loose_pow
    binary_adjoint(op, a, b, r, 1.0f, ga, gb);
    pow_second(op == H_BIN_OTHER + (F_LOOSE_POW - F_LOOSE_DIV), a, b, r, ga, gb, gaa, gab, gbb);
    return {r, ga * A.ta + gb * B.ta, ga * A.tb + gb * B.tb,
            ga * A.tab + gb * B.tab + gaa * A.ta * A.tb + gab * (A.ta * B.tb + A.tb * B.ta) + gbb * B.ta * B.tb};
}

// ---- host side: the launch of sr_hessian.hip, which sr_xgrad.hip's two entry points call when wrt holds pair codes.  The sizes are
// already checked; EVOGP_E_BADARG for a wrt that is not 1 .. 8 distinct pair codes with a <= b < var_len.  Materialising: loss == viol ==
// nullptr; fused: pred == dpred == nullptr.
int hessian_run(unsigned pop, unsigned D, unsigned gp_len, unsigned var_len, const float *value, const int16_t *type, const int16_t *size,
                const float *X, const float *y, const float *dy, const float *dmin, const float *dmax, unsigned n_wrt, const int *wrt,
                float *pred, float *dpred, float *loss, int *viol, hipStream_t stream);

}  // namespace evogp
