// sr_interval_rules.hpp — the device rules and the one-lane-per-tree walk of the interval pass, shared by sr_interval.hip (the fp32 value
// intervals of DESIGN 3.14) and sr_deriv.hip (the outward-rounded enclosures of the real value).  OUT = false gives the
// rules of tests/interval_ref.py, OUT = true those of tests/derivative_ref.py: the results of + - * sqrt loose_sqrt one ulp outward.
#pragma once
#include "interp.hpp"
#include "launch.hpp"
#include "sr_interval.hpp"

namespace evogp {

struct Itv {
    float lo, hi;
    unsigned fl;
};

constexpr float kItvInf = __builtin_huge_valf();

// which of two equal zeros is taken is part of the definition (interval_ref.fmin / fmax)
__device__ inline float itv_min(float a, float b) { return b < a ? b : a; }
__device__ inline float itv_max(float a, float b) { return b > a ? b : a; }
__device__ inline bool itv_isinf(float x) { return x == kItvInf || x == -kItvInf; }
__device__ inline bool itv_has_zero(float lo, float hi) { return lo <= 0.0f && hi >= 0.0f; }
__device__ inline Itv itv_make(float lo, float hi, unsigned fl) { Itv r; r.lo = lo; r.hi = hi; r.fl = fl; return r; }
__device__ inline Itv itv_full(unsigned fl) { return itv_make(-kItvInf, kItvInf, fl); }

// x moved by k ulps (k < 0: down): k times nextafter with -0.0 and +0.0 one point and +-inf the end of the line
__device__ inline float itv_step(float x, int k) {
    const int s = __float_as_int(x);
    int key = s >= 0 ? s : -(s & 0x7FFFFFFF);
    key += k;
    key = key < -0x7F800000 ? -0x7F800000 : (key > 0x7F800000 ? 0x7F800000 : key);
    return bits2f(key >= 0 ? (uint32_t)key : (0x80000000u | (uint32_t)(-key)));
}
__device__ inline Itv itv_out(float lo, float hi, int w, unsigned fl) { return itv_make(itv_step(lo, -w), itv_step(hi, w), fl); }

__device__ inline void itv_abs(float lo, float hi, float &mlo, float &mhi) {
    if (lo >= 0.0f) { mlo = fabsf(lo); mhi = fabsf(hi); }
    else if (hi <= 0.0f) { mlo = fabsf(hi); mhi = fabsf(lo); }
    else { mlo = 0.0f; mhi = itv_max(fabsf(lo), hi); }
}

// The library's own fp32 results (the functions the interpreters call).  Not inlined: one copy of each expansion in the kernel.
static __device__ __noinline__ float itv_lib(int f, float x) {
    switch (f) {
    case F_SIN: return sinf(x);
    case F_COS: return cosf(x);
    case F_TAN: return tanf(x);
    case F_SINH: return sinhf(x);
    case F_COSH: return coshf(x);
    case F_TANH: return tanhf(x);
    case F_EXP: return expf(x);
    default: return logf(x);
    }
}
static __device__ __noinline__ float itv_powf(float a, float b) { return powf(a, b); }

// (an integer lies in [u_lo, u_hi], an endpoint lies within the margin of an integer): float64, + - floor ceil only
__device__ inline void itv_inside(double u_lo, double u_hi, bool &in, bool &near) {
    near = fabs(u_lo - floor(u_lo + 0.5)) <= kItvTrigMargin || fabs(u_hi - floor(u_hi + 0.5)) <= kItvTrigMargin;
    in = ceil(u_lo) <= floor(u_hi);
}

__device__ inline Itv itv_sincos(int f, float lo, float hi, unsigned fl) {
    const Itv full = itv_out(-1.0f, 1.0f, kWSinCos, fl);
    if (itv_isinf(lo) || itv_isinf(hi)) return itv_make(full.lo, full.hi, fl | kItvMayNan);
    const double dlo = (double)lo, dhi = (double)hi;
    if (dhi - dlo >= kItvTwoPi || fabs(dlo) > kItvTrigMax || fabs(dhi) > kItvTrigMax) return full;
    const double top = f == F_SIN ? kItvHalfPi : 0.0, bottom = f == F_SIN ? -kItvHalfPi : kItvPi;
    bool has_max, near1, has_min, near2;
    itv_inside((dlo - top) / kItvTwoPi, (dhi - top) / kItvTwoPi, has_max, near1);
    itv_inside((dlo - bottom) / kItvTwoPi, (dhi - bottom) / kItvTwoPi, has_min, near2);
    if (near1 || near2) return full;
    const float vlo = itv_lib(f, lo), vhi = itv_lib(f, hi);
    const float rlo = has_min ? -1.0f : itv_min(vlo, vhi);
    const float rhi = has_max ? 1.0f : itv_max(vlo, vhi);
    return itv_out(rlo, rhi, kWSinCos, fl);
}

__device__ inline Itv itv_tan(float lo, float hi, unsigned fl) {
    if (itv_isinf(lo) || itv_isinf(hi)) return itv_full(fl | kItvMayNan);
    const double dlo = (double)lo, dhi = (double)hi;
    if (dhi - dlo >= kItvPi || fabs(dlo) > kItvTrigMax || fabs(dhi) > kItvTrigMax) return itv_full(fl);
    bool pole, near;
    itv_inside((dlo - kItvHalfPi) / kItvPi, (dhi - kItvHalfPi) / kItvPi, pole, near);
    if (pole || near) return itv_full(fl);
    const float vlo = itv_lib(F_TAN, lo), vhi = itv_lib(F_TAN, hi);
    return itv_out(vlo, vhi, kWTan, fl);
}

// a / d over up to two divisor intervals (none contains 0): the corner quotients, NaN corners (inf / inf) skipped, one ulp outward
struct ItvParts {
    float lo[2], hi[2];
    int n;
};

__device__ inline ItvParts itv_loose_divisor(float lo, float hi) {
    ItvParts p;
    p.n = 0;
    if (lo <= 0.0f) { p.lo[p.n] = itv_min(lo, -kDelta); p.hi[p.n] = itv_min(hi, -kDelta); ++p.n; }
    if (hi >= 0.0f) { p.lo[p.n] = itv_max(lo, kDelta); p.hi[p.n] = itv_max(hi, kDelta); ++p.n; }
    return p;
}

__device__ inline Itv itv_divide(float alo, float ahi, const ItvParts &p, unsigned fl) {
    float rlo = 0.0f, rhi = 0.0f;
    bool have = false;
    const bool a_inf = itv_isinf(alo) || itv_isinf(ahi);
    for (int k = 0; k < p.n; ++k) {
        const float dlo = p.lo[k], dhi = p.hi[k];
        if (a_inf && (itv_isinf(dlo) || itv_isinf(dhi))) fl |= kItvMayNan;
        const float q[4] = {alo / dlo, alo / dhi, ahi / dlo, ahi / dhi};
        float blo = 0.0f, bhi = 0.0f;
        bool any = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (q[c] != q[c]) continue;
            if (!any) { blo = bhi = q[c]; any = true; }
            else { blo = itv_min(blo, q[c]); bhi = itv_max(bhi, q[c]); }
        }
        if (!any) return itv_full(fl | kItvMayNan);
        if (!have) { rlo = blo; rhi = bhi; have = true; }
        else { rlo = itv_min(rlo, blo); rhi = itv_max(rhi, bhi); }
    }
    return itv_make(itv_step(rlo, -kWDiv), itv_step(rhi, kWDiv), fl);
}

__device__ inline ItvParts itv_one_part(float lo, float hi) {
    ItvParts p;
    p.n = 1;
    p.lo[0] = lo; p.hi[0] = hi;
    p.lo[1] = lo; p.hi[1] = hi;
    return p;
}

// a^b over alo >= +0: monotone in each argument, so the four corners
__device__ inline Itv itv_pow_corners(float alo, float ahi, float blo, float bhi, unsigned fl) {
    const float c0 = itv_powf(alo, blo), c1 = itv_powf(alo, bhi), c2 = itv_powf(ahi, blo), c3 = itv_powf(ahi, bhi);
    const float lo = itv_min(itv_min(c0, c1), itv_min(c2, c3));
    const float hi = itv_max(itv_max(c0, c1), itv_max(c2, c3));
    return itv_out(lo, hi, kWPow, fl);
}

__device__ inline Itv itv_pow(float alo, float ahi, float blo, float bhi, unsigned fl) {
    if (alo > 0.0f || (alo >= 0.0f && blo > 0.0f)) return itv_pow_corners(fabsf(alo), ahi, blo, bhi, fl);
    if (blo == bhi && !itv_isinf(blo) && blo == truncf(blo)) {
        const float n = blo, half = n * 0.5f;
        if (half == truncf(half)) {   // even
            float mlo, mhi;
            itv_abs(alo, ahi, mlo, mhi);
            return itv_pow_corners(mlo, mhi, n, n, fl);
        }
        if (n > 0.0f) {
            const float vlo = itv_powf(alo, n), vhi = itv_powf(ahi, n);
            return itv_out(vlo, vhi, kWPow, fl);
        }
        if (itv_has_zero(alo, ahi)) return itv_full(fl);
        const float vlo = itv_powf(ahi, n), vhi = itv_powf(alo, n);
        return itv_out(vlo, vhi, kWPow, fl);
    }
    return itv_full(fl | kItvMayNan);
}

__device__ inline bool itv_is_point(Itv a, float c) { return a.lo == c && a.hi == c; }

// f: the function id, or -1 for an unknown one.  OUT: the results of sqrt / loose_sqrt one ulp outward (derivative_ref.r_unary)
template <bool OUT>
__device__ inline Itv itv_unary(int f, Itv a) {
    float lo = a.lo, hi = a.hi;
    unsigned fl = a.fl;
    if (f < 0) return itv_make(0.0f, 0.0f, 0u);
    switch (f) {
    case F_NEG: return itv_make(-hi, -lo, fl);
    case F_ABS: {
        float mlo, mhi;
        itv_abs(lo, hi, mlo, mhi);
        return itv_make(mlo, mhi, fl);
    }
    case F_SQRT:
    case F_LOOSE_SQRT: {
        if (f == F_LOOSE_SQRT) {
            float mlo, mhi;
            itv_abs(lo, hi, mlo, mhi);
            lo = mlo; hi = mhi;
        }
        if (hi < 0.0f) return itv_full(fl | kItvMayNan);
        if (lo < 0.0f) { lo = 0.0f; fl |= kItvMayNan; }
        const float slo = sqrtf(lo), shi = sqrtf(hi);
        if (OUT) return itv_make(slo == 0.0f ? slo : itv_step(slo, -1), shi == 0.0f ? shi : itv_step(shi, 1), fl);   // (sqrt(0) is exact)
        return itv_make(slo, shi, fl);
    }
    case F_INV:
        if (itv_has_zero(lo, hi)) return itv_full(fl | kItvMayNan);
        return itv_divide(1.0f, 1.0f, itv_one_part(lo, hi), fl);
    case F_LOOSE_INV: return itv_divide(1.0f, 1.0f, itv_loose_divisor(lo, hi), fl);
    case F_SIN:
    case F_COS: return itv_sincos(f, lo, hi, fl);
    case F_TAN: return itv_tan(lo, hi, fl);
    case F_SINH:
    case F_TANH:
    case F_EXP: {
        const float vlo = itv_lib(f, lo), vhi = itv_lib(f, hi);
        return itv_out(vlo, vhi, f == F_EXP ? kWLogExp : kWHyp, fl);
    }
    case F_COSH: {
        float mlo, mhi;
        itv_abs(lo, hi, mlo, mhi);
        const float vlo = itv_lib(F_COSH, mlo), vhi = itv_lib(F_COSH, mhi);
        return itv_out(vlo, vhi, kWHyp, fl);
    }
    case F_LOG: {
        if (hi < 0.0f) return itv_full(fl | kItvMayNan);
        if (lo < 0.0f) fl |= kItvMayNan;
        const float vlo = lo > 0.0f ? itv_lib(F_LOG, lo) : -kItvInf, vhi = itv_lib(F_LOG, hi);
        return itv_out(vlo, vhi, kWLogExp, fl);
    }
    default: {   // F_LOOSE_LOG
        const bool zero = itv_has_zero(lo, hi);
        float mlo, mhi;
        itv_abs(lo, hi, mlo, mhi);
        if (mhi == 0.0f) return itv_make(-kMaxVal, -kMaxVal, fl);
        const float vlo = zero ? -kItvInf : itv_lib(F_LOG, mlo), vhi = itv_lib(F_LOG, mhi);
        const Itv r = itv_out(vlo, vhi, kWLogExp, fl);
        return itv_make(zero ? -kMaxVal : r.lo, r.hi, fl);
    }
    }
}

__device__ inline Itv itv_compare(int f, Itv a, Itv b) {
    const bool nan = ((a.fl | b.fl) & kItvMayNan) != 0;
    bool can_t, can_f;
    if (f == F_LT) { can_t = a.lo < b.hi; can_f = !(a.hi < b.lo); }
    else if (f == F_GT) { can_t = a.hi > b.lo; can_f = !(a.lo > b.hi); }
    else if (f == F_LE) { can_t = a.lo <= b.hi; can_f = !(a.hi <= b.lo); }
    else { can_t = a.hi >= b.lo; can_f = !(a.lo >= b.hi); }
    can_f = can_f || nan;
    return itv_make(can_f ? -1.0f : 1.0f, can_t ? 1.0f : -1.0f, 0u);
}

// OUT: the results of + - * one ulp outward unless the operation is exact: an endpoint sum with a zero term, a point-zero or point-one
// operand of *, a zero endpoint of * that no underflow produced (derivative_ref.r_binary)
template <bool OUT>
__device__ inline Itv itv_binary(int f, Itv a, Itv b, bool a_nan_const, bool b_nan_const) {
    const float alo = a.lo, ahi = a.hi;
    float blo = b.lo, bhi = b.hi;
    if (f < 0) return itv_make(0.0f, 0.0f, 0u);
    unsigned fl = (a.fl | b.fl) & kItvMayNan;
    const bool a_inf = itv_isinf(alo) || itv_isinf(ahi), b_inf = itv_isinf(blo) || itv_isinf(bhi);
    switch (f) {
    case F_ADD:
    case F_SUB: {
        if (f == F_SUB) { const float t = blo; blo = -bhi; bhi = -t; }
        if ((ahi == kItvInf && blo == -kItvInf) || (alo == -kItvInf && bhi == kItvInf)) fl |= kItvMayNan;
        const float lo = alo + blo, hi = ahi + bhi;
        const Itv r = itv_make(lo != lo ? -kItvInf : lo, hi != hi ? kItvInf : hi, fl);
        if (OUT)   // an endpoint sum one of whose terms is 0 is exact
            return itv_make((alo == 0.0f || blo == 0.0f) ? r.lo : itv_step(r.lo, -1), (ahi == 0.0f || bhi == 0.0f) ? r.hi : itv_step(r.hi, 1), fl);
        return r;
    }
    case F_MUL: {
        if ((itv_has_zero(alo, ahi) && b_inf) || (itv_has_zero(blo, bhi) && a_inf)) fl |= kItvMayNan;
        const float xs[2] = {alo, ahi}, ys[2] = {blo, bhi};
        float c[4];
        bool under = false;   // (OUT) a product of two nonzero endpoints underflowed to 0: a zero endpoint is then not exact
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float x = xs[i], y = ys[j];
                c[2 * i + j] = ((x == 0.0f && itv_isinf(y)) || (y == 0.0f && itv_isinf(x))) ? 0.0f : x * y;
                if (OUT && x != 0.0f && y != 0.0f && c[2 * i + j] == 0.0f) under = true;
            }
        const Itv r = itv_make(itv_min(itv_min(c[0], c[1]), itv_min(c[2], c[3])), itv_max(itv_max(c[0], c[1]), itv_max(c[2], c[3])), fl);
        if (OUT && !(itv_is_point(a, 0.0f) || itv_is_point(b, 0.0f) || itv_is_point(a, 1.0f) || itv_is_point(b, 1.0f)))
            return itv_make((r.lo == 0.0f && !under) ? r.lo : itv_step(r.lo, -1), (r.hi == 0.0f && !under) ? r.hi : itv_step(r.hi, 1), fl);
        return r;
    }
    case F_DIV:
        if (itv_has_zero(blo, bhi)) return itv_full(fl | kItvMayNan);
        return itv_divide(alo, ahi, itv_one_part(blo, bhi), fl);
    case F_LOOSE_DIV: return itv_divide(alo, ahi, itv_loose_divisor(blo, bhi), fl);
    case F_POW: return itv_pow(alo, ahi, blo, bhi, fl);
    case F_LOOSE_POW: {
        float mlo, mhi;
        itv_abs(alo, ahi, mlo, mhi);
        Itv r = itv_pow_corners(mlo, mhi, blo, bhi, fl);
        if (itv_has_zero(alo, ahi) && itv_has_zero(blo, bhi)) { r.lo = itv_min(r.lo, 0.0f); r.hi = itv_max(r.hi, 0.0f); }
        return r;
    }
    case F_MAX:
    case F_MIN: {
        if (a_nan_const) return itv_make(blo, bhi, b.fl);
        float lo, hi;
        if (f == F_MAX) {
            lo = itv_max(alo, blo); hi = itv_max(ahi, bhi);
            if (a.fl & kItvMayNan) lo = itv_min(lo, blo);
        } else {
            lo = itv_min(alo, blo); hi = itv_min(ahi, bhi);
            if (a.fl & kItvMayNan) hi = itv_max(hi, bhi);
        }
        return itv_make(lo, hi, b.fl & kItvMayNan);
    }
    default:   // F_LT .. F_GE
        if (a_nan_const || b_nan_const) return itv_make(-1.0f, -1.0f, 0u);
        return itv_compare(f, a, b);
    }
}

__device__ inline Itv itv_ternary(Itv a, Itv b, Itv c, bool a_nan_const) {
    if (a_nan_const || a.hi <= 0.0f) return c;
    if (a.lo > 0.0f && !(a.fl & kItvMayNan)) return b;
    return itv_make(itv_min(b.lo, c.lo), itv_max(b.hi, c.hi), (b.fl | c.fl) & kItvMayNan);
}

// the function id of a handler id (interp.hpp), -1 for the handlers that yield 0
__device__ inline int itv_func_of(uint32_t op) {
    if (op >= H_ADD && op <= H_DIV) return F_ADD + (int)(op - H_ADD);
    if (op >= H_BIN_OTHER && op < H_BIN_ZERO) return F_LOOSE_DIV + (int)(op - H_BIN_OTHER);
    if (op >= H_UN && op < H_UN_ZERO) return F_SIN + (int)(op - H_UN);
    return -1;
}

// OUT = false: the fp32 value intervals (sr_interval.hip); OUT = true: the enclosures of the real value (sr_deriv.hip, launch 1)
template <bool OUT>
__global__ __launch_bounds__(kWave) void tree_intervals_kernel(const float *__restrict__ value, const int16_t *__restrict__ type,
                                                                const int16_t *__restrict__ size, const float *__restrict__ lower,
                                                                const float *__restrict__ upper, unsigned pop, unsigned gp_len,
                                                                unsigned var_len, float *lo_out, float *hi_out, unsigned char *fl_out) {
    const unsigned lane = threadIdx.x;
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
        for (unsigned j = (unsigned)(nr > 0 ? nr : 1) + lane; j < gp_len; j += (unsigned)kWave) {
            lo_out[at + j] = 0.0f;
            hi_out[at + j] = 0.0f;
            fl_out[at + j] = 0;
        }
    }
    if (!live) return;

    bool ok = n > 0;
    int h = 0;               // operand-stack height after the nodes walked so far
    Itv prev = itv_make(0.0f, 0.0f, 0u);   // node i + 1: its interval, its (verified) size, is it a NaN constant
    int prev_size = 0;
    bool prev_nanc = false;
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
        Itv r;
        int span = 1;
        bool nanc = false;
        if (d.op == H_CONST) {
            const float c = bits2f(d.pay);
            nanc = c != c;
            r = nanc ? itv_full(kItvMayNan) : itv_make(c, c, 0u);
        } else if (d.op == H_VAR) {
            r = itv_make(lower[d.pay], upper[d.pay], 0u);
        } else if (arity == 1) {
            span = 1 + prev_size;
            r = itv_unary<OUT>(itv_func_of(d.op), prev);
        } else {
            const int c2 = i + 1 + prev_size;
            const Itv b = itv_make(lo_out[row + c2], hi_out[row + c2], fl_out[row + c2]);
            const int size2 = size[row + c2];
            if (arity == 2) {
                span = 1 + prev_size + size2;
                const int f = itv_func_of(d.op);
                bool b_nanc = false;
                if (f >= F_LT && f <= F_GE) {
                    const float bv = value[row + c2];
                    b_nanc = type[row + c2] == T_CONST && bv != bv;
                }
                r = itv_binary<OUT>(f, prev, b, prev_nanc, b_nanc);
            } else {
                const int c3 = c2 + size2;
                const Itv c = itv_make(lo_out[row + c3], hi_out[row + c3], fl_out[row + c3]);
                span = 1 + prev_size + size2 + (int)size[row + c3];
                r = itv_ternary(prev, b, c, prev_nanc);
            }
        }
        if (sz_i != span) { ok = false; break; }
        lo_out[row + i] = r.lo;
        hi_out[row + i] = r.hi;
        fl_out[row + i] = (unsigned char)r.fl;
        prev = r;
        prev_size = span;
        prev_nanc = nanc;
    }
    if (!ok || h != 1) {
        const float nan = __builtin_nanf("");
        const int m = n > 0 ? n : 1;   // (an empty row marks word 0: the root of every row tells whether it is safe)
        for (int i = 0; i < m; ++i) {
            lo_out[row + i] = nan;
            hi_out[row + i] = nan;
            fl_out[row + i] = (unsigned char)(kItvMayNan | kItvMalformed);
        }
    }
}

} // namespace evogp
