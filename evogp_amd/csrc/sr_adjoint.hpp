// sr_adjoint.hpp — the adjoint rules of DESIGN.md's "Constant gradients" table, shared by the reverse walks of sr_grad.hip (gradient of
// the loss) and sr_lm.hip (per-row Jacobian of the prediction), and the number of constants per tree the Levenberg-Marquardt
// optimiser tunes.
#pragma once
#include "sr_forward.hpp"
#include "../../include/evogp_hip.h"

namespace evogp {

constexpr int kLmMaxConsts = EVOGP_LM_MAX_CONSTS;  // K of sr_lm.hip (include/evogp_hip.h)

// Partial adjoints of a binary node's operands: g is the adjoint of its result r = f(a, b).
__device__ inline void binary_adjoint(uint32_t op, float a, float b, float r, float g, float &da, float &db) {
    da = 0.0f; db = 0.0f;
    switch (op) {
    case H_ADD: da = g; db = g; break;
    case H_SUB: da = g; db = -g; break;
    case H_MUL: da = g * b; db = g * a; break;
    case H_DIV: da = g / b; db = -g * r / b; break;  // (r is NaN when b == 0)
    case H_BIN_OTHER + (F_LOOSE_DIV - F_LOOSE_DIV): {
        const bool tiny = fabsf(b) <= kDelta;
        const float d = tiny ? copysignf(kDelta, b) : b;
        da = g / d;
        db = tiny ? 0.0f : -g * r / d;
        break;
    }
    case H_BIN_OTHER + (F_POW - F_LOOSE_DIV):
        da = g * b * powf(a, b - 1.0f);
        db = a > 0.0f ? g * r * logf(a) : 0.0f;
        break;
    case H_BIN_OTHER + (F_LOOSE_POW - F_LOOSE_DIV): {
        const float m = fabsf(a);
        da = (a == 0.0f && b == 0.0f) ? 0.0f : g * b * powf(m, b - 1.0f) * sign_of(a);
        db = m > 0.0f ? g * r * logf(m) : 0.0f;
        break;
    }
    case H_BIN_OTHER + (F_MAX - F_LOOSE_DIV): if (a >= b) da = g; else db = g; break;
    case H_BIN_OTHER + (F_MIN - F_LOOSE_DIV): if (a <= b) da = g; else db = g; break;
    default: break;  // LT GT LE GE, unknown ids: 0
    }
}

__device__ inline float unary_adjoint(uint32_t op, float a, float r, float g) {
    switch (op) {
    case H_UN + (F_SIN - F_SIN): return g * cosf(a);
    case H_UN + (F_COS - F_SIN): return -g * sinf(a);
    case H_UN + (F_TAN - F_SIN): return g * (1.0f + r * r);
    case H_UN + (F_SINH - F_SIN): return g * coshf(a);
    case H_UN + (F_COSH - F_SIN): return g * sinhf(a);
    case H_UN + (F_TANH - F_SIN): return g * (1.0f - r * r);
    case H_UN + (F_LOG - F_SIN): return g / a;
    case H_UN + (F_LOOSE_LOG - F_SIN): return a == 0.0f ? 0.0f : g / a;
    case H_UN + (F_EXP - F_SIN): return g * r;
    case H_UN + (F_INV - F_SIN): return a == 0.0f ? __builtin_nanf("") : -g * r * r;
    case H_UN + (F_LOOSE_INV - F_SIN): return fabsf(a) <= kDelta ? 0.0f : -g * r * r;
    case H_UN + (F_NEG - F_SIN): return -g;
    case H_UN + (F_ABS - F_SIN): return g * sign_of(a);
    case H_UN + (F_SQRT - F_SIN): return g * 0.5f / r;
    case H_UN + (F_LOOSE_SQRT - F_SIN): return a == 0.0f ? 0.0f : g * 0.5f / r * sign_of(a);
    default: return 0.0f;  // unknown ids
    }
}

}  // namespace evogp
