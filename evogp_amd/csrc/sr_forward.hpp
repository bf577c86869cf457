// sr_forward.hpp — what the tape kernels (sr_grad.hip, sr_lm.hip, sr_subtree.hip) share: the value of a node from its operands' values, the
// per-row error, and the OPERAND TABLE wave 0 of a workgroup builds for its tree (for every function node the indices of the nodes
// whose pushed values it pops).  The forward semantics are run_general's (interp.hpp).
#pragma once
#include "interp.hpp"

namespace evogp {

constexpr uint32_t kOpMask = 0xFFu;  // operand-table word: handler id in bits 0..7, "operand k is a CONST node" in bit 8 + k

__device__ inline float sign_of(float a) { return a > 0.0f ? 1.0f : a < 0.0f ? -1.0f : a == 0.0f ? 0.0f : a; }  // NaN stays NaN

__device__ inline float binary_value(uint32_t op, float a, float b) {
    if (op == H_ADD) return a + b;
    if (op == H_SUB) return a - b;
    if (op == H_MUL) return a * b;
    if (op == H_DIV) return b == 0.0f ? __builtin_nanf("") : a / b;
    return op_binary_other<false>(op, a, b);
}

__device__ inline float grad_err(float diff, int use_mse) { return use_mse ? diff * diff : fabsf(diff); }

// Wave 0 of a workgroup: decode the `len` nodes of a TREE_OK tree at `row` into s_op / s_pay and walk it once in execution order
// (reverse prefix) with a stack of node indices (s_stk), leaving in s_kid[i] the operands of function node i (10 bits each, the
// first popped lowest) and in bits 8.. of s_op[i] which of them are CONST nodes.  Called by every lane of the wave.
template <bool MO>
__device__ inline void build_operand_table(const int16_t *type, const float *value, size_t row, int len, int var_len, int out_len,
                                           uint32_t *s_op, uint32_t *s_kid, uint32_t *s_pay, int *s_stk) {
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < len; i += kWave) {
        const Decoded d = decode_node(type[row + i], value[row + i], MO, var_len, out_len);
        s_op[i] = d.op;
        s_pay[i] = d.pay;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int h = 0;
    for (int i = len - 1; i >= 0; --i) {
        const uint32_t op = (uint32_t)uni((int)s_op[i]);
        const int arity = op < H_ADD ? 0 : op < H_UN ? 2 : op < H_IF ? 1 : 3;
        uint32_t kid = 0, flags = 0;
        for (int k = 0; k < arity; ++k) {
            const int c = uni(s_stk[h - 1 - k]);
            kid |= (uint32_t)c << (10 * k);
            if ((uni((int)s_op[c]) & kOpMask) == H_CONST) flags |= 1u << (8 + k);
        }
        h -= arity;
        if (lane == 0) {
            s_stk[h] = i;
            s_kid[i] = kid;
            s_op[i] = op | flags;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        ++h;
    }
}

// The per-stream global tapes of rows too long for LDS (sr_grad.hip owns them; launches on one stream run one after the other, so the
// tape kernels share one buffer per stream).  Grown outside stream captures, freed by evogp_hip_release_workspaces.
float *grad_workspace(hipStream_t stream, size_t bytes, int *rc);

}  // namespace evogp
