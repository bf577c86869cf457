// sr_forward.hpp — what the tape kernels (sr_grad.hip, sr_lm.hip, sr_subtree.hip, sr_subtree_sig.hip) share: the value of a node from its operands' values, the
// per-row error, the OPERAND TABLE wave 0 of a workgroup builds for its tree (for every function node the indices of the nodes
// whose pushed values it pops) and, on the host, the LAUNCH PLAN of the three passes (plan_tape_launch).  The forward semantics are
// run_general's (interp.hpp).
#pragma once
#include "interp.hpp"
#include "launch.hpp"

#include <initializer_list>

namespace evogp {

constexpr int kTapeLdsLen = 64;     // rows up to this length keep their two [node][lane] tapes in LDS (2 x 64 x 256 B = 32 KiB per wave)
constexpr int kTapeMaxWaves = 4;    // waves per workgroup (row tiles of one tree)

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

// ---- host side: the launch of a tape kernel --------------------------------------------------------------------------------------
// The per-stream global tapes of rows too long for LDS: one block per stream (g_tape_workspaces, launch.hpp), which the three passes share.
inline float *grad_workspace(hipStream_t stream, size_t bytes, int *rc) { return g_tape_workspaces.get(stream, bytes, rc); }

struct TapePlan {
    int W;          // waves per workgroup
    long blocks;    // workgroups (each takes trees blocks apart)
    size_t lds;     // dynamic LDS of a workgroup in bytes: the kernel's head and, for rows of at most kTapeLdsLen nodes, its W x tape_words tapes
    float *tape;    // global tapes [blocks * W][tape_words][gp_len][64] of longer rows; nullptr: the tapes are in LDS
};

// The plan of one pass over `pop` rows of `gp_len` words and D data points on `stream`; head_words(L, W) is the kernel's own LDS in
// front of the tapes (its layout stays next to the kernel that carves it).  Returns 0, or the error of the workspace request.
// THE CONTRACT: W and blocks depend on nothing but (pop, D, gp_len) and the device, so the gradient, the normal-equation and the
// subtree pass split the rows of a tree among the same waves and sum them in the same order: their losses are equal bit for bit.
// tape_words: 32-bit words a wave keeps per node and lane (two float tapes in the three passes above, the value tape alone in
// sr_subtree_sig.hip); it sizes the LDS and the global workspace and therefore `blocks` of an LDS-tape launch, never W.
inline int plan_tape_launch(int pop, int D, int gp_len, hipStream_t stream, size_t (*head_words)(int L, int W), TapePlan *plan,
                            int tape_words = 2) {
    const DeviceInfo &dev = device_info();
    const int ntiles = (D + kWave - 1) / kWave;
    const bool lds_tape = gp_len <= kTapeLdsLen;
    // Waves per workgroup: one when the population alone fills the chip, up to four (row tiles of one tree) when it does not.
    const long fill = (long)dev.num_cus * 16;
    const int W = pop >= fill ? 1 : (ntiles < kTapeMaxWaves ? ntiles : kTapeMaxWaves);
    size_t lds = head_words(gp_len, W) * 4;
    long blocks;
    if (lds_tape) {
        lds += (size_t)W * tape_words * gp_len * kWave * sizeof(float);
        const long per_cu = (long)(dev.lds_per_cu / lds);
        blocks = (long)dev.num_cus * (per_cu < 1 ? 1 : per_cu);
    } else {
        blocks = (long)dev.num_cus * 2 / W;  // 512 resident waves on a 256-CU device: 256 MiB of tapes at gp_len 1024
    }
    if (blocks > pop) blocks = pop;
    *plan = {W, blocks, lds, nullptr};
    if (!lds_tape) {
        int rc = 0;
        plan->tape = grad_workspace(stream, (size_t)blocks * W * tape_words * gp_len * kWave * sizeof(float), &rc);
        if (!plan->tape) return rc;
    }
    return 0;
}

// Dynamic LDS beyond 64 KiB must be granted per kernel: once per LdsGrant (a static of the entry point), the first error sticks.
struct LdsGrant { std::once_flag once; hipError_t err = hipSuccess; };
inline hipError_t grant_tape_lds(LdsGrant &g, std::initializer_list<const void *> kernels) {
    std::call_once(g.once, [&] {
        for (const void *k : kernels)
            if (g.err == hipSuccess) g.err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    return g.err;
}

}  // namespace evogp
