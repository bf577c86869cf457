// sr_gram_panel.hpp — the float32 prediction panel of a list of single-output SR trees: the parameters, the per-tree helpers and the three
// panel kernels that sr_gram.hip (the Gram matrix) and sr_neigh.hip (semantic neighbourhoods) both launch.  A kernel fills the rows
// [row0, row0 + rows) of every selected tree into panel[i * stride + (row - row0)]; the caller chooses `stride` and where `panel` points,
// so one user keeps a slab at a time and the other every row.  The non-template kernels are static: each translation unit holds its own.
#pragma once
#include "interp.hpp"
#include "launch.hpp"
#include "sr_gram_order.hpp"
#include "sr_params.hpp"

namespace evogp {

constexpr int kGramK = 4;                      // rows per lane of an interpreter tile
constexpr int kGramTile = kWave * kGramK;      // rows per interpreter tile
constexpr int kGramDepth = 16;                 // register stack entries; deeper trees go to the scratch stack
constexpr int kGramLeanWaves = 3;              // resident waves per SIMD of the LEAN build (sr_pair.hip kPairLeanWaves)
constexpr int kGramWaves = 4;                  // waves of a workgroup, in every kernel of the pass
constexpr int kGramBlock = 64;                 // vectors per side of an output block
constexpr int kGramChunk = 32;                 // rows per LDS chunk: eight matrix-instruction groups between two barriers
constexpr int kGramLd = kGramChunk + 4;        // floats per LDS row: the 16 vectors x 4 rows of an operand read fall in 64 different banks
constexpr unsigned char kGramNone = 0, kGramDeep = 1, kGramHeavy = 2;

static_assert(kGramSlab % kGramSegment == 0 && kGramSegment % kGramChunk == 0 && kGramChunk % kGramGroup == 0 && kGramSlab % kGramTile == 0, "");

struct GramParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    int pop, gp_len;
    const float *X;              // [D][var_len]
    const float *y;              // [D] or nullptr
    const int *index;            // [n]
    float *panel;                // [n][stride]: the predictions of the current slab
    int *bad;                    // [n] != 0: tree i is unusable;  then [2]: some tree is marked heavy, some tree is marked deep
    unsigned char *mark;         // [n]: which later panel kernel takes the tree
    double *part;                // [segments of a slab][blocks][64][64]: partial blocks (small n only)
    double *G, *lin;             // [n][n], [n][2]
    unsigned char *usable;       // [n]
    int n, D, var_len, residuals, stride;
    int row0, rows;              // the current slab: its first row and its 1 .. kGramSlab rows
};

struct GramTree {
    const float *tv;
    const int16_t *tt;
    int len;
};
__device__ inline bool gram_tree(const GramParams &p, int i, GramTree *t) {
    const int idx = uni(p.index[i]);
    if (idx < 0 || idx >= p.pop) return false;
    const size_t row = (size_t)idx * p.gp_len;
    t->tv = p.value + row;
    t->tt = p.type + row;
    const int len = uni((int)p.size[row]);
    t->len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
    return true;
}

// ---- 1. the panel: every selected tree interpreted once per slab ------------------------------------------------------------------------
template <int VL, bool LEAN>
__device__ inline void gram_interpret(const GramTree &t, int var_len, const typename VecOf<VL>::type (&vars)[kGramK], float (&out)[kGramK]) {
    constexpr int K = kGramK;
    const int lane = threadIdx.x & 63;
    v16f outs[K];
    RegStack<K, kGramDepth> st;
    st.h = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) st.tos[k] = 0.0f;
    for (int base = 0; base < t.len; base += kWave) {
        const int r = base + lane;
        uint32_t opv = 0, payv = 0;
        if (r < t.len) {
            const int i = t.len - 1 - r;
            const Decoded dn = decode_node(t.tt[i], t.tv[i], false, var_len, 1);
            opv = dn.op; payv = dn.pay;
        }
        const int n = t.len - base < kWave ? t.len - base : kWave;
        run_chunk<false, LEAN, K, kGramDepth>(opv, payv, n, st, RegVars<VL, K>{vars}, outs);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = st.tos[k];
}

// the panel words of a tree that is unusable by its structure or its index: zeros
__device__ inline void gram_zero_row(const GramParams &p, int i) {
    float *row = p.panel + (size_t)i * p.stride;
    for (int r = threadIdx.x; r < p.rows; r += blockDim.x) row[r] = 0.0f;
    if (threadIdx.x == 0) p.bad[i] = 1;
}

template <int VL, bool LEAN>
__global__ __launch_bounds__(kGramWaves * 64, VL <= 16 ? (LEAN ? kGramLeanWaves : 2) : 1) void gram_panel_kernel(GramParams p) {
    constexpr int K = kGramK, TILE = kGramTile;
    using VARS = typename VecOf<VL>::type;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int i = blockIdx.x;
    int *const flags = p.bad + p.n;
    if (!LEAN && (uni(flags[0]) == 0 || uni((int)p.mark[i]) != kGramHeavy)) return;

    GramTree t;
    const int c = gram_tree(p, i, &t) ? classify_tree(t.tt, t.tv, t.len, false, p.var_len, 1, kGramDepth, LEAN ? 1 : 0) : TREE_BAD;
    if (c == TREE_BAD) {
        gram_zero_row(p, i);
        if (LEAN && threadIdx.x == 0) p.mark[i] = kGramNone;
        return;
    }
    if (c == TREE_HEAVY || c == TREE_DEEP) {   // another panel kernel fills the row
        if (threadIdx.x == 0) {
            p.mark[i] = c == TREE_HEAVY ? kGramHeavy : kGramDeep;
            flags[c == TREE_HEAVY ? 0 : 1] = 1;
        }
        return;
    }
    if (LEAN && threadIdx.x == 0) p.mark[i] = kGramNone;   // (the FULL build's waves read their mark on entry: it stays)

    float *const out = p.panel + (size_t)i * p.stride;
    const int ntiles = (p.rows + TILE - 1) / TILE;
    bool bad = false;
    for (int tile = w; tile < ntiles; tile += kGramWaves) {
        const int first = tile * TILE;
        const int rows = p.rows - first < TILE ? p.rows - first : TILE;   // rows of this tile, >= 1
        VARS vars[K];
        bool valid[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int off = k * kWave + lane;
            valid[k] = off < rows;
            const size_t dc = (size_t)p.row0 + (size_t)first + (size_t)(valid[k] ? off : rows - 1);   // lanes past the end repeat the last row
            const float *xr = p.X + dc * p.var_len;
#pragma unroll
            for (int v = 0; v < VL; ++v) vars[k][v] = v < p.var_len ? xr[v] : 0.0f;
        }
        float pr[K];
        gram_interpret<VL, LEAN>(t, p.var_len, vars, pr);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool fin = finite_f(pr[k]);
            bad |= !fin;
            if (valid[k]) out[first + k * kWave + lane] = fin ? pr[k] : 0.0f;
        }
    }
    if (__any(bad) && lane == 0) p.bad[i] = 1;
}

// the scratch-stack interpreter: a workgroup per tree, lanes are rows; every tree (`all`: var_len > 32) or the trees marked deep
static __global__ __launch_bounds__(kGramWaves * 64) void gram_panel_general_kernel(GramParams p, int all) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x;
    if (!all && (uni(p.bad[p.n + 1]) == 0 || uni((int)p.mark[i]) != kGramDeep)) return;
    float stk[kMaxStack + 2];
    float outs[1];
    GramTree t;
    if (!gram_tree(p, i, &t) || uni(classify_tree(t.tt, t.tv, t.len, false, p.var_len, 1, kMaxStack)) != TREE_OK) {
        gram_zero_row(p, i);
        return;
    }
    float *const out = p.panel + (size_t)i * p.stride;
    bool bad = false;
    for (int base = (int)(threadIdx.x >> 6) * kWave; base < p.rows; base += kGramWaves * kWave) {
        const int r = base + lane;
        const bool valid = r < p.rows;
        const float *xr = p.X + ((size_t)p.row0 + (size_t)(valid ? r : p.rows - 1)) * p.var_len;
        const float pr = run_general<false>(t.tt, t.tv, t.len, xr, p.var_len, 1, outs, stk);
        const bool fin = finite_f(pr);
        bad |= !fin;
        if (valid) out[r] = fin ? pr : 0.0f;
    }
    if (__any(bad) && lane == 0) p.bad[i] = 1;
}

template <int VL, bool LEAN>
static hipError_t launch_panel(const GramParams &p, hipStream_t stream) {
    hipLaunchKernelGGL((gram_panel_kernel<VL, LEAN>), dim3((unsigned)p.n), dim3(kGramWaves * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace evogp
