// sr_pair.hip — pairwise semantic moments of single-output SR trees: for E events, one FIRST tree of forest A against M <= 16 CANDIDATE
// trees of forest B each (gfx950; no counterpart in the reference).  include/evogp_hip.h has the contract, DESIGN 3.29 the reasoning.
//
// p_t[d] is the float32 prediction of tree t on row d (batch_evaluate's bits), r_t[d] = (double)p_t[d] - (double)y[d] (y = 0 without
// labels).  For event e with a = first[e], b = candidates[e][m]:
//     own[e] = sum r_a^2      moments[e][m] = { sum r_b^2, sum r_a r_b, sum ((double)p_a - (double)p_b)^2 }
// A tree is UNUSABLE when it is malformed, when a prediction is not finite, or when its index lies outside its forest: an unusable first
// tree makes own[e] and every word of moments[e] NaN, an unusable candidate its three words.  Decided by flags, never by arithmetic.
//
// sr_scale.hip's decomposition, with EVENTS where it has trees:
//   1. sr_pair_kernel          the register interpreter (interp.hpp run_chunk) over row tiles of 64 x K, the LEAN build over every
//                              event, then the FULL build over the events the LEAN one marked.  A workgroup pulls batches of events from
//                              a counter; its waves split the batch's (1 + M) trees per event to classify them, then every wave takes
//                              every event on its own tiles: the first tree ONCE per tile (its K root values and the K labels stay in
//                              registers), then the M candidates one after the other.  After each candidate the lane's three partials
//                              are reduced across the wave and added by lane 0 into the wave's LDS word of (event, m): no lane holds
//                              3 M accumulators, and an event costs M + 1 interpretations per tile.  Non-finite predictions are found
//                              by a ballot.  One thread per word adds the waves' words in wave order and writes it, or NaN by the flags
//   2. sr_pair_general_kernel  one wave per marked event (operand stack in scratch memory, run_general): the events with a tree too deep
//                              for the register stack; with more than 32 variables one wave per PAIR, every pair (kernel 1 is not
//                              launched).  A pair costs two interpretations here: the path is the exception, and it keeps no state
// An event goes to ONE kernel as a whole (a byte per event in the workspace says which).  Both kernels add a pair's terms through
// sr_pair_order.hpp and nothing else, so the words of a pair do not depend on the kernel, the event, the slot, M, E or the neighbours.
// No float atomics, no (pop, D) array, nothing synchronises with the host.
#include "interp.hpp"
#include "launch.hpp"
#include "sr_pair_order.hpp"
#include "sr_params.hpp"

namespace evogp {

constexpr int kPairDepth = 16;     // register stack entries; deeper trees go to the scratch stack
constexpr int kPairLeanWaves = 3;  // resident waves per SIMD of the LEAN build (sr_scale.hip kScaleLeanWaves)
constexpr int kPairBatch = 8;      // events per batch: an event is up to 17 trees, and its words live in LDS
constexpr int kPairSlots = EVOGP_PAIR_MAX_CANDIDATES + 1;   // trees of an event: slot 0 the first tree, slot 1 + m candidate m
constexpr unsigned char kPairNone = 0, kPairDeep = 1, kPairHeavy = 2;

struct PairParams {
    const float *value[2];       // [0] forest A (first trees), [1] forest B (candidates)
    const int16_t *type[2];
    const int16_t *size[2];
    int pop[2], gp_len[2];
    const float *X;              // [D][var_len]
    const float *y;              // [D] or nullptr: every label is 0
    const int *first;            // [E]
    const int *cand;             // [E][M]
    double *own;                 // [E]
    double *mom;                 // [E][M][3]
    unsigned char *mark;         // [E]: kPairDeep "take me in the general kernel", kPairHeavy "take me in the FULL register kernel"
    unsigned *counter;           // as sr_scale.hip: [0] LEAN batch counter, [1] some event is marked deep, [2] some is marked heavy, [3] FULL batch counter
    int E, M, D, var_len, batch, ntiles;
};

// the tree in slot s of event e: its row, its clamped live length; false: its index lies outside its forest
struct PairTree {
    const float *tv;
    const int16_t *tt;
    int len;
};
__device__ inline bool pair_tree(const PairParams &p, int e, int s, PairTree *t) {
    const int f = s == 0 ? 0 : 1;
    const int idx = uni(s == 0 ? p.first[e] : p.cand[(size_t)e * p.M + (s - 1)]);
    if (idx < 0 || idx >= p.pop[f]) return false;
    const size_t row = (size_t)idx * p.gp_len[f];
    t->tv = p.value[f] + row;
    t->tt = p.type[f] + row;
    const int len = uni((int)p.size[f][row]);
    t->len = len < 0 ? 0 : (len > p.gp_len[f] ? p.gp_len[f] : len);
    return true;
}

// ---- 1. the register interpreter (sr_scale_kernel's decomposition over events) -----------------------------------------------------------
template <int VL, bool LEAN>
__device__ inline void pair_interpret(const PairTree &t, int var_len, const typename VecOf<VL>::type (&vars)[kPairK], float (&out)[kPairK]) {
    constexpr int K = kPairK;
    const int lane = threadIdx.x & 63;
    v16f outs[K];
    RegStack<K, kPairDepth> st;
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
        run_chunk<false, LEAN, K, kPairDepth>(opv, payv, n, st, RegVars<VL, K>{vars}, outs);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = st.tos[k];
}

template <int VL, bool LEAN>
__global__ __launch_bounds__(kPairWaves * 64, VL <= 16 ? (LEAN ? kPairLeanWaves : 2) : 1) void sr_pair_kernel(PairParams p) {
    constexpr int K = kPairK, TILE = kPairTile;
    __shared__ double part[2][kPairBatch][kPairSlots][kPairWaves][3];   // per event, slot and wave: slot 0 {Saa}, slot 1 + m {Sbb, Sab, Sdd}; double-buffered by batch parity
    __shared__ int bad_s[2][kPairBatch][kPairSlots][kPairWaves];        // != 0: a prediction of the slot's tree was not finite on the wave's rows
    __shared__ int cls_s[2][kPairBatch][kPairSlots];
    __shared__ unsigned next_s[2];   // (unsigned: the counter runs past E by up to two batches per workgroup)

    if (!LEAN && uni((int)p.counter[2]) == 0) return;   // the LEAN pass marked nothing
    unsigned *const batches = p.counter + (LEAN ? 0 : 3);
    using VARS = typename VecOf<VL>::type;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;   // pair_waves(D)
    const int batch = p.batch;
    const int S = p.M + 1;
    const bool single = p.ntiles <= W;   // every wave owns one tile for its whole life: rows and labels are loaded once

    VARS vars[K];
    float yv[K];
    bool valid[K];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long first = (long long)tile * TILE;   // (64 bits, wave-uniform: D may lie within a tile of INT_MAX)
            const long long left = (long long)p.D - first;
            const int rows = left < TILE ? (int)left : TILE;  // rows of this tile, >= 1
            const int off = k * kWave + lane;
            valid[k] = off < rows;
            const size_t dc = (size_t)first + (size_t)(valid[k] ? off : rows - 1);   // lanes past the end repeat the last row: "finite" is not disturbed
            const float *xr = p.X + dc * p.var_len;
#pragma unroll
            for (int v = 0; v < VL; ++v) vars[k][v] = v < p.var_len ? xr[v] : 0.0f;
            yv[k] = p.y ? p.y[dc] : 0.0f;
        }
    };
    if (single) load_tile(w < p.ntiles ? w : 0);

    if (threadIdx.x == 0) next_s[0] = atomicAdd(batches, (unsigned)batch);
    __syncthreads();
    int par = 0;
    for (;;) {
        const unsigned next = uni(next_s[par]);
        if (next >= (unsigned)p.E) break;
        const int e0 = (int)next;
        const int nb = p.E - e0 < batch ? p.E - e0 : batch;
        if (threadIdx.x == 0) next_s[par ^ 1] = atomicAdd(batches, (unsigned)batch);   // prefetch

        // ---- phase 1: classify the batch's trees, (event, slot) items split between the waves ----
        for (int i = w; i < nb * S; i += W) {
            const int b = i / S, s = i - b * S;
            int c = TREE_SKIP;   // (FULL pass: the event is not marked for it)
            if (LEAN || uni((int)p.mark[e0 + b]) == kPairHeavy) {
                PairTree t;
                c = pair_tree(p, e0 + b, s, &t) ? classify_tree(t.tt, t.tv, t.len, false, p.var_len, 1, kPairDepth, LEAN ? 1 : 0) : TREE_BAD;
            }
            if (lane == 0) cls_s[par][b][s] = c;
        }
        __syncthreads();

        // ---- phase 2: every wave takes every event of the batch on its own rows ----
        for (int b = 0; b < nb; ++b) {
            const int c = lane < S ? cls_s[par][b][lane] : TREE_OK;
            const int c0 = __builtin_amdgcn_readlane(c, 0);
            if (c0 == TREE_SKIP || c0 == TREE_BAD) continue;                                   // not this pass's; all NaN
            if (__ballot(c == TREE_HEAVY || c == TREE_DEEP) != 0ull) continue;                 // another kernel takes the whole event
            const unsigned long long okm = __ballot(c == TREE_OK);
            PairTree ta;
            pair_tree(p, e0 + b, 0, &ta);

            for (int tile = w; tile < p.ntiles; tile += W) {
                if (!single) load_tile(tile);
                const bool head = tile == w;   // the wave's first tile: its words start from 0
                float pa[K];
                pair_interpret<VL, LEAN>(ta, p.var_len, vars, pa);
                {
                    bool bad = false;
                    double ra[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        bad |= !finite_f(pa[k]);
                        ra[k] = valid[k] ? (double)pa[k] - (double)yv[k] : 0.0;
                    }
                    const int any_bad = __any(bad) ? 1 : 0;
                    double *word = part[par][b][0][w];
                    double old = 0.0;
                    int oldbad = 0;
                    if (lane == 0 && !head) { old = word[0]; oldbad = bad_s[par][b][0][w]; }
                    const double saa = pair_add_tile(old, ra, ra);
                    if (lane == 0) { word[0] = saa; bad_s[par][b][0][w] = oldbad | any_bad; }
                }
                for (int m = 0; m < p.M; ++m) {
                    if (((okm >> (m + 1)) & 1ull) == 0ull) continue;
                    PairTree tb;
                    pair_tree(p, e0 + b, m + 1, &tb);
                    float pb[K];
                    pair_interpret<VL, LEAN>(tb, p.var_len, vars, pb);
                    bool bad = false;
                    double ra[K], rb[K], dd[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        bad |= !finite_f(pb[k]);
                        ra[k] = valid[k] ? (double)pa[k] - (double)yv[k] : 0.0;
                        rb[k] = valid[k] ? (double)pb[k] - (double)yv[k] : 0.0;
                        dd[k] = valid[k] ? (double)pa[k] - (double)pb[k] : 0.0;
                    }
                    const int any_bad = __any(bad) ? 1 : 0;
                    double *word = part[par][b][m + 1][w];
                    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
                    int oldbad = 0;
                    if (lane == 0 && !head) { o0 = word[0]; o1 = word[1]; o2 = word[2]; oldbad = bad_s[par][b][m + 1][w]; }
                    const double sbb = pair_add_tile(o0, rb, rb);
                    const double sab = pair_add_tile(o1, ra, rb);
                    const double sdd = pair_add_tile(o2, dd, dd);
                    if (lane == 0) { word[0] = sbb; word[1] = sab; word[2] = sdd; bad_s[par][b][m + 1][w] = oldbad | any_bad; }
                }
            }
        }
        __syncthreads();

        // ---- phase 3: one thread per (event, slot) adds the waves' words in wave order and writes them, or NaN by the flags ----
        for (int j = threadIdx.x; j < nb * S; j += blockDim.x) {
            const int b = j / S, s = j - b * S, e = e0 + b;
            const int c0 = cls_s[par][b][0];
            if (c0 == TREE_SKIP) continue;
            const double nan = __builtin_nan("");
            double *out = s == 0 ? p.own + e : p.mom + ((size_t)e * p.M + (s - 1)) * 3;
            const int nout = s == 0 ? 1 : 3;
            bool heavy = false, deep = false;
            if (c0 != TREE_BAD)
                for (int i = 0; i < S; ++i) {
                    heavy |= cls_s[par][b][i] == TREE_HEAVY;
                    deep |= cls_s[par][b][i] == TREE_DEEP;
                }
            if (heavy || deep) {   // the whole event is another kernel's (HEAVY first: the FULL build classifies again)
                if (s == 0) {
                    p.mark[e] = heavy ? kPairHeavy : kPairDeep;
                    p.counter[heavy ? 2 : 1] = 1u;
                }
                continue;
            }
            if (s == 0) p.mark[e] = kPairNone;
            const int nw = p.ntiles < W ? p.ntiles : W;
            const int cs = cls_s[par][b][s];
            bool unusable = c0 == TREE_BAD || cs == TREE_BAD;
            double tot[3] = {0.0, 0.0, 0.0};
            if (!unusable) {
                for (int i = 0; i < nw; ++i) {
                    unusable |= bad_s[par][b][0][i] != 0 || bad_s[par][b][s][i] != 0;
                    for (int q = 0; q < nout; ++q) tot[q] = pair_add_wave(tot[q], part[par][b][s][i][q]);
                }
            }
            for (int q = 0; q < nout; ++q) out[q] = unusable ? nan : tot[q];
        }
        par ^= 1;
    }
}

// ---- 2. the scratch-stack interpreter: one wave per pair, lanes are rows -------------------------------------------------------------
__global__ __launch_bounds__(64) void sr_pair_general_kernel(PairParams p, int only_marked) {
    constexpr int K = kPairK;
    const int lane = threadIdx.x & 63;
    if (only_marked && uni((int)p.counter[1]) == 0) return;   // no event was too deep for the register stack
    float stk[kMaxStack + 2];
    float outs[1];
    const int W = pair_waves(p.D);
    auto process = [&](int e, int m) {   // the words of pair (e, m), and own[e] with m == 0
        PairTree ta, tb;
        const bool ok_a = pair_tree(p, e, 0, &ta) && uni(classify_tree(ta.tt, ta.tv, ta.len, false, p.var_len, 1, kMaxStack)) == TREE_OK;
        const bool ok_b = ok_a && pair_tree(p, e, m + 1, &tb) && uni(classify_tree(tb.tt, tb.tv, tb.len, false, p.var_len, 1, kMaxStack)) == TREE_OK;
        double tot[4] = {0.0, 0.0, 0.0, 0.0};   // Saa, Sbb, Sab, Sdd
        bool bad_a = false, bad_b = false;
        if (ok_a) {
            for (int w = 0; w < W; ++w) {
                double word[4] = {0.0, 0.0, 0.0, 0.0};
                for (int tile = w; tile < p.ntiles; tile += W) {
                    const long long first = (long long)tile * kPairTile;
                    const long long left = (long long)p.D - first;
                    const int rows = left < kPairTile ? (int)left : kPairTile;
                    double ra[K], rb[K], dd[K];
                    for (int k = 0; k < K; ++k) {
                        const int off = k * kWave + lane;
                        const bool valid = off < rows;
                        const size_t dc = (size_t)first + (size_t)(valid ? off : rows - 1);
                        const float *xr = p.X + dc * p.var_len;
                        const double yd = p.y ? (double)p.y[dc] : 0.0;
                        const float pa = run_general<false>(ta.tt, ta.tv, ta.len, xr, p.var_len, 1, outs, stk);
                        bad_a |= !finite_f(pa);
                        ra[k] = valid ? (double)pa - yd : 0.0;
                        rb[k] = dd[k] = 0.0;
                        if (ok_b) {
                            const float pb = run_general<false>(tb.tt, tb.tv, tb.len, xr, p.var_len, 1, outs, stk);
                            bad_b |= !finite_f(pb);
                            rb[k] = valid ? (double)pb - yd : 0.0;
                            dd[k] = valid ? (double)pa - (double)pb : 0.0;
                        }
                    }
                    word[0] = pair_add_tile(word[0], ra, ra);
                    if (ok_b) {
                        word[1] = pair_add_tile(word[1], rb, rb);
                        word[2] = pair_add_tile(word[2], ra, rb);
                        word[3] = pair_add_tile(word[3], dd, dd);
                    }
                }
                for (int q = 0; q < 4; ++q) tot[q] = pair_add_wave(tot[q], word[q]);
            }
        }
        const bool no_a = !ok_a || __any(bad_a) != 0;
        const bool no_b = no_a || !ok_b || __any(bad_b) != 0;
        if (lane == 0) {
            const double nan = __builtin_nan("");
            if (m == 0) p.own[e] = no_a ? nan : tot[0];
            double *out = p.mom + ((size_t)e * p.M + m) * 3;
            for (int q = 0; q < 3; ++q) out[q] = no_b ? nan : tot[1 + q];
        }
    };
    if (!only_marked) {
        const long long pairs = (long long)p.E * p.M;
        for (long long i = blockIdx.x; i < pairs; i += gridDim.x) process((int)(i / p.M), (int)(i % p.M));
        return;
    }
    // behind the register kernel: a contiguous chunk of the events per wave, their marks read 64 at a time (sr_scale_general_kernel)
    const long long chunk = (((long long)p.E + gridDim.x - 1) / gridDim.x + 63) & ~63ll;
    const long long c0 = blockIdx.x * chunk < p.E ? blockIdx.x * chunk : p.E;
    const long long c1 = c0 + chunk < p.E ? c0 + chunk : p.E;
    for (long long base = c0; base < c1; base += kWave) {
        const long long e = base + lane;
        const bool hit = e < c1 && p.mark[e] == kPairDeep;
        unsigned long long mk = __ballot(hit);
        while (mk) {
            const int b = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            for (int m = 0; m < p.M; ++m) process((int)(base + b), m);
        }
    }
}

template <int VL, bool LEAN>
static hipError_t launch_pair(PairParams p, hipStream_t stream) {
    auto kern = sr_pair_kernel<VL, LEAN>;
    const DeviceInfo &dev = device_info();
    const int W = pair_waves(p.D);
    static int per_cu_cache[kPairWaves + 1] = {0};   // occupancy per block size of THIS instantiation
    int per_cu = per_cu_cache[W];
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, W * 64, 0);
        if (e != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        per_cu_cache[W] = per_cu;
    }
    long blocks = (long)dev.num_cus * per_cu;
    long batch = p.E / (blocks * 16);   // ~16 batches per workgroup: a short tail, rare atomics
    batch = batch < 1 ? 1 : (batch > kPairBatch ? kPairBatch : batch);
    p.batch = (int)batch;
    const long need = (p.E + batch - 1) / batch;
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(W * 64), 0, stream, p);
    return hipGetLastError();
}

static int pair_badarg(unsigned events, unsigned n_cand) {
    if (events > 0x7FFFFFFFu || n_cand == 0 || n_cand > (unsigned)EVOGP_PAIR_MAX_CANDIDATES) return EVOGP_E_BADARG;
    return EVOGP_OK;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_pair_moments_workspace_bytes(unsigned events, unsigned n_cand, unsigned long long *bytes) {
    if (const int rc = pair_badarg(events, n_cand)) return rc;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    a.take<unsigned char>(events);
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_pair_moments(unsigned events, unsigned n_cand, unsigned data_points, unsigned var_len, unsigned pop_a,
                                         unsigned gp_len_a, const float *value_a, const int16_t *type_a, const int16_t *size_a, unsigned pop_b,
                                         unsigned gp_len_b, const float *value_b, const int16_t *type_b, const int16_t *size_b,
                                         const float *variables, const float *labels, const int *first, const int *candidates, double *own_out,
                                         double *moments_out, void *workspace, evogp_stream_t stream_) {
    if (const int rc = pair_badarg(events, n_cand)) return rc;
    if (data_points == 0 || var_len == 0 || pop_a == 0 || pop_b == 0 || gp_len_a == 0 || gp_len_b == 0 || gp_len_a > (unsigned)kMaxStack ||
        gp_len_b > (unsigned)kMaxStack || data_points > 0x7FFFFFFFu || pop_a > 0x7FFFFFFFu || pop_b > 0x7FFFFFFFu || var_len > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value_a || !type_a || !size_a || !value_b || !type_b || !size_b || !variables) return EVOGP_E_NULLPTR;
    if (events == 0) return EVOGP_OK;   // empty outputs: nothing to launch, and nothing to point at
    if (!first || !candidates || !own_out || !moments_out || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const DeviceInfo &dev = device_info();
    hipError_t e;
    Arena a{(char *)workspace};
    PairParams p{};
    p.mark = a.take<unsigned char>(events);
    p.counter = acquire_counter(stream, &e);
    if (!p.counter) return (int)e;
    p.value[0] = value_a; p.type[0] = type_a; p.size[0] = size_a; p.pop[0] = (int)pop_a; p.gp_len[0] = (int)gp_len_a;
    p.value[1] = value_b; p.type[1] = type_b; p.size[1] = size_b; p.pop[1] = (int)pop_b; p.gp_len[1] = (int)gp_len_b;
    p.X = variables; p.y = labels; p.first = first; p.cand = candidates; p.own = own_out; p.mom = moments_out;
    p.E = (int)events; p.M = (int)n_cand; p.D = (int)data_points; p.var_len = (int)var_len;
    p.ntiles = pair_tiles(p.D);
    const bool regs = p.var_len <= 32;
    if (regs) {
        e = p.var_len <= 12 ? launch_pair<12, true>(p, stream) : launch_pair<32, true>(p, stream);
        if (e != hipSuccess) return (int)e;
        e = p.var_len <= 12 ? launch_pair<12, false>(p, stream) : launch_pair<32, false>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    long blocks = (long)dev.num_cus * (regs ? 4 : 16);
    const long long work = regs ? (long long)p.E : (long long)p.E * p.M;
    if (blocks > work) blocks = (long)work;
    hipLaunchKernelGGL(sr_pair_general_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, p, regs ? 1 : 0);
    return (int)hipGetLastError();
}
