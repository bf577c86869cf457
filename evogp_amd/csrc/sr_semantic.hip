// sr_semantic.hip — semantic duplicate classes of single-output SR trees: trees whose float32 predictions agree on every row of a
// dataset (gfx950; no counterpart in the reference).  include/evogp_hip.h has the contract, DESIGN 3.18 the reasoning.
//
// p[t][d] is the float32 prediction of tree t on row d (batch_evaluate's bits); its KEY is the bit pattern with -0.0 -> +0.0 and every
// NaN -> 0x7FC00000.  Two trees are EQUAL when both are well formed (classify_tree != TREE_BAD) and their keys agree on every row.
//
// evogp_hip_sr_semantic_hash:  sig[t] = mix64((sum_{d<D} mix64(key[t][d] ^ ((d + 1) * GOLD))) + D) mod 2^64, 0 for a malformed row.  The
// sum is position-keyed and modular, so no order of lanes, tiles or waves changes it.  sr_scale.hip's decomposition with an integer
// epilogue -- no labels, no float64, no float atomics:
//   1. sr_semantic_kernel          the register interpreter (interp.hpp run_chunk) over row tiles of 64 x K, the LEAN build over every
//                                  tree, then the FULL build over the trees the LEAN one marked.  A lane adds the terms of its rows, the
//                                  64 lanes are added by wave_sum_u64, the waves' partials are parked in LDS and added by one thread
//                                  per tree.  The DEEP / HEAVY marks cannot live in the output word (every 64-bit pattern is a valid
//                                  signature): they are a byte per tree in the workspace
//   2. sr_semantic_general_kernel  a wave per tree with the operand stack in scratch memory (run_general): the trees marked DEEP, and
//                                  every tree of a forest with more variables than the register tuples hold
//
// evogp_hip_sr_semantic_classes: class_id[t] = the smallest index of a tree equal to tree t.  Stages 1-3 are dedup.hip's (pairs, the
// stable sort of (hash, index), run starts); stage 4 is one wave per sorted position s: its tree is compared with the trees at st,
// st + 1, ..., s - 1 of its run in that order and takes the first equal one, else itself.  A comparison: (a) equal live prefixes are
// equal trees, no evaluation; (b) else both trees are evaluated by run_general on chunks of 64 rows, a row per lane, and (c) the wave
// leaves at the first chunk with a differing key.  Only equality decides a class; the hashes decide which trees are compared.  Without
// a collision every member of a class pays one comparison; a run of r distinct colliding trees costs O(r^2) comparisons of up to
// 2 D evaluations each.
#include "dedup.hpp"
#include "interp.hpp"
#include "launch.hpp"
#include "sem_key.hpp"
#include "sr_params.hpp"

namespace evogp {

constexpr int kSemK = 4;        // rows per lane
constexpr int kSemDepth = 16;   // register stack entries; deeper trees go to the scratch stack
constexpr int kSemWaves = 4;    // waves per workgroup: a workgroup's row tile is 64 * kSemK * kSemWaves = 1024 rows
constexpr int kSemLeanWaves = 3;   // resident waves per SIMD of the LEAN build (sr_scale.hip kScaleLeanWaves)
constexpr unsigned char kMarkNone = 0, kMarkDeep = 1, kMarkHeavy = 2;

struct SemParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;              // [D][var_len]
    unsigned long long *sig;     // [pop]
    unsigned char *mark;         // [pop]: kMarkDeep "evaluate me in the general kernel", kMarkHeavy "evaluate me in the FULL register kernel"
    unsigned *counter;           // as sr_scale.hip: [0] LEAN batch counter, [1] some tree is marked deep, [2] some is marked heavy, [3] FULL batch counter
    int pop, D, gp_len, var_len, batch, ntiles;
};

// sem_key, sem_term and sem_finish (the key of a prediction, the term of a row, the last mix) are sem_key.hpp's

// ---- 1. the register interpreter (sr_scale_kernel's decomposition) -----------------------------------------------------------------------
template <int VL, bool LEAN>
__global__ __launch_bounds__(kSemWaves * 64, VL <= 16 ? (LEAN ? kSemLeanWaves : 2) : 1) void sr_semantic_kernel(SemParams p) {
    constexpr int K = kSemK, DEPTH = kSemDepth, TILE = kWave * K;
    __shared__ unsigned long long part[2][kMaxBatch][kSemWaves];   // per tree and wave; double-buffered by batch parity
    __shared__ int cls_s[2][kMaxBatch];
    __shared__ unsigned next_s[2];   // (unsigned: the counter runs past pop by up to two batches per workgroup)

    if (!LEAN && uni((int)p.counter[2]) == 0) return;   // the LEAN pass marked nothing
    unsigned *const batches = p.counter + (LEAN ? 0 : 3);
    using VARS = typename VecOf<VL>::type;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;
    const int batch = p.batch;
    const bool single = p.ntiles <= W;   // every wave owns one tile for its whole life: its rows are loaded once

    VARS vars[K];
    bool valid[K];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long first = (long long)tile * TILE;   // (64 bits, wave-uniform: D may lie within a tile of INT_MAX)
            const long long left = (long long)p.D - first;
            const int rows = left < TILE ? (int)left : TILE;  // rows of this tile, >= 1
            const int off = k * kWave + lane;
            valid[k] = off < rows;
            const size_t dc = (size_t)first + (size_t)(valid[k] ? off : rows - 1);   // lanes past the end repeat the last row and add nothing
            const float *xr = p.X + dc * p.var_len;
#pragma unroll
            for (int v = 0; v < VL; ++v) vars[k][v] = v < p.var_len ? xr[v] : 0.0f;
        }
    };
    if (single) load_tile(w < p.ntiles ? w : 0);

    if (threadIdx.x == 0) next_s[0] = atomicAdd(batches, (unsigned)batch);
    __syncthreads();
    int par = 0;
    for (;;) {
        const unsigned next = uni(next_s[par]);
        if (next >= (unsigned)p.pop) break;
        const int t0 = (int)next;
        const int nb = p.pop - t0 < batch ? p.pop - t0 : batch;
        if (threadIdx.x == 0) next_s[par ^ 1] = atomicAdd(batches, (unsigned)batch);   // prefetch

        // ---- phase 1: classify the batch, trees split between the waves ----
        for (int b = w; b < nb; b += W) {
            const size_t row = (size_t)(t0 + b) * p.gp_len;
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
            int c = TREE_SKIP;   // (FULL pass: not marked for it)
            if (LEAN || uni((int)p.mark[t0 + b]) == kMarkHeavy)
                c = classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, DEPTH, LEAN ? 1 : 0);
            if (lane == 0) cls_s[par][b] = c;
        }
        __syncthreads();

        // ---- phase 2: every wave interprets every tree of the batch on its own rows ----
        for (int b = 0; b < nb; ++b) {
            if (uni(cls_s[par][b]) != TREE_OK) continue;
            const size_t row = (size_t)(t0 + b) * p.gp_len;
            const float *tv = p.value + row;
            const int16_t *tt = p.type + row;
            int len = uni((int)p.size[row]);
            len = len > p.gp_len ? p.gp_len : len;

            unsigned long long acc = 0ull;
            for (int tile = w; tile < p.ntiles; tile += W) {
                if (!single) load_tile(tile);
                v16f outs[K];
                RegStack<K, DEPTH> st;
                st.h = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) st.tos[k] = 0.0f;
                for (int base = 0; base < len; base += kWave) {
                    const int r = base + lane;
                    uint32_t opv = 0, payv = 0;
                    if (r < len) {
                        const int i = len - 1 - r;
                        const Decoded dn = decode_node(tt[i], tv[i], false, p.var_len, 1);
                        opv = dn.op; payv = dn.pay;
                    }
                    const int n = len - base < kWave ? len - base : kWave;
                    run_chunk<false, LEAN, K, DEPTH>(opv, payv, n, st, RegVars<VL, K>{vars}, outs);
                }
                const unsigned long long d0 = (unsigned long long)tile * TILE + (unsigned)lane;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const unsigned long long term = sem_term(st.tos[k], d0 + (unsigned)(k * kWave));
                    acc += valid[k] ? term : 0ull;
                }
            }
            const unsigned long long tot = wave_sum_u64(acc);
            if (lane == 0) part[par][b][w] = tot;
        }
        __syncthreads();

        // ---- phase 3: one thread per tree adds the waves' partials and finishes the signature ----
        if ((int)threadIdx.x < nb) {
            const int b = threadIdx.x, t = t0 + b;
            const int c = cls_s[par][b];
            if (c == TREE_OK) {
                const int nw = p.ntiles < W ? p.ntiles : W;
                unsigned long long sum = 0ull;
                for (int i = 0; i < nw; ++i) sum += part[par][b][i];
                p.sig[t] = sem_finish(sum, p.D);
                p.mark[t] = kMarkNone;
            } else if (c != TREE_SKIP) {
                p.sig[t] = 0ull;   // (a malformed row keeps this; a marked one is written again by the kernel it is marked for)
                p.mark[t] = c == TREE_DEEP ? kMarkDeep : c == TREE_HEAVY ? kMarkHeavy : kMarkNone;
                if (c == TREE_DEEP) p.counter[1] = 1u;
                if (c == TREE_HEAVY) p.counter[2] = 1u;
            }
        }
        par ^= 1;
    }
}

// ---- 2. the scratch-stack interpreter: one wave per tree, lanes are rows --------------------------------------------------------------
__global__ __launch_bounds__(64) void sr_semantic_general_kernel(SemParams p, int only_marked) {
    const int lane = threadIdx.x & 63;
    if (only_marked && uni((int)p.counter[1]) == 0) return;   // no tree was too deep for the register stack
    float stk[kMaxStack + 2];
    float outs[1];
    auto process = [&](int t) {
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *tt = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int cls = uni(classify_tree(tt, tv, len, false, p.var_len, 1, kMaxStack));
        unsigned long long sig = 0ull;
        if (cls == TREE_OK) {
            unsigned long long acc = 0ull;
            for (long long base = 0; base < p.D; base += kWave) {
                const long long d = base + lane;
                const bool valid = d < p.D;
                const size_t dc = valid ? (size_t)d : (size_t)p.D - 1;
                const float pr = run_general<false>(tt, tv, len, p.X + dc * p.var_len, p.var_len, 1, outs, stk);
                const unsigned long long term = sem_term(pr, (unsigned long long)dc);
                acc += valid ? term : 0ull;
            }
            sig = sem_finish(wave_sum_u64(acc), p.D);
        }
        if (lane == 0) p.sig[t] = sig;
    };
    if (!only_marked) {
        for (long long t = blockIdx.x; t < p.pop; t += gridDim.x) process((int)t);
        return;
    }
    // behind the register kernel: a contiguous chunk of the population per wave, its marks read 64 at a time (sr_scale_general_kernel)
    const long long chunk = (((long long)p.pop + gridDim.x - 1) / gridDim.x + 63) & ~63ll;   // (64 bits: pop may lie near INT_MAX)
    const long long c0 = blockIdx.x * chunk < p.pop ? blockIdx.x * chunk : p.pop;
    const long long c1 = c0 + chunk < p.pop ? c0 + chunk : p.pop;
    for (long long base = c0; base < c1; base += kWave) {
        const long long t = base + lane;
        const bool hit = t < c1 && p.mark[t] == kMarkDeep;
        unsigned long long mk = __ballot(hit);
        while (mk) {
            const int b = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            process((int)(base + b));
        }
    }
}

// ---- stage 4 of the classes pass: one wave per sorted position ------------------------------------------------------------------------
struct SemClassParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;            // [D][var_len]
    const unsigned *members;   // [pop]: tree indices sorted by (hash, index)
    const unsigned *seg;       // [pop]: the start of the run position s lies in
    int *class_id;             // [pop]
    int pop, D, gp_len, var_len;
};

__global__ __launch_bounds__(64) void sr_semantic_classes_kernel(SemClassParams q) {
    const int lane = threadIdx.x & 63;
    float stk[kMaxStack + 2];
    float outs[1];
    for (long long s = blockIdx.x; s < q.pop; s += gridDim.x) {
        const unsigned t = uni(q.members[s]);
        const unsigned st = uni(q.seg[s]);
        unsigned rep = t;
        if ((long long)st < s) {   // (a position that heads its run is its own class)
            const size_t row = (size_t)t * q.gp_len;
            const float *tv = q.value + row;
            const int16_t *tt = q.type + row;
            int n = uni((int)q.size[row]);
            n = n < 0 ? 0 : (n > q.gp_len ? q.gp_len : n);
            const bool formed = uni(classify_tree(tt, tv, n, false, q.var_len, 1, kMaxStack)) != TREE_BAD;   // (a malformed tree compares with nothing)
            for (unsigned j = st; formed && (long long)j < s; ++j) {
                const unsigned u = uni(q.members[j]);
                const size_t other = (size_t)u * q.gp_len;
                const float *uv = q.value + other;
                const int16_t *ut = q.type + other;
                int m = uni((int)q.size[other]);
                m = m < 0 ? 0 : (m > q.gp_len ? q.gp_len : m);
                // (a) the same live prefix: the same program, the same predictions
                bool same = m == n;
                for (int base = 0; base < n && same; base += kWave) {
                    const int i = base + lane;
                    bool diff = false;
                    if (i < n) diff = f2bits(tv[i]) != f2bits(uv[i]) || tt[i] != ut[i];
                    same = !__any(diff);
                }
                if (!same) {
                    if (uni(classify_tree(ut, uv, m, false, q.var_len, 1, kMaxStack)) == TREE_BAD) continue;
                    // (b), (c) both trees on chunks of 64 rows, out at the first chunk with a differing key
                    same = true;
                    for (long long base = 0; base < q.D && same; base += kWave) {
                        const long long d = base + lane;
                        const bool valid = d < q.D;
                        const float *xr = q.X + (valid ? (size_t)d : (size_t)q.D - 1) * q.var_len;
                        const uint32_t ka = sem_key(run_general<false>(tt, tv, n, xr, q.var_len, 1, outs, stk));
                        const uint32_t kb = sem_key(run_general<false>(ut, uv, m, xr, q.var_len, 1, outs, stk));
                        same = !__any(valid && ka != kb);
                    }
                }
                if (same) { rep = u; break; }
            }
        }
        if (lane == 0) q.class_id[t] = (int)rep;
    }
}

template <int VL, bool LEAN>
static hipError_t launch_semantic(SemParams p, hipStream_t stream) {
    auto kern = sr_semantic_kernel<VL, LEAN>;
    const DeviceInfo &dev = device_info();
    p.ntiles = (int)(((long long)p.D + kWave * kSemK - 1) / (kWave * kSemK));
    const int W = p.ntiles < kSemWaves ? p.ntiles : kSemWaves;
    static int per_cu_cache[kSemWaves + 1] = {0};   // occupancy per block size of THIS instantiation
    int per_cu = per_cu_cache[W];
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, W * 64, 0);
        if (e != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        per_cu_cache[W] = per_cu;
    }
    long blocks = (long)dev.num_cus * per_cu;
    long batch = p.pop / (blocks * 16);   // ~16 batches per workgroup: a short tail, rare atomics
    batch = batch < 4 ? 4 : (batch > kMaxBatch ? kMaxBatch : batch);
    p.batch = (int)batch;
    const long need = (p.pop + batch - 1) / batch;
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(W * 64), 0, stream, p);
    return hipGetLastError();
}

static int semantic_badarg(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    return out_len != 1 ? EVOGP_E_UNSUPPORTED : EVOGP_OK;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_semantic_hash_workspace_bytes(unsigned pop_size, unsigned long long *bytes) {
    if (pop_size == 0 || pop_size > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    a.take<unsigned char>(pop_size);
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_semantic_hash(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                          const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                          unsigned long long *sig_out, void *workspace, evogp_stream_t stream_) {
    if (const int rc = semantic_badarg(pop_size, data_points, gp_len, var_len, out_len)) return rc;
    if (!value || !type || !size || !variables || !sig_out || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const DeviceInfo &dev = device_info();
    hipError_t e;
    Arena a{(char *)workspace};
    SemParams p{};
    p.mark = a.take<unsigned char>(pop_size);
    p.counter = acquire_counter(stream, &e);
    if (!p.counter) return (int)e;
    p.value = value; p.type = type; p.size = size; p.X = variables; p.sig = sig_out;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len;
    const bool regs = p.var_len <= 32;
    if (regs) {
        e = p.var_len <= 12 ? launch_semantic<12, true>(p, stream) : launch_semantic<32, true>(p, stream);
        if (e != hipSuccess) return (int)e;
        e = p.var_len <= 12 ? launch_semantic<12, false>(p, stream) : launch_semantic<32, false>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    long blocks = (long)dev.num_cus * (regs ? 4 : 16);
    if (blocks > p.pop) blocks = p.pop;
    hipLaunchKernelGGL(sr_semantic_general_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, p, regs ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_semantic_classes_workspace_bytes(unsigned pop_size, unsigned long long *bytes) {
    return evogp_hip_tree_classes_workspace_bytes(pop_size, bytes);   // stages 1-3 are its; stage 4 needs nothing more
}

extern "C" int evogp_hip_sr_semantic_classes(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                             const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                             const unsigned long long *hash_in, int *class_id_out, void *workspace, evogp_stream_t stream_) {
    if (const int rc = semantic_badarg(pop_size, data_points, gp_len, var_len, out_len)) return rc;
    if (!value || !type || !size || !variables || !hash_in || !class_id_out || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    SemClassParams q{};
    const hipError_t e = dedup_sorted_runs(hash_in, pop_size, workspace, &q.members, &q.seg, stream);
    if (e != hipSuccess) return (int)e;
    q.value = value; q.type = type; q.size = size; q.X = variables; q.class_id = class_id_out;
    q.pop = (int)pop_size; q.D = (int)data_points; q.gp_len = (int)gp_len; q.var_len = (int)var_len;
    long blocks = (long)device_info().num_cus * 16;
    if (blocks > q.pop) blocks = q.pop;
    hipLaunchKernelGGL(sr_semantic_classes_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, q);
    return (int)hipGetLastError();
}
