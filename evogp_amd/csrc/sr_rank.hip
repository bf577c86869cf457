// sr_rank.hip — rank statistics of single-output SR trees: Spearman correlation and ROC-AUC from a sort per tree and row segment inside
// the evaluation kernel (gfx950; no counterpart in the reference).  include/evogp_hip.h has the contract, DESIGN 3.30 the reasoning.
//
// The rows are cut into G contiguous segments of 1 <= n_g <= 8192 rows.  The key of a prediction is the order-preserving u32 of its
// float32 bits (-0.0 as +0.0); within a segment R2_d = #{k_e < k_d} + #{k_e <= k_d} + 1 is its doubled mid-rank.  Per (tree, segment)
//     S1 = sum R2_d q_d      S2 = sum R2_d^2          (q the caller's payload, 0 .. 16384)
// are exact integers; sr_rank_formula.hpp turns them into the segment's Spearman or AUC score, added per tree in ascending segment order.
//
//   1. rank_rows_kernel        one workgroup per segment: mid-ranks of a float vector (the labels of a Spearman payload), scattered back
//                              to the rows' places, and Q = sum q, Q2 = sum q^2 of a payload
//   2. sr_rank_kernel          sr_scale.hip's decomposition with a sort in the epilogue.  A workgroup of 4 waves pulls batches of trees
//                              from a counter and walks the segments in ascending order.  Every wave interprets a tree on its own row
//                              tiles (run_chunk) and stores key and payload of each row into an LDS segment buffer (u32 keys, u16
//                              payloads: 6 bytes a row).  LARGE = false (every n_g <= 1024): four trees go into four buffers, then wave w
//                              sorts buffer w ALONE, 16 elements per lane, no barrier inside.  LARGE = true: one buffer of 8192 rows
//                              sorted by the whole workgroup, a barrier only where the stride crosses waves
//   3. sr_rank_general_kernel  one workgroup per tree on the scratch-stack interpreter (run_general): the trees kernel 2 marked too deep,
//                              and every tree with var_len > 32; the same buffer, sorter and epilogue
// The sorter is a bitonic network over T x E elements, element r of thread t at position t * E + r: the steps whose partner is one of a
// lane's own E elements run in registers, the steps between lanes go through ds_bpermute, the steps between waves through the LDS
// buffer.  A segment that is shorter than the network is padded with a key above every real key; padding takes no part in any sum.
// Run heads of the sorted keys are joined by a max scan (run start i) and a reverse min scan (run end j): R2 = i + j + 1.
// No atomics but the batch counter, no float reduction but a tree's segment sum; nothing synchronises with the host.
#include "interp.hpp"
#include "launch.hpp"
#include "sr_params.hpp"
#include "sr_rank_formula.hpp"

namespace evogp {

constexpr int kRankK = 4;           // rows per lane of a row tile
constexpr int kRankDepth = 16;      // register stack entries; deeper trees go to the scratch stack
constexpr int kRankWaves = 4;       // waves per workgroup
constexpr int kRankThreads = kRankWaves * 64;
constexpr int kRankTile = kWave * kRankK;
constexpr int kRankSmall = 1024;    // rows of a buffer of the LARGE = false build (one wave x 16 elements per lane)
constexpr int kRankLarge = EVOGP_RANK_MAX_SEGMENT;   // rows of the buffer of the LARGE = true build (4 waves x 32 elements per lane)
constexpr unsigned char kRankNone = 0, kRankDeep = 1, kRankHeavy = 2;
constexpr unsigned long long kRankPad = 0xFFFFFFFFull << 16;   // key 0xFFFFFFFF (no real key: it is the image of a NaN), payload 0

struct RankParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;            // [D][var_len]
    const int *q;              // [D] payload
    const int *seg;            // [G + 1]
    const long long *consts;   // [G][2]: Q, Q2 (rank_rows_kernel on the payload alone)
    long long *words;          // [pop][G][2] or nullptr
    double *fused;             // [pop][3] or nullptr
    double *scores;            // [pop][G] or nullptr: NaN where the segment's score is undefined
    unsigned char *status;     // [pop]
    unsigned char *mark;       // [pop]: kRankDeep "take me in the general kernel", kRankHeavy "take me in the FULL register kernel"
    unsigned *counter;         // as sr_scale.hip: [0] LEAN batch counter, [1] some tree is marked deep, [2] some is marked heavy, [3] FULL batch counter
    int pop, D, G, gp_len, var_len, batch, metric;
};

__device__ inline uint32_t rank_key(float v) {
    uint32_t u = f2bits(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the rows [s0, s0 + n) of segment g, clamped to the dataset and to `cap` rows: no index leaves the arrays whatever seg holds
__device__ inline void rank_segment(const int *seg, int g, int D, int cap, int *s0, int *n) {
    int a = uni(seg[g]), b = uni(seg[g + 1]);
    a = a < 0 ? 0 : (a > D ? D : a);
    b = b < a ? a : (b > D ? D : b);
    *s0 = a;
    *n = b - a > cap ? cap : b - a;
}

// ---- the sorter ----------------------------------------------------------------------------------------------------------------------
// An element is key << 16 | payload.  ties in the key are broken by the payload: a run of equal keys stays one run.
__device__ inline void rank_cx(unsigned long long &a, unsigned long long &b, bool asc) {
    const bool sw = (a > b) == asc;
    const unsigned long long lo = sw ? b : a, hi = sw ? a : b;
    a = lo; b = hi;
}

// WAVES == 1: the calling wave alone, T = 64, no barrier.  WAVES == 4: the whole workgroup, T = 256; every thread must call.
// kb / pb: the buffer (>= T * E entries when WAVES > 1: the steps between waves go through it), rows [0, n) filled.
// f(r2, payload) is called once for every real element by the thread that holds it after the sort.
template <int E, int WAVES, class F>
__device__ inline void rank_buffer_e(uint32_t *kb, uint16_t *pb, int n, unsigned (*xs)[4], F &&f) {
    constexpr int T = WAVES * 64, N = T * E;
    const int lane = threadIdx.x & 63;
    const int tid = WAVES == 1 ? lane : (int)threadIdx.x;
    const int w = WAVES == 1 ? 0 : uni((int)(threadIdx.x >> 6));
    unsigned long long e[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {   // (any assignment of rows to threads will do before the sort: striped, free of bank conflicts)
        const int i = r * T + tid;
        e[r] = i < n ? ((unsigned long long)kb[i] << 16) | pb[i] : kRankPad;
    }
    // stages k <= E: in registers; at k == E the direction is the thread's
#pragma unroll
    for (int k = 2; k <= E; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int r = 0; r < E; ++r) {
                if ((r ^ j) > r) rank_cx(e[r], e[r ^ j], ((tid * E + r) & k) == 0);
            }
        }
    }
    // stages k > E: the strides >= E between threads (partner thread tid ^ m, same r), then the strides < E in registers
    for (int k = 2 * E; k <= N; k <<= 1) {
        const bool asc = ((tid * E) & k) == 0;
        for (int m = k / (2 * E); m >= 1; m >>= 1) {
            const bool keep_min = ((tid & m) == 0) == asc;
            if (WAVES > 1 && m >= 64) {
                __syncthreads();   // (every thread has read what it needs of the buffer)
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    kb[r * T + tid] = (uint32_t)(e[r] >> 16);
                    pb[r * T + tid] = (uint16_t)e[r];
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    const int i = r * T + (tid ^ m);
                    const unsigned long long o = ((unsigned long long)kb[i] << 16) | pb[i];
                    e[r] = (o < e[r]) == keep_min ? o : e[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)e[r], m, 64);
                    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(e[r] >> 32), m, 64);
                    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
                    e[r] = (o < e[r]) == keep_min ? o : e[r];
                }
            }
        }
#pragma unroll
        for (int j = E >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int r = 0; r < E; ++r) {
                if ((r ^ j) > r) rank_cx(e[r], e[r ^ j], asc);
            }
        }
    }
    // ---- sorted: position p0 + r.  Run heads, run start by a max scan, run end by a reverse min scan ----
    const int p0 = tid * E;
    const uint32_t last = (uint32_t)(e[E - 1] >> 16);
    uint32_t kprev = (uint32_t)__shfl_up((int)last, 1, 64);
    if (WAVES > 1) {
        if (lane == 63) xs[w][0] = last;
        __syncthreads();
        if (lane == 0 && w > 0) kprev = xs[w - 1][0];
    }
    int start[E];
    int s = -1, first = 0x7FFFFFFF;
    {
        uint32_t kp = kprev;
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const uint32_t kr = (uint32_t)(e[r] >> 16);
            const bool head = (r == 0 && tid == 0) || kr != kp;
            if (head) {
                s = p0 + r;
                first = first < s ? first : s;
            }
            start[r] = s;
            kp = kr;
        }
    }
    int vmax = s, vmin = first;
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(vmax, o, 64), b = __shfl_down(vmin, o, 64);
        if (lane >= o) vmax = vmax > a ? vmax : a;
        if (lane + o < 64) vmin = vmin < b ? vmin : b;
    }
    int cmax = __shfl_up(vmax, 1, 64), cmin = __shfl_down(vmin, 1, 64);
    if (lane == 0) cmax = -1;
    if (lane == 63) cmin = 0x7FFFFFFF;
    if (WAVES > 1) {
        if (lane == 63) xs[w][1] = (unsigned)vmax;
        if (lane == 0) xs[w][2] = (unsigned)vmin;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < WAVES; ++i) {
            const int a = (int)xs[i][1], b = (int)xs[i][2];
            if (i < w) cmax = cmax > a ? cmax : a;
            if (i > w) cmin = cmin < b ? cmin : b;
        }
    }
    cmin = cmin < n ? cmin : n;
    int nxt = cmin;   // the next run head behind position p0 + r
#pragma unroll
    for (int r = E - 1; r >= 0; --r) {
        const int i = start[r] > cmax ? start[r] : cmax;
        if (p0 + r < n) f(i + nxt + 1, (int)(e[r] & 0xFFFFu));
        if (start[r] == p0 + r) nxt = p0 + r;
    }
}

template <int WAVES, class F>
__device__ inline void rank_buffer(uint32_t *kb, uint16_t *pb, int n, unsigned (*xs)[4], F &&f) {
    if (WAVES == 1) {
        if (n <= 256) rank_buffer_e<4, 1>(kb, pb, n, xs, f);
        else rank_buffer_e<16, 1>(kb, pb, n, xs, f);
    } else {
        if (n <= 2048) rank_buffer_e<8, WAVES>(kb, pb, n, xs, f);
        else if (n <= 4096) rank_buffer_e<16, WAVES>(kb, pb, n, xs, f);
        else rank_buffer_e<32, WAVES>(kb, pb, n, xs, f);
    }
}

// sum of a per-thread pair over the workgroup: every thread calls; the result is exact in every thread
__device__ inline void rank_block_sum(unsigned long long &a, unsigned long long &b, unsigned long long (*ws)[2]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    a = wave_sum_u64(a);
    b = wave_sum_u64(b);
    __syncthreads();
    if (lane == 0) { ws[w][0] = a; ws[w][1] = b; }
    __syncthreads();
    a = ws[0][0] + ws[1][0] + ws[2][0] + ws[3][0];
    b = ws[0][1] + ws[1][1] + ws[2][1] + ws[3][1];
}

// ---- 1. mid-ranks of a vector within its segments, and the constants of a payload ---------------------------------------------------------
__global__ __launch_bounds__(kRankThreads) void rank_rows_kernel(const float *values, const int *payload, const int *seg, int D, int *r2_out,
                                                                 long long *consts, int *status) {
    __shared__ uint32_t key_s[kRankLarge];
    __shared__ uint16_t pay_s[kRankLarge];
    __shared__ unsigned xs[kRankWaves][4];
    __shared__ unsigned long long ws[kRankWaves][2];
    const int g = blockIdx.x;
    int s0, n;
    rank_segment(seg, g, D, kRankLarge, &s0, &n);
    unsigned long long q1 = 0, q2 = 0;
    int bad = 0;
    if (values) {
        for (int off = threadIdx.x; off < n; off += kRankThreads) {
            const float v = values[s0 + off];
            bad |= v != v ? 1 : 0;
            key_s[off] = rank_key(v);
            pay_s[off] = (uint16_t)off;
        }
        bad = __syncthreads_or(bad);
        if (!bad) {
            rank_buffer<kRankWaves>(key_s, pay_s, n, xs, [&](int r2, int off) {
                if (r2_out) r2_out[s0 + off] = r2;
                q1 += (unsigned long long)r2;
                q2 += (unsigned long long)r2 * (unsigned long long)r2;
            });
        } else if (r2_out) {
            for (int off = threadIdx.x; off < n; off += kRankThreads) r2_out[s0 + off] = 0;
        }
    }
    if (payload) {
        q1 = q2 = 0;
        for (int off = threadIdx.x; off < n; off += kRankThreads) {
            const unsigned long long v = (unsigned long long)(long long)payload[s0 + off];
            q1 += v;
            q2 += v * v;
        }
    }
    rank_block_sum(q1, q2, ws);
    if (threadIdx.x == 0) {
        if (consts) { consts[2 * (size_t)g] = (long long)q1; consts[2 * (size_t)g + 1] = (long long)q2; }
        if (status) status[g] = bad ? 1 : 0;
    }
}

// ---- the epilogue of one (tree, segment): the words, and the tree's fused sums in the thread that keeps them --------------------------------
struct RankSums {
    double s, ss;
    int count;
};
__device__ inline void rank_store(const RankParams &p, int t, int g, int n, unsigned long long S1, unsigned long long S2, RankSums &acc) {
    if (p.words) {
        long long *out = p.words + ((size_t)t * p.G + g) * 2;
        out[0] = (long long)S1;
        out[1] = (long long)S2;
    }
    if (p.fused || p.scores) {
        double sc = __builtin_nan("");
        if (rank_segment_score(p.metric, n, (long long)S1, (long long)S2, p.consts[2 * (size_t)g], p.consts[2 * (size_t)g + 1], &sc)) {
            acc.s = __dadd_rn(acc.s, sc);
            acc.ss = __dadd_rn(acc.ss, __dmul_rn(sc, sc));
            acc.count += 1;
        }
        if (p.scores) p.scores[(size_t)t * p.G + g] = sc;
    }
}
// a segment without rows (a seg_start the contract excludes): words 0, no score
__device__ inline void rank_store_empty(const RankParams &p, int t, int g) {
    if (p.words) p.words[((size_t)t * p.G + g) * 2] = p.words[((size_t)t * p.G + g) * 2 + 1] = 0;
    if (p.scores) p.scores[(size_t)t * p.G + g] = __builtin_nan("");
}
// every word of an unusable tree is 0, every score NaN: the whole workgroup writes
__device__ inline void rank_clear(const RankParams &p, int t) {
    if (p.words)
        for (int j = threadIdx.x; j < 2 * p.G; j += kRankThreads) p.words[(size_t)t * p.G * 2 + j] = 0;
    if (p.scores)
        for (int j = threadIdx.x; j < p.G; j += kRankThreads) p.scores[(size_t)t * p.G + j] = __builtin_nan("");
}
__device__ inline void rank_finish(const RankParams &p, int t, bool unusable, const RankSums &acc) {
    p.status[t] = unusable ? 1 : 0;
    if (p.fused) {
        const double nan = __builtin_nan("");
        double *out = p.fused + 3 * (size_t)t;
        out[0] = unusable ? nan : acc.s;
        out[1] = unusable ? nan : acc.ss;
        out[2] = unusable ? nan : (double)acc.count;
    }
}

// ---- 2. the register interpreter -------------------------------------------------------------------------------------------------------
// Two resident waves per SIMD for the small LEAN build only: the FULL build (29 functions) needs more than 256 registers next to the sort's
// 16 elements per lane and would spill to scratch at two; at one wave it keeps them in AGPRs (profiles/rank_resources.txt).
template <int VL, bool LEAN, bool LARGE>
__global__ __launch_bounds__(kRankThreads, LARGE || VL > 16 || !LEAN ? 1 : 2) void sr_rank_kernel(RankParams p) {
    constexpr int K = kRankK, DEPTH = kRankDepth, TILE = kRankTile, W = kRankWaves;
    constexpr int NT = LARGE ? 1 : W;                   // trees interpreted back to back before a sort
    constexpr int CAP = LARGE ? kRankLarge : kRankSmall;
    __shared__ uint32_t key_s[NT * CAP];
    __shared__ uint16_t pay_s[NT * CAP];
    __shared__ unsigned xs[W][4];
    __shared__ unsigned long long word_s[W][2];   // LARGE: the waves' partial sums; else: the words of the group's four trees
    __shared__ int cls_s[kMaxBatch];
    __shared__ int nan_s[kMaxBatch];              // != 0: a prediction of the tree was a NaN: no more work on it
    __shared__ unsigned next_s;

    if (!LEAN && uni((int)p.counter[2]) == 0) return;   // the LEAN pass marked nothing
    unsigned *const batches = p.counter + (LEAN ? 0 : 3);
    using VARS = typename VecOf<VL>::type;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int batch = p.batch;

    VARS vars[K];
    int qv[K], pos[K];
    bool valid[K];
    auto load_tile = [&](int s0, int n, int tile) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int first = tile * TILE;
            const int rows = n - first < TILE ? n - first : TILE;   // rows of this tile, >= 1
            const int off = k * kWave + lane;
            valid[k] = off < rows;
            pos[k] = first + off;
            const size_t dc = (size_t)s0 + (size_t)(first + (valid[k] ? off : rows - 1));   // lanes past the end repeat the last row: no new NaN
            const float *xr = p.X + dc * p.var_len;
#pragma unroll
            for (int v = 0; v < VL; ++v) vars[k][v] = v < p.var_len ? xr[v] : 0.0f;
            qv[k] = p.q[dc];
        }
    };
    int loaded = -1;   // the segment whose tile `w` sits in the registers

    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) next_s = atomicAdd(batches, (unsigned)batch);
        __syncthreads();
        const unsigned next = uni(next_s);
        if (next >= (unsigned)p.pop) break;
        const int t0 = (int)next;
        const int nb = p.pop - t0 < batch ? p.pop - t0 : batch;

        // ---- classify the batch, trees split between the waves ----
        for (int b = w; b < nb; b += W) {
            const size_t row = (size_t)(t0 + b) * p.gp_len;
            int len = uni((int)p.size[row]);
            len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
            int c = TREE_SKIP;   // (FULL pass: not marked for it)
            if (LEAN || uni((int)p.mark[t0 + b]) == kRankHeavy)
                c = classify_tree(p.type + row, p.value + row, len, false, p.var_len, 1, DEPTH, LEAN ? 1 : 0);
            if (lane == 0) { cls_s[b] = c; nan_s[b] = 0; }
        }
        __syncthreads();

        RankSums acc{0.0, 0.0, 0};   // of tree t0 + threadIdx.x, added in segment order
        for (int g = 0; g < p.G; ++g) {
            int s0, n;
            rank_segment(p.seg, g, p.D, CAP, &s0, &n);
            if (n <= 0) {
                if ((int)threadIdx.x < nb && cls_s[threadIdx.x] == TREE_OK) rank_store_empty(p, t0 + threadIdx.x, g);
                continue;
            }
            const int ntiles = (n + TILE - 1) / TILE;
            const bool single = ntiles <= W;   // every wave owns one tile of the segment: loaded once for the whole batch
            if (single && loaded != g) {
                load_tile(s0, n, w < ntiles ? w : 0);
                loaded = g;
            }
            for (int b0 = 0; b0 < nb; b0 += NT) {
                // ---- every wave interprets the group's trees on its own tiles: keys and payloads into the buffers ----
                for (int u = 0; u < NT; ++u) {
                    const int b = b0 + u;
                    // (nan_s[b] is read here while another wave, ahead in this same phase, may raise it: an unsynchronised LDS read, and either
                    // outcome is right -- a wave that goes on fills a buffer nobody sorts, the flag is settled at the barrier below)
                    if (b >= nb || uni(cls_s[b]) != TREE_OK || uni(nan_s[b]) != 0) continue;
                    const size_t row = (size_t)(t0 + b) * p.gp_len;
                    const float *tv = p.value + row;
                    const int16_t *tt = p.type + row;
                    int len = uni((int)p.size[row]);
                    len = len > p.gp_len ? p.gp_len : len;
                    uint32_t *kb = key_s + u * CAP;
                    uint16_t *pb = pay_s + u * CAP;
                    bool bad = false;
                    for (int tile = w; tile < ntiles; tile += W) {
                        if (!single) { load_tile(s0, n, tile); loaded = -1; }
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
                            const int cn = len - base < kWave ? len - base : kWave;
                            run_chunk<false, LEAN, K, DEPTH>(opv, payv, cn, st, RegVars<VL, K>{vars}, outs);
                        }
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const float pr = st.tos[k];
                            bad |= pr != pr;
                            if (valid[k]) {
                                kb[pos[k]] = rank_key(pr);
                                pb[pos[k]] = (uint16_t)qv[k];
                            }
                        }
                    }
                    if (__any(bad) != 0 && lane == 0) nan_s[b] = 1;
                }
                __syncthreads();

                // ---- the sort: wave w takes buffer w alone (LARGE: the workgroup takes the one buffer) ----
                {
                    const int b = LARGE ? b0 : b0 + w;
                    if (b < nb && uni(cls_s[b]) == TREE_OK && uni(nan_s[b]) == 0) {
                        unsigned long long S1 = 0, S2 = 0;
                        rank_buffer<LARGE ? W : 1>(key_s + (LARGE ? 0 : w * CAP), pay_s + (LARGE ? 0 : w * CAP), n, xs, [&](int r2, int q) {
                            S1 += (unsigned long long)(r2 * q);
                            S2 += (unsigned long long)(r2 * r2);
                        });
                        S1 = wave_sum_u64(S1);
                        S2 = wave_sum_u64(S2);
                        if (lane == 0) { word_s[w][0] = S1; word_s[w][1] = S2; }
                    }
                }
                __syncthreads();

                // ---- one thread per tree: the words, and the segment's score into the tree's sums ----
                {
                    const int b = threadIdx.x;
                    if (b >= b0 && b < b0 + NT && b < nb && cls_s[b] == TREE_OK && nan_s[b] == 0) {
                        unsigned long long S1, S2;
                        if (LARGE) {
                            S1 = word_s[0][0] + word_s[1][0] + word_s[2][0] + word_s[3][0];
                            S2 = word_s[0][1] + word_s[1][1] + word_s[2][1] + word_s[3][1];
                        } else {
                            S1 = word_s[b - b0][0];
                            S2 = word_s[b - b0][1];
                        }
                        rank_store(p, t0 + b, g, n, S1, S2, acc);
                    }
                }
            }
        }
        __syncthreads();

        // ---- one thread per tree: status and fused sums, or the mark for the kernel that takes the tree ----
        if ((int)threadIdx.x < nb) {
            const int b = threadIdx.x, t = t0 + b;
            const int c = cls_s[b];
            if (c == TREE_OK || c == TREE_BAD) {
                if (c == TREE_BAD) nan_s[b] = 1;
                rank_finish(p, t, nan_s[b] != 0, acc);
                p.mark[t] = kRankNone;
            } else if (c != TREE_SKIP) {
                p.mark[t] = c == TREE_DEEP ? kRankDeep : kRankHeavy;
                p.counter[c == TREE_DEEP ? 1 : 2] = 1u;
            }
        }
        __syncthreads();
        // ---- the words of an unusable tree are 0 in every segment ----
        for (int b = 0; b < nb; ++b) {
            const int c = uni(cls_s[b]);
            if ((c == TREE_OK || c == TREE_BAD) && uni(nan_s[b]) != 0) rank_clear(p, t0 + b);
        }
    }
}

// ---- 3. the scratch-stack interpreter: one workgroup per tree, threads are rows ------------------------------------------------------------
__global__ __launch_bounds__(kRankThreads) void sr_rank_general_kernel(RankParams p, int only_marked) {
    __shared__ uint32_t key_s[kRankLarge];
    __shared__ uint16_t pay_s[kRankLarge];
    __shared__ unsigned xs[kRankWaves][4];
    __shared__ unsigned long long ws[kRankWaves][2];
    if (only_marked && uni((int)p.counter[1]) == 0) return;   // no tree was too deep for the register stack
    float stk[kMaxStack + 2];
    float outs[1];
    for (long long tl = blockIdx.x; tl < p.pop; tl += gridDim.x) {
        const int t = (int)tl;
        if (only_marked && uni((int)p.mark[t]) != kRankDeep) continue;
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *tt = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int cls = uni(classify_tree(tt, tv, len, false, p.var_len, 1, kMaxStack));
        bool unusable = cls != TREE_OK;
        RankSums acc{0.0, 0.0, 0};
        for (int g = 0; g < p.G && !unusable; ++g) {
            int s0, n;
            rank_segment(p.seg, g, p.D, kRankLarge, &s0, &n);
            if (n <= 0) {
                if (threadIdx.x == 0) rank_store_empty(p, t, g);
                continue;
            }
            int bad = 0;
            __syncthreads();   // (the buffer's last readers are done)
            for (int base = 0; base < n; base += kRankThreads) {
                const int off = base + (int)threadIdx.x;
                const size_t dc = (size_t)s0 + (size_t)(off < n ? off : n - 1);
                const float pr = run_general<false>(tt, tv, len, p.X + dc * p.var_len, p.var_len, 1, outs, stk);
                bad |= pr != pr ? 1 : 0;
                if (off < n) {
                    key_s[off] = rank_key(pr);
                    pay_s[off] = (uint16_t)p.q[dc];
                }
            }
            if (__syncthreads_or(bad)) {
                unusable = true;
                break;
            }
            unsigned long long S1 = 0, S2 = 0;
            rank_buffer<kRankWaves>(key_s, pay_s, n, xs, [&](int r2, int q) {
                S1 += (unsigned long long)(r2 * q);
                S2 += (unsigned long long)(r2 * r2);
            });
            rank_block_sum(S1, S2, ws);
            if (threadIdx.x == 0) rank_store(p, t, g, n, S1, S2, acc);
        }
        if (threadIdx.x == 0) rank_finish(p, t, unusable, acc);
        if (unusable) {
            __syncthreads();   // (behind thread 0's words of the segments before the NaN)
            rank_clear(p, t);
        }
    }
}

template <int VL, bool LEAN, bool LARGE>
static hipError_t launch_rank(RankParams p, hipStream_t stream) {
    auto kern = sr_rank_kernel<VL, LEAN, LARGE>;
    const DeviceInfo &dev = device_info();
    static int per_cu = 0;   // occupancy of THIS instantiation
    if (per_cu == 0) {
        int v = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kern, kRankThreads, 0);
        if (e != hipSuccess) return e;
        per_cu = v < 1 ? 1 : v;
    }
    long blocks = (long)dev.num_cus * per_cu;
    long batch = p.pop / (blocks * 16);   // ~16 batches per workgroup: a short tail, rare atomics
    batch = batch < 4 ? 4 : (batch > kMaxBatch ? kMaxBatch : batch);
    p.batch = (int)batch;
    const long need = (p.pop + batch - 1) / batch;
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kRankThreads), 0, stream, p);
    return hipGetLastError();
}

template <int VL, bool LARGE>
static hipError_t launch_rank_pair(const RankParams &p, hipStream_t stream) {
    hipError_t e = launch_rank<VL, true, LARGE>(p, stream);
    if (e != hipSuccess) return e;
    return launch_rank<VL, false, LARGE>(p, stream);
}

static int rank_badarg(unsigned data_points, unsigned n_segments, unsigned max_segment) {
    if (data_points == 0 || n_segments == 0 || max_segment == 0 || data_points > 0x7FFFFFFFu || n_segments > data_points ||
        max_segment > (unsigned)kRankLarge || max_segment > data_points)
        return EVOGP_E_BADARG;
    return EVOGP_OK;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_rank_rows(unsigned data_points, unsigned n_segments, unsigned max_segment, const float *values, const int *payload,
                                   const int *seg_start, int *r2_out, long long *consts_out, int *status_out, evogp_stream_t stream_) {
    if (const int rc = rank_badarg(data_points, n_segments, max_segment)) return rc;
    if (!seg_start || (!values && !payload) || (values && !status_out)) return EVOGP_E_NULLPTR;
    hipLaunchKernelGGL(rank_rows_kernel, dim3(n_segments), dim3(kRankThreads), 0, (hipStream_t)stream_, values, payload, seg_start,
                       (int)data_points, r2_out, consts_out, status_out);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_sr_rank_stats_workspace_bytes(unsigned pop_size, unsigned n_segments, unsigned long long *bytes) {
    if (pop_size == 0 || n_segments == 0 || pop_size > 0x7FFFFFFFu || n_segments > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    a.take<unsigned char>(pop_size);
    a.take<long long>(2 * (size_t)n_segments);
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_rank_stats(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned n_segments,
                                       unsigned max_segment, const float *value, const int16_t *type, const int16_t *size,
                                       const float *variables, const int *payload, const int *seg_start, int metric, long long *words_out,
                                       double *fused_out, double *scores_out, unsigned char *status_out, void *workspace, evogp_stream_t stream_) {
    if (const int rc = rank_badarg(data_points, n_segments, max_segment)) return rc;
    if (pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || pop_size > 0x7FFFFFFFu || var_len > 0x7FFFFFFFu ||
        (metric != kRankSpearman && metric != kRankAuc))
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !payload || !seg_start || !status_out || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const DeviceInfo &dev = device_info();
    hipError_t e;
    Arena a{(char *)workspace};
    RankParams p{};
    p.mark = a.take<unsigned char>(pop_size);
    long long *consts = a.take<long long>(2 * (size_t)n_segments);
    p.consts = consts;
    p.counter = acquire_counter(stream, &e);
    if (!p.counter) return (int)e;
    p.value = value; p.type = type; p.size = size; p.X = variables; p.q = payload; p.seg = seg_start;
    p.words = words_out; p.fused = fused_out; p.scores = scores_out; p.status = status_out;
    p.pop = (int)pop_size; p.D = (int)data_points; p.G = (int)n_segments; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.metric = metric;
    hipLaunchKernelGGL(rank_rows_kernel, dim3(n_segments), dim3(kRankThreads), 0, stream, (const float *)nullptr, payload, seg_start, p.D,
                       (int *)nullptr, consts, (int *)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const bool regs = p.var_len <= 32;
    const bool large = max_segment > (unsigned)kRankSmall;
    if (regs) {
        if (p.var_len <= 12) e = large ? launch_rank_pair<12, true>(p, stream) : launch_rank_pair<12, false>(p, stream);
        else e = large ? launch_rank_pair<32, true>(p, stream) : launch_rank_pair<32, false>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    long blocks = (long)dev.num_cus * (regs ? 2 : 4);
    if (blocks > p.pop) blocks = p.pop;
    hipLaunchKernelGGL(sr_rank_general_kernel, dim3((unsigned)blocks), dim3(kRankThreads), 0, stream, p, regs ? 1 : 0);
    return (int)hipGetLastError();
}
