// nsga2.hip — Pareto ranking of a population on (error, complexity) and NSGA-II parent selection (gfx950; no counterpart in the
// reference).  include/evogp_hip.h has the contract of evogp_hip_pareto_rank / evogp_hip_nsga2_select; tests/nsga2_ref.py restates it.
//
// evogp_hip_pareto_rank, all on the caller's stream, nothing synchronises with the host, the launch count is fixed:
//   1. keys      one thread per tree: the order-preserving integer image of key(err), 0xFFFFFFFF for an unranked tree; a stable radix
//                sort (rocPRIM) gives the key order, a max-scan of the head positions the FIRST position of every run of equal keys
//   2. buckets   a second stable sort, by cx (17 bits; unranked trees in a bucket of their own behind the others): every bucket is in
//                ascending key order, clones next to each other.  Head marks of the groups of equal key inside a bucket, a plus-scan
//                numbers the groups, the last tree of a bucket records where the bucket ends
//   3. fronts    ONE workgroup walks the buckets in ascending cx (the dependent chain stays inside it: no grid barrier, no launch per
//                bucket).  T is a Fenwick tree for prefix maxima over the key-order positions: T answers "the largest front among the
//                processed trees with key <= mine" in <= log2(pop) loads.  Per bucket: every tree queries a = T(first position of its
//                key), group i takes front_i = i + max over i' <= i of (a_i' + 1 - i') (a block-wide inclusive max-scan with a carry
//                between chunks), and once ALL queries of the bucket are answered the group heads raise T with integer atomic maxima
//                (order-independent, so the result is deterministic).  O(n_c log pop) work per bucket of n_c trees.
//   4. crowding  a sort by (front, cx): trees with equal (front, cx) are one point (of two trees of equal cx the one with the smaller
//                key dominates the other), its first tree the representative.  Points numbered by a scan; the first and last point
//                of every front recorded by the trees at the front's boundaries; Deb's distance in plain float32 operations
//   5. order     a sort by (front, ~image(crowding)); all four sorts are stable and start from ascending tree index
#include "evogp_defs.hpp"
#include "group_sort.hpp"
#include "launch.hpp"

namespace evogp {

constexpr unsigned kNsgaRowContender = (1u << 22);    // words 2^22 + k: contender k of tournament i
constexpr unsigned kNsgaUnrankedKey = 0xFFFFFFFFu;    // (the image of a finite key is below 0xFF800000)
constexpr unsigned kNsgaUnrankedCx = 0x10000u;
constexpr int kNsgaUnrankedFront = 0x7FFFFFFF;
constexpr unsigned kNsgaChainThreads = 1024, kNsgaChainItems = 4;

// inclusive max-scan over the 64 lanes (the DPP sequence of wave_scan_incl)
__device__ inline int wave_scan_max_incl(int v) {
    const int lo = (int)0x80000000;
    v = max(v, dpp_move<kDppRowShr | 1, 0xf>(lo, v));
    v = max(v, dpp_move<kDppRowShr | 2, 0xf>(lo, v));
    v = max(v, dpp_move<kDppRowShr | 4, 0xf>(lo, v));
    v = max(v, dpp_move<kDppRowShr | 8, 0xf>(lo, v));
    v = max(v, dpp_move<kDppBcast15, 0xa>(lo, v));
    v = max(v, dpp_move<kDppBcast31, 0xc>(lo, v));
    return v;
}

// ---- 1. keys ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nsga_keys_kernel(const float *err, const int *cx, unsigned pop, unsigned cx_bound, unsigned *key,
                                                        unsigned *tree) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= pop) return;
    const float k = error_key(err[t]);
    const int c = cx[t];
    const bool ranked = k > -__builtin_inff() && k < __builtin_inff() && c >= 0 && (unsigned)c <= cx_bound;
    key[t] = ranked ? float_ord(k) : kNsgaUnrankedKey;
    tree[t] = t;
}

// over the key order s: where a run of equal keys starts (for the max-scan), and the second sort's key and value
__global__ __launch_bounds__(256) void nsga_runs_kernel(const unsigned *key, const unsigned *tree, const int *cx, unsigned pop, unsigned *head_pos,
                                                        unsigned *cx_key, unsigned *pos) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= pop) return;
    const unsigned k = key[s];
    head_pos[s] = (s == 0u || k != key[s - 1u]) ? s : 0u;
    cx_key[s] = k == kNsgaUnrankedKey ? kNsgaUnrankedCx : (unsigned)cx[tree[s]];
    pos[s] = s;
}

// ---- 2. buckets ------------------------------------------------------------------------------------------------------------------
// over the bucket order u: the tree, the first key-order position of its key, the group heads, the bucket ends; unranked trees get
// their front here
__global__ __launch_bounds__(256) void nsga_groups_kernel(const unsigned *c2, const unsigned *s2, const unsigned *seg, const unsigned *tree,
                                                          unsigned pop, unsigned *f2, unsigned *t2, unsigned *head2, unsigned *bend, int *front) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= pop) return;
    const unsigned c = c2[u], s = s2[u], f = seg[s], t = tree[s];
    f2[u] = f;
    t2[u] = t;
    head2[u] = (u == 0u || c2[u - 1u] != c || seg[s2[u - 1u]] != f) ? 1u : 0u;
    if (u + 1u == pop || c2[u + 1u] != c) bend[c] = u + 1u;
    if (c == kNsgaUnrankedCx) front[t] = kNsgaUnrankedFront;
}

// ---- 3. fronts -------------------------------------------------------------------------------------------------------------------
struct NsgaChain {
    const unsigned *c2, *f2, *t2, *gid, *bend;
    int *fen;      // [pop + 1], all -1 on entry: Fenwick tree of prefix maxima, node j covers positions (j - lowbit(j), j]
    int *front_u;  // fronts in bucket order
    int *front;    // fronts by tree
    unsigned pop;
};

// kNsgaChainItems prefix maxima at once: the chains of dependent loads advance together, so their latencies overlap.  f[k] + 1 = 0
// asks for nothing (node 0 is never raised: it stays -1).  Agent-scope loads: the atomic maxima of the earlier buckets live in L2.
__device__ inline void nsga_fen_query(const int *fen, unsigned (&j)[kNsgaChainItems], int (&r)[kNsgaChainItems]) {
    unsigned any = 0;
#pragma unroll
    for (unsigned k = 0; k < kNsgaChainItems; ++k) {
        r[k] = -1;
        any |= j[k];
    }
    while (any) {
        any = 0;
#pragma unroll
        for (unsigned k = 0; k < kNsgaChainItems; ++k) {
            r[k] = max(r[k], __hip_atomic_load(fen + j[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            j[k] &= j[k] - 1u;
            any |= j[k];
        }
    }
}

__device__ inline void nsga_fen_raise(int *fen, unsigned pop, unsigned f, int v) {
    for (unsigned j = f + 1u; j <= pop; j += j & (0u - j)) atomicMax(fen + j, v);
}

__global__ __launch_bounds__(1024) void nsga_chain_kernel(NsgaChain q) {
    __shared__ int s_w[16];
    __shared__ int s_carry;
    constexpr int kLo = (int)0x80000000;
    constexpr unsigned kChunk = kNsgaChainThreads * kNsgaChainItems;
    const unsigned tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    unsigned u0 = 0;
    while (u0 < q.pop) {                       // (every loop bound below is the same for all threads of the workgroup)
        const unsigned c = q.c2[u0];
        if (c >= kNsgaUnrankedCx) break;       // the unranked trees come last
        const unsigned u1 = q.bend[c], g0 = q.gid[u0];
        if (u1 <= u0 || u1 > q.pop) break;     // (cannot happen: bend[c] is behind the last tree of bucket c)
        if (tid == 0) s_carry = kLo;
        __syncthreads();
        // the queries and the scan: thread tid owns kNsgaChainItems consecutive trees of a chunk
        for (unsigned base = u0; base < u1; base += kChunk) {
            int gi[kNsgaChainItems], run[kNsgaChainItems], a[kNsgaChainItems];
            unsigned node[kNsgaChainItems];
            const unsigned first = base + tid * kNsgaChainItems;
#pragma unroll
            for (unsigned k = 0; k < kNsgaChainItems; ++k) {
                const unsigned u = first + k;
                gi[k] = u < u1 ? (int)(q.gid[u] - g0) : 0;
                node[k] = u < u1 ? q.f2[u] + 1u : 0u;
            }
            nsga_fen_query(q.fen, node, a);
#pragma unroll
            for (unsigned k = 0; k < kNsgaChainItems; ++k) a[k] = first + k < u1 ? a[k] + 1 - gi[k] : kLo;
            int m = kLo;
#pragma unroll
            for (unsigned k = 0; k < kNsgaChainItems; ++k) {
                m = max(m, a[k]);
                run[k] = m;
            }
            const int incl = wave_scan_max_incl(m);
            int excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = kLo;
            if (lane == 63u) s_w[w] = incl;
            __syncthreads();
            int before = s_carry, total = s_carry;
#pragma unroll
            for (unsigned k = 0; k < 16u; ++k) {
                const int v = s_w[k];
                total = max(total, v);
                before = k < w ? max(before, v) : before;
            }
            before = max(before, excl);
#pragma unroll
            for (unsigned k = 0; k < kNsgaChainItems; ++k) {
                const unsigned u = first + k;
                if (u < u1) {
                    const int fr = gi[k] + max(before, run[k]);
                    q.front_u[u] = fr;
                    q.front[q.t2[u]] = fr;
                }
            }
            __syncthreads();
            if (tid == 0) s_carry = total;
            __syncthreads();
        }
        // the updates, by the group heads, every thread on the trees it wrote above
        for (unsigned base = u0; base < u1; base += kChunk) {
            const unsigned first = base + tid * kNsgaChainItems;
#pragma unroll
            for (unsigned k = 0; k < kNsgaChainItems; ++k) {
                const unsigned u = first + k;
                if (u < u1 && (u == u0 || q.gid[u] != q.gid[u - 1u])) nsga_fen_raise(q.fen, q.pop, q.f2[u], q.front_u[u]);
            }
        }
        __threadfence();
        __syncthreads();
        u0 = u1;
    }
}

// ---- 4. crowding -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nsga_front_keys_kernel(const int *front, const int *cx, unsigned pop, unsigned long long *key, unsigned *tree) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= pop) return;
    const int fr = front[t];
    key[t] = fr == kNsgaUnrankedFront ? (((unsigned long long)kNsgaUnrankedFront << 17) | 0x1FFFFull)
                                      : (((unsigned long long)(unsigned)fr << 17) | (unsigned long long)(unsigned)cx[t]);
    tree[t] = t;
}

__global__ __launch_bounds__(256) void nsga_point_heads_kernel(const unsigned long long *key, unsigned pop, unsigned *head) {
    const unsigned w = blockIdx.x * 256u + threadIdx.x;
    if (w >= pop) return;
    head[w] = (w == 0u || key[w] != key[w - 1u]) ? 1u : 0u;
}

// over the (front, cx) order w: the points' key and cx, and the first and last point of every front
__global__ __launch_bounds__(256) void nsga_points_kernel(const unsigned long long *key, const unsigned *tree, const unsigned *head, const unsigned *pid,
                                                          const float *err, unsigned pop, float *pt_key, unsigned *pt_cx, unsigned *first_of,
                                                          unsigned *last_of) {
    const unsigned w = blockIdx.x * 256u + threadIdx.x;
    if (w >= pop) return;
    const unsigned long long k = key[w];
    const unsigned fr = (unsigned)(k >> 17);
    if (fr == (unsigned)kNsgaUnrankedFront) return;
    const unsigned p = pid[w] + head[w] - 1u;      // (pid: the heads in front of w)
    if (head[w]) {
        pt_key[p] = error_key(err[tree[w]]);
        pt_cx[p] = (unsigned)(k & 0x1FFFFull);
    }
    if (w == 0u || (unsigned)(key[w - 1u] >> 17) != fr) first_of[fr] = p;
    if (w + 1u == pop || (unsigned)(key[w + 1u] >> 17) != fr) last_of[fr] = p;
}

__global__ __launch_bounds__(256) void nsga_crowding_kernel(const unsigned long long *key, const unsigned *tree, const unsigned *head, const unsigned *pid,
                                                            const float *pt_key, const unsigned *pt_cx, const unsigned *first_of,
                                                            const unsigned *last_of, unsigned pop, float *crowding, unsigned long long *okey,
                                                            unsigned *otree) {
    const unsigned w = blockIdx.x * 256u + threadIdx.x;
    if (w >= pop) return;
    const unsigned fr = (unsigned)(key[w] >> 17), t = tree[w];
    float d = 0.0f;
    if (fr != (unsigned)kNsgaUnrankedFront && head[w]) {
        const unsigned p = pid[w], a = first_of[fr], b = last_of[fr];
        if (p <= a || p >= b) {
            d = __builtin_inff();
        } else {
            const float dc = ((float)pt_cx[p + 1u] - (float)pt_cx[p - 1u]) / ((float)pt_cx[b] - (float)pt_cx[a]);
            const float dk = (pt_key[p - 1u] - pt_key[p + 1u]) / (pt_key[a] - pt_key[b]);
            d = dc + dk;
            if (d != d) d = __builtin_inff();
        }
    }
    crowding[t] = d;
    okey[t] = ((unsigned long long)fr << 32) | (unsigned long long)(~float_ord(d));   // front ascending, then crowding descending
    otree[t] = t;
}

// ---- selection -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nsga_select_kernel(const int *order, unsigned pool, unsigned n, unsigned t_size, unsigned long long base,
                                                          int *winners) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    unsigned best = pool;
    for (unsigned k = 0; k < t_size; ++k) best = min(best, counter_word(base, kNsgaRowContender + k, (unsigned long long)i) % pool);
    winners[i] = order[best];
}

// ---- workspace -------------------------------------------------------------------------------------------------------------------
struct NsgaWorkspace {
    unsigned *k32_a, *k32_b, *v_a, *v_b;
    unsigned long long *k64_a, *k64_b;
    unsigned *head, *scan, *f2, *t2, *gid, *bend;
    int *fen, *front_u;
    float *pt_key;
    unsigned *pt_cx, *first_of, *last_of;
    void *temp;
    size_t temp_bytes;
};

static int g_nsga_stop = 0;

static hipError_t nsga_workspace(unsigned pop, Arena &a, NsgaWorkspace *w) {
    hipError_t e;
    w->temp_bytes = 0;
    if ((e = sort_pairs_u32_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = sort_pairs_u64_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = scan_plus_excl_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = scan_plus_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = scan_max_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    w->k32_a = a.take<unsigned>(pop); w->k32_b = a.take<unsigned>(pop); w->v_a = a.take<unsigned>(pop); w->v_b = a.take<unsigned>(pop);
    w->k64_a = a.take<unsigned long long>(pop); w->k64_b = a.take<unsigned long long>(pop);
    w->head = a.take<unsigned>(pop); w->scan = a.take<unsigned>(pop); w->f2 = a.take<unsigned>(pop); w->t2 = a.take<unsigned>(pop);
    w->gid = a.take<unsigned>(pop);
    w->bend = a.take<unsigned>(kNsgaUnrankedCx + 1u);
    w->fen = a.take<int>((size_t)pop + 1u);
    w->front_u = a.take<int>(pop); w->pt_key = a.take<float>(pop); w->pt_cx = a.take<unsigned>(pop);
    w->first_of = a.take<unsigned>(pop); w->last_of = a.take<unsigned>(pop);
    w->temp = a.take_bytes(w->temp_bytes);
    return hipSuccess;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_pareto_rank_workspace_bytes(unsigned pop, unsigned long long *bytes) {
    if (pop == 0 || pop >= 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    NsgaWorkspace w;
    const hipError_t e = nsga_workspace(pop, a, &w);
    if (e != hipSuccess) return (int)e;
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_pareto_rank(unsigned pop, unsigned cx_bound, const float *err, const int *cx, int *front, float *crowding, int *order,
                                     void *workspace, evogp_stream_t stream_) {
    if (pop == 0 || pop >= 0x7FFFFFFFu || cx_bound > 65535u) return EVOGP_E_BADARG;
    if (!err || !cx || !front || !crowding || !order || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    Arena a{(char *)workspace};
    NsgaWorkspace w;
    hipError_t e = nsga_workspace(pop, a, &w);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((pop + 255u) / 256u), block(256);

    // 1. the key order: k32_b / v_b = keys and trees in key order, scan = the first position of every tree's run of equal keys
    hipLaunchKernelGGL(nsga_keys_kernel, grid, block, 0, stream, err, cx, pop, cx_bound, w.k32_a, w.v_a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = sort_pairs(w.temp, w.temp_bytes, w.k32_a, w.k32_b, w.v_a, w.v_b, pop, 0u, 32u, stream)) != hipSuccess) return (int)e;
    const unsigned *tree1 = w.v_b;
    hipLaunchKernelGGL(nsga_runs_kernel, grid, block, 0, stream, (const unsigned *)w.k32_b, tree1, cx, pop, w.head, w.k32_a, w.v_a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = scan_max(w.temp, w.temp_bytes, w.head, w.scan, pop, stream)) != hipSuccess) return (int)e;
    if (g_nsga_stop == 1) return EVOGP_OK;

    // 2. the bucket order: k32_b = cx, t2 / f2 = the tree and the first position of its key, gid = the group numbers
    unsigned *s2 = (unsigned *)w.front_u;   // (free until the chain kernel)
    if ((e = sort_pairs(w.temp, w.temp_bytes, w.k32_a, w.k32_b, w.v_a, s2, pop, 0u, 17u, stream)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nsga_groups_kernel, grid, block, 0, stream, (const unsigned *)w.k32_b, (const unsigned *)s2, (const unsigned *)w.scan, tree1,
                       pop, w.f2, w.t2, w.head, w.bend, front);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = scan_plus(w.temp, w.temp_bytes, w.head, w.gid, pop, stream)) != hipSuccess) return (int)e;
    if (g_nsga_stop == 2) return EVOGP_OK;

    // 3. the fronts
    if ((e = hipMemsetAsync(w.fen, 0xFF, ((size_t)pop + 1u) * 4, stream)) != hipSuccess) return (int)e;
    NsgaChain ch{w.k32_b, w.f2, w.t2, w.gid, w.bend, w.fen, w.front_u, front, pop};
    hipLaunchKernelGGL(nsga_chain_kernel, dim3(1), dim3(kNsgaChainThreads), 0, stream, ch);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (g_nsga_stop == 3) return EVOGP_OK;

    // 4. the points of every front and their crowding distance
    hipLaunchKernelGGL(nsga_front_keys_kernel, grid, block, 0, stream, (const int *)front, cx, pop, w.k64_a, w.v_a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = sort_pairs(w.temp, w.temp_bytes, w.k64_a, w.k64_b, w.v_a, w.v_b, pop, 0u, 48u, stream)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nsga_point_heads_kernel, grid, block, 0, stream, (const unsigned long long *)w.k64_b, pop, w.head);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = scan_plus_excl(w.temp, w.temp_bytes, w.head, w.scan, pop, stream)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nsga_points_kernel, grid, block, 0, stream, (const unsigned long long *)w.k64_b, (const unsigned *)w.v_b,
                       (const unsigned *)w.head, (const unsigned *)w.scan, err, pop, w.pt_key, w.pt_cx, w.first_of, w.last_of);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nsga_crowding_kernel, grid, block, 0, stream, (const unsigned long long *)w.k64_b, (const unsigned *)w.v_b,
                       (const unsigned *)w.head, (const unsigned *)w.scan, (const float *)w.pt_key, (const unsigned *)w.pt_cx,
                       (const unsigned *)w.first_of, (const unsigned *)w.last_of, pop, crowding, w.k64_a, w.v_a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (g_nsga_stop == 4) return EVOGP_OK;

    // 5. the order
    return (int)sort_pairs(w.temp, w.temp_bytes, w.k64_a, w.k64_b, w.v_a, (unsigned *)order, pop, 0u, 63u, stream);
}

extern "C" int evogp_hip_nsga2_select(unsigned pop, const int *order, unsigned pool, unsigned n_tournaments, unsigned t_size, long long seed,
                                      long long generation, int *winners, evogp_stream_t stream_) {
    if (pop == 0 || pop >= 0x7FFFFFFFu || pool == 0 || pool > pop || t_size == 0 || t_size > (1u << 20) || n_tournaments > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (n_tournaments == 0) return EVOGP_OK;
    if (!order || !winners) return EVOGP_E_NULLPTR;
    hipLaunchKernelGGL(nsga_select_kernel, dim3((n_tournaments + 255u) / 256u), dim3(256), 0, (hipStream_t)stream_, order, pool, n_tournaments, t_size,
                       counter_base(seed, generation), winners);
    return (int)hipGetLastError();
}

// Measurement hook (include/evogp_hip_debug.h)
extern "C" int evogp_hip_debug_pareto_rank(int stop_after) {
    if (stop_after < 0 || stop_after > 4) return EVOGP_E_BADARG;
    g_nsga_stop = stop_after;
    return EVOGP_OK;
}
