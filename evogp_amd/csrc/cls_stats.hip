// cls_stats.hip — classification statistics and the soft-max cross-entropy of a multi-output forest in one pass (gfx950).
//
// For every tree t, every row split g < G and every class c < C (= out_len):
//   hits[t][g][c]       rows of split g with label c that tree t predicts as c
//   predicted[t][g][c]  rows of split g that tree t predicts as c
//   loss[t][g]          mean soft-max cross-entropy of tree t over the rows of split g (float64)
// Row d belongs to split groups[d] when 0 <= groups[d] < G (no groups: split 0) and is COUNTED when, besides, 0 <= labels[d] < C; a row that
// is not counted is looked at in no output.  The prediction is the rule of evogp_hip_batch_argmax_count (interp.hpp: torch.argmax(clip(
// softmax(x))), first maximum, index 0 for a NaN output or an infinite maximum, near-ties by argmax_as_torch).  Per counted row, in
// float32: m = max_o x_o; poisoned (a NaN output or an infinite m) -> NaN; else s = sum_o expf(x_o - m) with o ascending,
// l = logf(s) - (x_y - m) clamped to [0, 34.538776 = -log(1e-15)].  loss[t][g] = (sum of l over the counted rows of g) / their number;
// an empty split gives NaN.
//
// The skeleton is sr_wide_kernel<MO = true, MODE = 1> (sr_wide.hip): a workgroup stages one TILE of R = 64 K rows as [variable][row] in
// LDS and its eight waves walk different trees over it with the register-stack interpreter; lane l holds rows K l .. K l + K - 1.
//   counts  every wave keeps a histogram [split][class][hit] in LDS: one ds_add per counted row, then one integer atomic per non-zero
//           entry (hits, predicted) -- the tiles of a tree meet in global memory, and integer sums do not depend on the order;
//   loss    float64, no atomics: a lane adds its rows in ascending order, the 64 lanes by wave_sum_d, lane 0 stores the partial of
//           (tree, tile, split) into the stream's workspace and cls_finish_kernel adds the partials in tile order and divides.
//           Every row's l is split as l = l_hi + l_lo, l_hi = l rounded to a multiple of 2^-20 (one add and one subtract of 2^32):
//           l is 0 or a float in [2^-24, 2^6), so l_lo is a multiple of 2^-47 below 2^-20, and both column sums are EXACT in float64 for
//           any D < 2^26.  The loss is therefore ((sum l_hi) + (sum l_lo)) / n with two roundings whatever the order -- a split's column
//           equals, bit for bit, that of a call on the split's rows alone -- and a NaN row poisons its own split only.
//   workspace  2 doubles per (tree, tile, split) and one flag word per tree; the population is cut into slices of at most
//           kClsWorkspaceBytes.
// Trees the register stack cannot hold (TREE_DEEP) and trees with a row whose arg-max hangs on the soft-max's rounding are FLAGGED and
// redone by cls_recount_kernel: scratch-stack interpreter (run_general), argmax_as_torch, the same row layout, the same epilogue.  A
// malformed tree has every output NaN: class 0 on every counted row, loss NaN.
#include "interp.hpp"
#include "launch.hpp"
#include "sr_moments.hpp"
#include <cstdlib>

namespace evogp {

constexpr int kClsWaves = 8;
constexpr int kClsMaxGroups = 8;
constexpr int kClsHistWords = 2 * kClsMaxGroups * kMaxOutRegs;   // per wave: [split][class][hit]
constexpr float kClsLossCap = 34.538776f;                        // -log(1e-15)
constexpr size_t kClsWorkspaceBytes = (size_t)128 << 20;

struct ClsParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;        // [D][var_len]
    const int *labels;     // [D]
    const int *groups;     // [D] or null
    int *hits, *predicted; // [pop][G][C], zeroed before the launch
    double *loss;          // [pop][G]
    double2 *part;         // [pop][ntiles][G]: {sum l_hi, sum l_lo}
    unsigned *flags;       // [pop], zeroed before the launch: 1 = cls_recount_kernel redoes the tree
    unsigned *marks;       // [1] != 0: some tree is flagged
    int pop, D, gp_len, var_len, out_len, G;
    int ntiles, workers;   // grid = ntiles * workers workgroups
};

struct ClsRow { int best; float loss; bool amb; };

// one row: the raw arg-max with its ambiguity (interp.hpp argmax_raw) and the clamped cross-entropy against `label`
__device__ inline ClsRow cls_row(const v16f &x, int C, int label) {
    int best = 0;
    float m = x[0];
    bool poisoned = m != m;
#pragma unroll
    for (int o = 1; o < kMaxOutRegs; ++o) {
        if (o < C) {
            const float v = x[o];
            poisoned |= v != v;
            if (v > m) { m = v; best = o; }
        }
    }
    const bool forced = poisoned || __builtin_isinf(m);
    const float thr = m - kSoftmaxTieMargin;
    bool amb = false;
    float s = 0.0f, xy = x[0];
#pragma unroll
    for (int o = 0; o < kMaxOutRegs; ++o) {
        if (o < C) {
            amb |= o < best && x[o] >= thr;
            s += expf(x[o] - m);
            xy = o == label ? x[o] : xy;
        }
    }
    float l = logf(s) - (xy - m);
    l = l < 0.0f ? 0.0f : (l > kClsLossCap ? kClsLossCap : l);
    ClsRow r;
    r.best = forced ? 0 : best;
    r.loss = forced ? __builtin_nanf("") : l;
    r.amb = amb && !forced;
    return r;
}

// a lane's K rows of tile `tile`: row[k] = split << 4 | label of a counted row, -1 of any other; -> the splits the wave's rows touch
template <int K>
__device__ inline unsigned cls_rows(const ClsParams &p, int tile, int lane, int (&row)[K]) {
    unsigned present = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int d = tile * K * 64 + lane * K + k, dc = d < p.D ? d : p.D - 1;
        const int y = p.labels[dc];
        const int g = p.groups ? p.groups[dc] : 0;
        const bool counted = d < p.D && g >= 0 && g < p.G && y >= 0 && y < p.out_len;
        row[k] = counted ? (g << 4 | y) : -1;
        for (int q = 0; q < p.G; ++q) present |= __ballot((row[k] >> 4) == q) != 0ull ? 1u << q : 0u;
    }
    return present;
}

// the epilogue of one (tree, tile) of one wave: hist is the wave's zeroed histogram and is left zeroed
template <int K>
__device__ inline void cls_emit(const ClsParams &p, int *hist, int t, int tile, int lane, unsigned present, const int (&row)[K],
                                const int (&pred)[K], const float (&l)[K]) {
    const int C = p.out_len, n = p.G * C;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (row[k] >= 0) atomicAdd(hist + ((((row[k] >> 4) * C + pred[k]) << 1) | (pred[k] == (row[k] & 15) ? 1 : 0)), 1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int e = lane; e < n; e += 64) {
        const int miss = hist[2 * e], hit = hist[2 * e + 1];
        hist[2 * e] = 0; hist[2 * e + 1] = 0;
        if (hit) atomicAdd(p.hits + (size_t)t * n + e, hit);
        if (miss + hit) atomicAdd(p.predicted + (size_t)t * n + e, miss + hit);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double2 *mine = p.part + ((size_t)t * p.ntiles + tile) * p.G;
    for (int g = 0; g < p.G; ++g) {
        double hi = 0.0, lo = 0.0;
        if ((present >> g) & 1u) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if ((row[k] >> 4) == g) {
                    const double dl = (double)l[k];
                    const double h = (dl + 0x1p32) - 0x1p32;   // l to a multiple of 2^-20 (NaN stays NaN)
                    hi += h;
                    lo += dl - h;
                }
            }
            hi = wave_sum_d(hi);
            lo = wave_sum_d(lo);
        }
        if (lane == 0) mine[g] = make_double2(hi, lo);
    }
}

template <int K, int DEPTH>
__global__ __launch_bounds__(kClsWaves * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void cls_stats_kernel(ClsParams p) {
    extern __shared__ float cls_lds[];  // [variable][R], then the waves' histograms
    constexpr int R = K * 64;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int tile = blockIdx.x % p.ntiles, worker = blockIdx.x / p.ntiles;
    const int row0 = tile * R;
    for (int e = threadIdx.x; e < R * p.var_len; e += blockDim.x) {
        const int dl = e / p.var_len, v = e - dl * p.var_len;
        const int d = row0 + dl < p.D ? row0 + dl : p.D - 1;
        cls_lds[v * R + dl] = p.X[(size_t)d * p.var_len + v];
    }
    int *hist = reinterpret_cast<int *>(cls_lds + (size_t)p.var_len * R) + w * kClsHistWords;
    for (int e = lane; e < kClsHistWords; e += 64) hist[e] = 0;
    __syncthreads();
    const LdsVars vars{cls_lds + lane * K, R};
    int row[K];
    const unsigned present = uni(cls_rows<K>(p, tile, lane, row));

    for (int t = worker * kClsWaves + w; t < p.pop; t += p.workers * kClsWaves) {
        const size_t at = (size_t)t * p.gp_len;
        const float *tv = p.value + at;
        const int16_t *tt = p.type + at;
        int len = uni((int)p.size[at]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int cls = uni(classify_tree(tt, tv, len, true, p.var_len, p.out_len, DEPTH));
        int pred[K];
        float l[K];
        if (cls == TREE_DEEP) {  // redone by cls_recount_kernel (every tile writes the same flag)
            if (lane == 0) { p.flags[t] = 1u; p.marks[1] = 1u; }
            continue;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) { pred[k] = 0; l[k] = __builtin_nanf(""); }   // malformed: all outputs NaN -> class 0, loss NaN
        bool any_amb = false;
        if (cls == TREE_OK) {
            v16f outs[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int o = 0; o < kMaxOutRegs; ++o) outs[k][o] = 0.0f;
            RegStack<K, DEPTH> st;
            st.h = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) st.tos[k] = 0.0f;
            for (int base = 0; base < len; base += kWave) {
                const int r = base + lane;
                uint32_t opv = 0, payv = 0;
                if (r < len) {
                    const Decoded dn = decode_node(tt[len - 1 - r], tv[len - 1 - r], true, p.var_len, p.out_len);
                    opv = dn.op; payv = dn.pay;
                }
                const int n = len - base < kWave ? len - base : kWave;
                run_chunk<true, false, K, DEPTH>(opv, payv, n, st, vars, outs);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const ClsRow r = cls_row(outs[k], p.out_len, row[k] & 15);
                pred[k] = r.best; l[k] = r.loss;
                any_amb |= r.amb && row[k] >= 0;
            }
        }
        if (__ballot(any_amb) != 0ull) {   // a counted row's arg-max hangs on the soft-max's rounding: redone with torch's arithmetic
            if (lane == 0) { p.flags[t] = 1u; p.marks[1] = 1u; }
            continue;
        }
        cls_emit<K>(p, hist, t, tile, lane, present, row, pred, l);
    }
}

// ---- the follow-up: flagged trees on the scratch-stack interpreter -------------------------------------------------------------------
// Three launches, all leaving at once when nothing is flagged: clear (the other tiles of a flagged tree may have added their counts),
// recount (a wave takes ONE tile of a flagged tree, blockIdx.y = tile, as wide_deep_count_kernel takes one row block), finish.
__global__ void cls_clear_kernel(ClsParams p) {
    if (p.marks[1] == 0u) return;
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= p.pop || p.flags[t] == 0u) return;
    const int n = p.G * p.out_len;
    for (int e = 0; e < n; ++e) { p.hits[(size_t)t * n + e] = 0; p.predicted[(size_t)t * n + e] = 0; }
}

template <int K>
__global__ __launch_bounds__(64) void cls_recount_kernel(ClsParams p) {
    if (p.marks[1] == 0u) return;
    __shared__ int hist[kClsHistWords];
    const int lane = threadIdx.x;
    float stk[kMaxStack + 2];
    float o16[kMaxOutRegs];
    for (int e = lane; e < kClsHistWords; e += 64) hist[e] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int tile = (int)blockIdx.y; tile < p.ntiles; tile += (int)gridDim.y) {
        int row[K];
        const unsigned present = uni(cls_rows<K>(p, tile, lane, row));
        for (int t0 = blockIdx.x * 64; t0 < p.pop; t0 += gridDim.x * 64) {
            const int tl = t0 + lane;
            unsigned long long marked = __ballot(tl < p.pop && p.flags[tl] != 0u);
            while (marked) {
                const int t = t0 + __builtin_ctzll(marked);
                marked &= marked - 1;
                const size_t at = (size_t)t * p.gp_len;
                int len = uni((int)p.size[at]);
                len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
                int pred[K];
                float l[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int d = tile * K * 64 + lane * K + k, dc = d < p.D ? d : p.D - 1;
                    (void)run_general<true>(p.type + at, p.value + at, len, p.X + (size_t)dc * p.var_len, p.var_len, p.out_len, o16, stk);
                    v16f x;
#pragma unroll
                    for (int o = 0; o < kMaxOutRegs; ++o) x[o] = o < p.out_len ? o16[o] : 0.0f;
                    l[k] = cls_row(x, p.out_len, row[k] & 15).loss;
                    pred[k] = argmax_as_torch(o16, p.out_len);
                }
                cls_emit<K>(p, hist, t, tile, lane, present, row, pred, l);
            }
        }
    }
}

// loss[t][g] = ((sum of the tiles' l_hi) + (sum of the tiles' l_lo)) / counted rows, the tiles in tile order
__global__ void cls_finish_kernel(ClsParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)p.pop * p.G) return;
    const int t = (int)(i / p.G), g = (int)(i - (long)t * p.G);
    long n = 0;
    for (int c = 0; c < p.out_len; ++c) n += p.predicted[((size_t)t * p.G + g) * p.out_len + c];
    double hi = 0.0, lo = 0.0;
    for (int tile = 0; tile < p.ntiles; ++tile) {
        const double2 q = p.part[((size_t)t * p.ntiles + tile) * p.G + g];
        hi += q.x; lo += q.y;
    }
    p.loss[i] = (hi + lo) / (double)n;   // (an empty split: 0 / 0)
}

template <int K, int DEPTH>
static hipError_t launch_cls(ClsParams p, hipStream_t stream) {
    const DeviceInfo &dev = device_info();
    constexpr int R = K * 64;
    const size_t lds = ((size_t)p.var_len * R + (size_t)kClsWaves * kClsHistWords) * 4;
    int per_cu = (int)((dev.lds_per_cu - 2048) / lds);
    per_cu = per_cu > 2 ? 2 : (per_cu < 1 ? 1 : per_cu);  // 2 x 8 waves = four per SIMD
    int workers = dev.num_cus * per_cu / p.ntiles;
    workers = workers < 1 ? 1 : workers;
    const int max_workers = (p.pop + kClsWaves - 1) / kClsWaves;
    p.workers = workers > max_workers ? max_workers : workers;
    auto kern = cls_stats_kernel<K, DEPTH>;
    static bool attr_done = false;
    if (!attr_done || lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { (void)hipGetLastError(); if (lds > 64 * 1024) return e; }
        attr_done = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.ntiles * p.workers)), dim3(kClsWaves * 64), lds, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cls_clear_kernel, dim3((unsigned)((p.pop + 255) / 256)), dim3(256), 0, stream, p);
    long blocks = ((long)p.pop + 63) / 64;
    blocks = blocks > 512 ? 512 : blocks;
    hipLaunchKernelGGL(cls_recount_kernel<K>, dim3((unsigned)blocks, (unsigned)(p.ntiles > 65535 ? 65535 : p.ntiles)), dim3(64), 0, stream, p);
    const long cells = (long)p.pop * p.G;
    hipLaunchKernelGGL(cls_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// rows per lane: two when two workgroups of them fit a CU's LDS and the dataset has more than 64 rows; EVOGP_CLS_K (1 | 2) overrides
static int cls_rows_per_lane(int var_len, int D) {
    const size_t budget = device_info().lds_per_cu - 2048;
    auto bytes = [&](int k) { return ((size_t)var_len * k * 64 + (size_t)kClsWaves * kClsHistWords) * 4; };
    int k = bytes(2) * 2 <= budget && D > 64 ? 2 : 1;
    if (const char *e = getenv("EVOGP_CLS_K")) { const int v = atoi(e); if (v == 1 || (v == 2 && bytes(2) <= budget)) k = v; }
    return k;
}

} // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_batch_class_stats(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                           const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                           const int *labels, const int *groups, unsigned n_groups, int *hits, int *predicted,
                                           double *loss, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len < 2 || n_groups < 1 ||
        n_groups > (unsigned)kClsMaxGroups || pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !labels || !hits || !predicted || !loss) return EVOGP_E_NULLPTR;
    if (out_len > (unsigned)kMaxOutRegs || (size_t)var_len * 256 > 150 * 1024) return EVOGP_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int K = cls_rows_per_lane((int)var_len, (int)data_points);
    const size_t ntiles = ((size_t)data_points + 64 * K - 1) / (64 * K);
    const size_t cells = (size_t)pop_size * n_groups * out_len;
    hipError_t e;
    if ((e = zero_words_async(hits, cells, stream)) != hipSuccess) return (int)e;
    if ((e = zero_words_async(predicted, cells, stream)) != hipSuccess) return (int)e;
    // slices of the population whose partials fit the workspace
    const size_t per_tree = ntiles * n_groups * sizeof(double2);
    size_t slice = kClsWorkspaceBytes / per_tree;
    slice = slice < 1 ? 1 : (slice > pop_size ? pop_size : slice);
    const size_t flag_bytes = (slice * 4 + 255) & ~(size_t)255;
    int rc = EVOGP_OK;
    char *ws = (char *)g_tape_workspaces.get(stream, flag_bytes + slice * per_tree, &rc);
    if (!ws) return rc;
    for (size_t t0 = 0; t0 < pop_size; t0 += slice) {
        const size_t n = pop_size - t0 < slice ? pop_size - t0 : slice;
        ClsParams p{};
        p.marks = acquire_counter(stream, &e);  // [1] != 0: some tree of the slice goes to the follow-up
        if (!p.marks) return (int)e;
        p.flags = (unsigned *)ws;
        p.part = (double2 *)(ws + flag_bytes);
        if ((e = zero_words_async(p.flags, n, stream)) != hipSuccess) return (int)e;
        p.value = value + t0 * gp_len; p.type = type + t0 * gp_len; p.size = size + t0 * gp_len;
        p.X = variables; p.labels = labels; p.groups = groups;
        p.hits = hits + t0 * n_groups * out_len; p.predicted = predicted + t0 * n_groups * out_len; p.loss = loss + t0 * n_groups;
        p.pop = (int)n; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.out_len = (int)out_len;
        p.G = (int)n_groups; p.ntiles = (int)ntiles;
        e = K == 2 ? launch_cls<2, 16>(p, stream) : launch_cls<1, 32>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    return EVOGP_OK;
}
