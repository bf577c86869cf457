// dedup.hip — structural duplicate detection over a forest (gfx950; no counterpart in the reference).
//
// Two rows are EQUAL when their live lengths n = size[t][0] are equal and in [1, gp_len] and, for every i < n, the fp32 bit pattern of
// value[i], the 16 bits of type[i] and size[i] agree (-0.0 != 0.0, NaNs by bits, the OUT flag counts; words at i >= n are never read).
// A row whose n is out of range is a class of its own, with hash 0.
//
// evogp_hip_tree_hash: one wave per tree, lanes over the nodes of the live prefix in chunks of 64:
//     w_i = (uint64)(uint16)type[i] << 32 | bits(value[i]);   hash = mix64((sum_{i<n} mix64(w_i ^ ((i + 1) * 0x9E3779B97F4A7C15))) + n)
// The sum is position-keyed and all arithmetic is mod 2^64, so the order in which the lanes add does not matter.
//
// evogp_hip_tree_classes: class_id[t] = the smallest tree index whose row equals row t.  Four stages on the caller's stream, nothing
// synchronises with the host, no atomics:
//   1. pairs     (hash_in[t], t) into the sort's buffers
//   2. sort      a stable radix sort of the pairs (rocPRIM): tree indices ascend within a run of equal hashes
//   3. runs      head marks and an inclusive maximum scan: the start st of the run every sorted position s lies in
//   4. classes   one wave per sorted position s: its tree compares its live prefix with the trees at st, st + 1, ..., s - 1 in that
//                order and takes the first equal one (the smallest equal index, since every equal row is in the run), else itself
// Only equality decides a class; the hashes decide which rows get compared.  The result is the same partition for any hash_in in which
// equal rows carry equal hashes.  Without a collision the first comparison decides; a run of r colliding distinct rows costs O(r^2)
// comparisons of up to n words each.
#include "dedup.hpp"
#include "evogp_defs.hpp"
#include "group_sort.hpp"
#include "launch.hpp"

namespace evogp {

constexpr unsigned kDedupWaves = 4;   // waves (trees) per workgroup

__global__ __launch_bounds__(kDedupWaves * 64) void tree_hash_kernel(const float *value, const int16_t *type, const int16_t *size, unsigned pop,
                                                                     unsigned gp_len, unsigned long long *hash) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned t = uni(blockIdx.x * kDedupWaves + (threadIdx.x >> 6));
    if (t >= pop) return;
    const size_t row = (size_t)t * gp_len;
    const int n = uni((int)size[row]);
    if (n < 1 || n > (int)gp_len) {
        if (lane == 0) hash[t] = 0ull;
        return;
    }
    unsigned long long acc = 0ull;
    for (unsigned i = lane; i < (unsigned)n; i += 64u) {
        const unsigned long long w = ((unsigned long long)(uint16_t)type[row + i] << 32) | (unsigned long long)f2bits(value[row + i]);
        acc += mix64(w ^ ((unsigned long long)(i + 1u) * kDedupGold));
    }
    acc = wave_sum_u64(acc);
    if (lane == 0) hash[t] = mix64(acc + (unsigned long long)n);
}

__global__ __launch_bounds__(256) void dedup_pairs_kernel(const unsigned long long *hash, unsigned pop, unsigned long long *key, unsigned *idx) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pop) return;
    key[i] = hash[i];
    idx[i] = i;
}

__global__ __launch_bounds__(256) void dedup_heads_kernel(const unsigned long long *key, unsigned pop, unsigned *head_pos) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= pop) return;
    head_pos[s] = (s == 0u || key[s] != key[s - 1u]) ? s : 0u;
}

__global__ __launch_bounds__(kDedupWaves * 64) void tree_classes_kernel(const float *value, const int16_t *type, const int16_t *size,
                                                                        const unsigned *members, const unsigned *seg, unsigned pop,
                                                                        unsigned gp_len, int *class_id) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned s = uni(blockIdx.x * kDedupWaves + (threadIdx.x >> 6));
    if (s >= pop) return;
    const unsigned t = uni(members[s]);
    const size_t row = (size_t)t * gp_len;
    const int n = uni((int)size[row]);
    unsigned rep = t;
    if (n >= 1 && n <= (int)gp_len) {
        const unsigned st = uni(seg[s]);
        for (unsigned j = st; j < s; ++j) {
            const unsigned u = uni(members[j]);
            const size_t other = (size_t)u * gp_len;
            if (uni((int)size[other]) != n) continue;
            bool same = true;
            for (unsigned base = 0; base < (unsigned)n && same; base += 64u) {
                const unsigned i = base + lane;
                bool diff = false;
                if (i < (unsigned)n)
                    diff = f2bits(value[row + i]) != f2bits(value[other + i]) || type[row + i] != type[other + i] ||
                           size[row + i] != size[other + i];
                same = !__any(diff);
            }
            if (same) { rep = u; break; }
        }
    }
    if (lane == 0) class_id[t] = (int)rep;
}

struct DedupWorkspace {
    unsigned long long *keys_a, *keys_b;
    unsigned *vals_a, *vals_b, *head_pos, *seg;
    void *temp;
    size_t temp_bytes;
};

static hipError_t dedup_workspace(unsigned pop, Arena &a, DedupWorkspace *w) {
    hipError_t e;
    w->temp_bytes = 0;
    if ((e = sort_buffers_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = scan_max_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    w->keys_a = a.take<unsigned long long>(pop); w->keys_b = a.take<unsigned long long>(pop);
    w->vals_a = a.take<unsigned>(pop); w->vals_b = a.take<unsigned>(pop);
    w->head_pos = a.take<unsigned>(pop); w->seg = a.take<unsigned>(pop);
    w->temp = a.take_bytes(w->temp_bytes);
    return hipSuccess;
}

hipError_t dedup_sorted_runs(const unsigned long long *hash_in, unsigned pop, void *workspace, const unsigned **members, const unsigned **seg,
                             hipStream_t stream) {
    Arena a{(char *)workspace};
    DedupWorkspace w;
    hipError_t e = dedup_workspace(pop, a, &w);
    if (e != hipSuccess) return e;
    const dim3 grid((pop + 255u) / 256u), block(256);
    hipLaunchKernelGGL(dedup_pairs_kernel, grid, block, 0, stream, hash_in, pop, w.keys_a, w.vals_a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bool in_b;
    if ((e = sort_buffers(w.temp, w.temp_bytes, w.keys_a, w.keys_b, w.vals_a, w.vals_b, pop, &in_b, stream)) != hipSuccess) return e;
    const unsigned long long *key = in_b ? w.keys_b : w.keys_a;
    *members = in_b ? w.vals_b : w.vals_a;
    hipLaunchKernelGGL(dedup_heads_kernel, grid, block, 0, stream, key, pop, w.head_pos);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = scan_max(w.temp, w.temp_bytes, w.head_pos, w.seg, pop, stream)) != hipSuccess) return e;
    *seg = w.seg;
    return hipSuccess;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_tree_hash(unsigned pop, unsigned gp_len, const float *value, const int16_t *type, const int16_t *size,
                                   unsigned long long *hash_out, evogp_stream_t stream_) {
    if (pop == 0 || pop > 0x7FFFFFFFu || gp_len == 0 || gp_len > (unsigned)kMaxStack) return EVOGP_E_BADARG;
    if (!value || !type || !size || !hash_out) return EVOGP_E_NULLPTR;
    hipLaunchKernelGGL(tree_hash_kernel, dim3((pop + kDedupWaves - 1u) / kDedupWaves), dim3(kDedupWaves * 64), 0, (hipStream_t)stream_, value, type,
                       size, pop, gp_len, hash_out);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_tree_classes_workspace_bytes(unsigned pop, unsigned long long *bytes) {
    if (pop == 0 || pop > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    DedupWorkspace w;
    const hipError_t e = dedup_workspace(pop, a, &w);
    if (e != hipSuccess) return (int)e;
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_tree_classes(unsigned pop, unsigned gp_len, const float *value, const int16_t *type, const int16_t *size,
                                      const unsigned long long *hash_in, int *class_id_out, void *workspace, evogp_stream_t stream_) {
    if (pop == 0 || pop > 0x7FFFFFFFu || gp_len == 0 || gp_len > (unsigned)kMaxStack) return EVOGP_E_BADARG;
    if (!value || !type || !size || !hash_in || !class_id_out || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    const unsigned *members, *seg;
    const hipError_t e = dedup_sorted_runs(hash_in, pop, workspace, &members, &seg, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(tree_classes_kernel, dim3((pop + kDedupWaves - 1u) / kDedupWaves), dim3(kDedupWaves * 64), 0, stream, value, type, size,
                       members, seg, pop, gp_len, class_id_out);
    return (int)hipGetLastError();
}
