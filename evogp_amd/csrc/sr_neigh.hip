// sr_neigh.hip — semantic neighbourhoods of a whole population of single-output SR trees: for every tree of a list its k nearest trees by
// squared Euclidean distance between prediction vectors, and how many lie within given radii, on the float64 matrix cores and WITHOUT the
// n x n matrix (gfx950; no counterpart in the reference).  include/evogp_hip.h has the contract, DESIGN 3.32 the reasoning,
// sr_gram_order.hpp the order of summation it shares with the Gram matrix (sr_gram.hip).
//
// For index[0 .. n): p_i the float32 predictions of tree index[i], G_ij = sum_d (double)p_i[d] (double)p_j[d] in the pinned order,
// N_i = G_ii,  d2(i, j) = max(0, fma(-2, G_ij, N_i + N_j)).  A word G_ij has the same bits wherever the pair falls (the order depends on D
// alone), so d2 is symmetric bit for bit and exactly 0 between two trees of equal prediction bits.
//
//   1. gram_panel_kernel<VL, LEAN>, gram_panel_general_kernel (sr_gram_panel.hpp), once per slab of 4096 rows into a panel that keeps ALL
//                              rows of every tree: [n][roundup4(D)] floats
//   2. neigh_norm_kernel       the diagonal 64 x 64 blocks through the same chain of v_mfma_f64_16x16x4_f64: N_i (a scalar sum would have
//                              other bits, and duplicates would not come out at distance 0)
//   3. neigh_strip_kernel      grid (row block I, column split s).  Four waves, a 32 x 32 quadrant = 2 x 2 instruction tiles each.  For
//                              every column block J of the split the workgroup runs the full-D chain (32-row chunks of the 64 + 64 panel
//                              rows through LDS, double-buffered through registers), then CONSUMES the block: the 64 x 64 words go to an
//                              LDS tile that aliases the staging buffers, a wave takes 16 rows with the 64 candidates of a row one per
//                              lane, forms d2, counts the radii by ballots and offers the candidates that beat the row's k-th (d2, j) to
//                              the row's sorted list.  The lists and counts live in REGISTERS for the whole strip: the 16 slots of row
//                              4 rr + g of a wave are register rr of the lanes 16 g .. 16 g + 15.  Nothing of the block is stored.
//                              The full square is computed, not the triangle: the mirror of a block would feed the lists of rows that
//                              other workgroups own.  At the end the partial lists and counts go to the workspace as [n][S][k].
//   4. neigh_merge_kernel      a wave per row merges the S partial lists by the same offer and adds the counts; NaN, -1 and 0 by the flags.
// The k smallest of a set under the total order (d2, j) do not depend on the order of arrival and counts are integer sums: no result
// depends on the split or on the order of the blocks.  No float atomics, nothing synchronises with the host, the engine allocates nothing.
#include <climits>

#include "sr_gram_panel.hpp"

namespace evogp {

constexpr int kNeighMaxK = 16;                 // list slots per row: a quarter wave
constexpr int kNeighMaxRadii = 8;
constexpr int kNeighFullGrid = 512;            // workgroups the strip kernel wants at least; from this many row blocks on one split
constexpr int kNeighTileLd = kGramBlock + 16;  // doubles per row of the LDS tile: the four row groups of a store fall 32 banks apart
constexpr size_t kNeighStageBytes = sizeof(float) * 2 * 2 * kGramBlock * kGramLd;
constexpr size_t kNeighTileBytes = sizeof(double) * kGramBlock * kNeighTileLd;
constexpr size_t kNeighLds = kNeighStageBytes > kNeighTileBytes ? kNeighStageBytes : kNeighTileBytes;
constexpr unsigned long long kNeighMaxPanel = 1ull << 29;   // floats of the resident panel

struct NeighParams {
    const float *panel;          // [n][stride]: every row of every tree
    const int *bad;              // [n] != 0: tree i is unusable
    double *normw;               // [n]: N_i (workspace)
    const double *radius2;       // [R]
    double *part_d;              // [n][S][k]: the partial lists, (+inf, INT_MAX) in their empty slots
    int *part_j;
    int *part_c;                 // [n][S][R]
    double *dist2;               // [n][k]
    int *neigh;                  // [n][k]
    int *count;                  // [n][R]
    double *norm;                // [n]
    unsigned char *usable;       // [n]
    int n, D, stride, k, R;
    int S, per;                  // column splits, column blocks per split
};

__host__ __device__ inline int neigh_blocks_side(int n) { return (n + kGramBlock - 1) / kGramBlock; }

__global__ void neigh_init_kernel(int *bad, int words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) bad[i] = 0;
}

// ---- the chain ------------------------------------------------------------------------------------------------------------------------------
// The lane's 16 words of block (I, J) over all D rows, in the order of sr_gram_order.hpp: tile (ti, tj), register r is the word of vectors
// (I 64 + wi 32 + ti 16 + 4 r + q, J 64 + wj 32 + tj 16 + m).  Vectors past n and rows past D enter as 0.  v_s: [buffer][side I / J][vector]
// [row of the chunk].  Every thread of the workgroup calls it; the last thing it does is a barrier, so v_s is free on return.
__device__ inline void neigh_chain(const NeighParams &p, int I, int J, float (*v_s)[2][kGramBlock][kGramLd], double (&tot)[2][2][4]) {
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int wi = w >> 1, wj = w & 1;
    const int m = lane & 15, q = lane >> 4;

    float4 pre[4];   // the global side of the double buffer: 128 vectors x 8 float4 per chunk, four float4 per thread
    auto fetch = [&](int r0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int item = (int)threadIdx.x + k * 256;
            const int vl = item >> 3, c4 = item & 7;
            const int g = ((vl >> 6) ? J : I) * kGramBlock + (vl & 63);
            const int r = r0 + c4 * 4;
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (g < p.n && r < p.D) {
                const float4 x = *(const float4 *)(p.panel + (size_t)g * p.stride + r);   // r + 3 < stride: both are multiples of 4
                e[0] = x.x; e[1] = x.y; e[2] = x.z; e[3] = x.w;
#pragma unroll
                for (int u = 0; u < 4; ++u) e[u] = r + u < p.D ? e[u] : 0.0f;
            }
            pre[k] = make_float4(e[0], e[1], e[2], e[3]);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int item = (int)threadIdx.x + k * 256;
            const int vl = item >> 3, c4 = item & 7;
            *(float4 *)&v_s[buf][vl >> 6][vl & 63][c4 * 4] = pre[k];
        }
    };

#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) tot[ti][tj][r] = 0.0;

    const int nseg = gram_segments(p.D);
    for (int s = 0; s < nseg; ++s) {
        gram_acc acc[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = gram_acc{0.0, 0.0, 0.0, 0.0};
        constexpr int NCHUNK = kGramSegment / kGramChunk;
        const int seg0 = s * kGramSegment;
        fetch(seg0);
        stage(0);
        __syncthreads();
        for (int c = 0; c < NCHUNK; ++c) {
            const int buf = c & 1;
            if (c + 1 < NCHUNK) fetch(seg0 + (c + 1) * kGramChunk);
#pragma unroll
            for (int g = 0; g < kGramChunk / kGramGroup; ++g) {
                double a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = (double)v_s[buf][0][wi * 32 + t * 16 + m][g * kGramGroup + q];
                    b[t] = (double)v_s[buf][1][wj * 32 + t * 16 + m][g * kGramGroup + q];
                }
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = gram_step(acc[ti][tj], a[ti], b[tj]);
            }
            if (c + 1 < NCHUNK) stage(buf ^ 1);
            __syncthreads();
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) tot[ti][tj][r] = gram_add_segment(tot[ti][tj][r], acc[ti][tj][r]);
    }
}

// ---- 2. the norms ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGramWaves * 64, 2) void neigh_norm_kernel(NeighParams p) {
    __shared__ __align__(16) char smem[kNeighStageBytes];
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int m = lane & 15, q = lane >> 4;
    const int I = (int)blockIdx.x;
    double tot[2][2][4];
    neigh_chain(p, I, I, (float (*)[2][kGramBlock][kGramLd])smem, tot);
    const bool diagonal = (w >> 1) == (w & 1);   // the diagonal lies in the quadrants (0, 0) and (1, 1)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int g = I * kGramBlock + (w >> 1) * 32 + t * 16 + m;
            if (diagonal && 4 * r + q == m && g < p.n) p.normw[g] = p.norm[g] = tot[t][t][r];
        }
}

// ---- the sorted lists -------------------------------------------------------------------------------------------------------------------------
__device__ inline bool neigh_less(double d, int j, double ld, int lj) { return d < ld || (d == ld && j < lj); }

// The whole wave offers one candidate (d, j) per lane (take: the lane has one) to the ascending list whose slot t is (ld, lj) of lane
// base + t, t < k; the other lanes' ld, lj belong to other lists and stay.  The candidates that beat the k-th entry enter one at a time,
// lowest lane first, and the set that still beats it is taken again after every entry.  All branches are wave-uniform.
__device__ inline void neigh_offer(double d, int j, bool take, int base, int k, double &ld, int &lj) {
    const int t = (int)(threadIdx.x & 63) - base;
    const bool mine = t >= 0 && t < k;
    double kd = __shfl(ld, base + k - 1);
    int kj = __shfl(lj, base + k - 1);
    unsigned long long enter = __ballot(take && neigh_less(d, j, kd, kj));
    while (enter) {
        const int src = __ffsll((long long)enter) - 1;
        const double cd = __shfl(d, src);
        const int cj = __shfl(j, src);
        const int pos = __popcll(__ballot(mine && neigh_less(ld, lj, cd, cj)));   // the entries in front of it: a prefix of the list
        const double ud = __shfl_up(ld, 1);
        const int uj = __shfl_up(lj, 1);
        if (mine && t >= pos) {
            ld = t == pos ? cd : ud;
            lj = t == pos ? cj : uj;
        }
        kd = __shfl(ld, base + k - 1);
        kj = __shfl(lj, base + k - 1);
        enter &= enter - 1;
        enter &= __ballot(take && neigh_less(d, j, kd, kj));
    }
}

// ---- 3. the strip ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGramWaves * 64, 2) void neigh_strip_kernel(NeighParams p) {
    __shared__ __align__(16) char smem[kNeighLds];   // the staging buffers of the chain, then the 64 x 64 tile of the block's words
    __shared__ double ni_s[kGramBlock];              // N_i of the strip's rows
    __shared__ double rad_s[kNeighMaxRadii];
    float (*const v_s)[2][kGramBlock][kGramLd] = (float (*)[2][kGramBlock][kGramLd])smem;
    double (*const t_s)[kNeighTileLd] = (double (*)[kNeighTileLd])smem;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int wi = w >> 1, wj = w & 1;
    const int m = lane & 15, q = lane >> 4;
    const int I = (int)blockIdx.x, split = (int)blockIdx.y;
    const int nb = neigh_blocks_side(p.n);
    if (threadIdx.x < kGramBlock) {
        const int gi = I * kGramBlock + (int)threadIdx.x;
        ni_s[threadIdx.x] = gi < p.n ? p.normw[gi] : 0.0;
    }
    if (threadIdx.x < kNeighMaxRadii) rad_s[threadIdx.x] = (int)threadIdx.x < p.R ? p.radius2[threadIdx.x] : 0.0;
    // (the chain's first barrier comes before anyone reads ni_s or rad_s)

    double ld[4];   // slot lane % 16 of the list of row w 16 + 4 rr + lane / 16
    int lj[4];
    int cnt[4];     // the lanes 16 g + r, r < R: the count of radius r of that row
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        ld[rr] = __builtin_inf();
        lj[rr] = INT_MAX;
        cnt[rr] = 0;
    }

    const int J0 = split * p.per;
    const int J1 = J0 + p.per < nb ? J0 + p.per : nb;
    for (int J = J0; J < J1; ++J) {
        double tot[2][2][4];
        neigh_chain(p, I, J, v_s, tot);
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) t_s[wi * 32 + ti * 16 + 4 * r + q][wj * 32 + tj * 16 + m] = tot[ti][tj][r];
        const int gj = J * kGramBlock + lane;   // the lane's candidate in every row
        const bool col_ok = gj < p.n && p.bad[gj < p.n ? gj : 0] == 0;
        const double nj = gj < p.n ? p.normw[gj] : 0.0;
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            for (int g = 0; g < 4; ++g) {
                const int row = w * 16 + rr * 4 + g;
                const double d = fmax(0.0, fma(-2.0, t_s[row][lane], __dadd_rn(ni_s[row], nj)));
                const bool take = col_ok && gj != I * kGramBlock + row;   // (a row past n or of an unusable tree keeps a list nobody reads)
                for (int r = 0; r < p.R; ++r) {
                    const int inside = __popcll(__ballot(take && d <= rad_s[r]));
                    cnt[rr] += lane == g * 16 + r ? inside : 0;
                }
                neigh_offer(d, gj, take, g * 16, p.k, ld[rr], lj[rr]);
            }
        __syncthreads();   // the tile is consumed: the next chain may stage over it
    }

#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int gi = I * kGramBlock + w * 16 + rr * 4 + q;
        if (gi < p.n) {
            const size_t at = (size_t)gi * p.S + split;
            if (m < p.k) {
                p.part_d[at * p.k + m] = ld[rr];
                p.part_j[at * p.k + m] = lj[rr];
            }
            if (m < p.R) p.part_c[at * p.R + m] = cnt[rr];
        }
    }
}

// ---- 4. the merge ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGramWaves * 64) void neigh_merge_kernel(NeighParams p) {
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * kGramWaves + uni((int)(threadIdx.x >> 6));   // a wave per row
    if (i < p.n) {
        const bool bad = uni(p.bad[i]) != 0;
        const int total = p.S * p.k;
        double ld = __builtin_inf();
        int lj = INT_MAX;
        for (int base = 0; base < total; base += kWave) {
            const int e = base + lane;
            const bool in = e < total;
            const double d = in ? p.part_d[(size_t)i * total + e] : __builtin_inf();
            const int j = in ? p.part_j[(size_t)i * total + e] : INT_MAX;
            neigh_offer(d, j, in && j != INT_MAX, 0, p.k, ld, lj);
        }
        if (lane < p.k) {
            p.dist2[(size_t)i * p.k + lane] = bad ? __builtin_nan("") : ld;
            p.neigh[(size_t)i * p.k + lane] = bad || lj == INT_MAX ? -1 : lj;
        }
        if (lane < p.R) {
            int c = 0;
            for (int s = 0; s < p.S; ++s) c += p.part_c[((size_t)i * p.S + s) * p.R + lane];
            p.count[(size_t)i * p.R + lane] = bad ? 0 : c;
        }
        if (lane == 0) {
            p.norm[i] = bad ? __builtin_nan("") : p.normw[i];
            p.usable[i] = bad ? 0 : 1;
        }
    }
}

static int g_neigh_stages = 15;   // evogp_hip_debug_sr_neighbours: bit 0 the panel, bit 1 the norms, bit 2 the strip, bit 3 the merge
static int g_neigh_splits = 0;    // ... and a forced number of column splits (0: the host's choice)

static int neigh_stride(unsigned D) { return (int)((D + 3u) & ~3u); }

// the column splits of n trees: enough for about kNeighFullGrid workgroups, none of them empty
static void neigh_splits(int n, int *S, int *per) {
    const int nb = n > 0 ? neigh_blocks_side(n) : 1;
    int want = g_neigh_splits > 0 ? g_neigh_splits : (nb >= kNeighFullGrid ? 1 : (kNeighFullGrid + nb - 1) / nb);
    if (want > nb) want = nb;
    *per = (nb + want - 1) / want;
    *S = (nb + *per - 1) / *per;
}

static int neigh_badarg(unsigned n, unsigned data_points, unsigned k, unsigned n_radii) {
    if (n > (unsigned)EVOGP_NEIGH_MAX_TREES || data_points == 0 || data_points > 0x7FFFFFFFu || k < 1 || k > (unsigned)kNeighMaxK ||
        n_radii > (unsigned)kNeighMaxRadii)
        return EVOGP_E_BADARG;
    if ((unsigned long long)n * (((unsigned long long)data_points + 3u) & ~3ull) > kNeighMaxPanel) return EVOGP_E_BADARG;
    return EVOGP_OK;
}

// the buffers of the workspace, in one order for the size query and the call
static void neigh_carve(Arena &a, GramParams &g, NeighParams &p, unsigned n, unsigned D, unsigned k, unsigned R) {
    g.stride = p.stride = neigh_stride(D);
    g.panel = a.take<float>((size_t)n * p.stride);
    g.bad = a.take<int>((size_t)n + 2);
    g.mark = a.take<unsigned char>(n);
    p.normw = a.take<double>(n);
    neigh_splits((int)n, &p.S, &p.per);
    p.part_d = a.take<double>((size_t)n * p.S * k);
    p.part_j = a.take<int>((size_t)n * p.S * k);
    p.part_c = a.take<int>((size_t)n * p.S * (R ? R : 1));
    p.panel = g.panel;
    p.bad = g.bad;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_debug_sr_neighbours(int stages) {
    if (stages < 0 || (stages & 0xFF) > 15 || (stages >> 8) > 4096) return EVOGP_E_BADARG;
    g_neigh_stages = stages & 0xFF;
    g_neigh_splits = stages >> 8;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_neighbours_workspace_bytes(unsigned n, unsigned data_points, unsigned k, unsigned n_radii, unsigned long long *bytes) {
    if (const int rc = neigh_badarg(n, data_points, k, n_radii)) return rc;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    GramParams g{};
    NeighParams p{};
    neigh_carve(a, g, p, n, data_points, k, n_radii);
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_neighbours(unsigned n, unsigned data_points, unsigned var_len, unsigned pop_size, unsigned gp_len, const float *value,
                                       const int16_t *type, const int16_t *size, const float *variables, const int *index, unsigned k,
                                       unsigned n_radii, const double *radius2, double *dist2_out, int *neighbour_out, int *count_out,
                                       double *norm_out, unsigned char *usable_out, void *workspace, evogp_stream_t stream_) {
    if (const int rc = neigh_badarg(n, data_points, k, n_radii)) return rc;
    if (var_len == 0 || pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || pop_size > 0x7FFFFFFFu || var_len > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables) return EVOGP_E_NULLPTR;
    if (n == 0) return EVOGP_OK;   // empty outputs: nothing to launch, and nothing to point at
    if (!index || !dist2_out || !neighbour_out || !norm_out || !usable_out || !workspace || (n_radii && (!radius2 || !count_out)))
        return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    hipError_t e;
    Arena a{(char *)workspace};
    GramParams g{};
    NeighParams p{};
    neigh_carve(a, g, p, n, data_points, k, n_radii);
    g.value = value; g.type = type; g.size = size; g.pop = (int)pop_size; g.gp_len = (int)gp_len;
    g.X = variables; g.index = index; g.n = (int)n; g.D = (int)data_points; g.var_len = (int)var_len;
    p.radius2 = radius2; p.dist2 = dist2_out; p.neigh = neighbour_out; p.count = count_out; p.norm = norm_out; p.usable = usable_out;
    p.n = (int)n; p.D = (int)data_points; p.k = (int)k; p.R = (int)n_radii;

    hipLaunchKernelGGL(neigh_init_kernel, dim3((n + 2 + 255) / 256), dim3(256), 0, stream, g.bad, (int)n + 2);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const bool regs = g.var_len <= 32;
    float *const panel = g.panel;
    for (long long row0 = 0; (g_neigh_stages & 1) && row0 < (long long)g.D; row0 += kGramSlab) {
        g.row0 = (int)row0;
        g.rows = (long long)g.D - row0 < kGramSlab ? (int)((long long)g.D - row0) : kGramSlab;
        g.panel = panel + row0;   // the slab's columns of the resident panel
        if (regs) {
            e = g.var_len <= 12 ? launch_panel<12, true>(g, stream) : launch_panel<32, true>(g, stream);
            if (e != hipSuccess) return (int)e;
            e = g.var_len <= 12 ? launch_panel<12, false>(g, stream) : launch_panel<32, false>(g, stream);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(gram_panel_general_kernel, dim3(n), dim3(kGramWaves * 64), 0, stream, g, regs ? 0 : 1);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    const unsigned nb = (unsigned)neigh_blocks_side(p.n);
    if (g_neigh_stages & 2) {
        hipLaunchKernelGGL(neigh_norm_kernel, dim3(nb), dim3(kGramWaves * 64), 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    if (g_neigh_stages & 4) {
        hipLaunchKernelGGL(neigh_strip_kernel, dim3(nb, (unsigned)p.S), dim3(kGramWaves * 64), 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    if (g_neigh_stages & 8) {
        hipLaunchKernelGGL(neigh_merge_kernel, dim3((n + kGramWaves - 1) / kGramWaves), dim3(kGramWaves * 64), 0, stream, p);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    return EVOGP_OK;
}
