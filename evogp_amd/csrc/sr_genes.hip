// sr_genes.hip — multi-gene SR fitness (GPTIPS; Arnaldo et al. 2014): the G outputs g_1 .. g_G of a tree are features, the model is
//     yhat = b0 + sum_j w_j g_j(x)
// with the least-squares b0, w of every tree, and the loss is its mean squared error (gfx950; no counterpart in the reference).
// include/evogp_hip.h has the contract (evogp_hip_sr_gene_fitness), DESIGN 3.16 the reasoning.
//
// sr_scale.hip's structure, generalised from one column to G.  Per tree the float64 co-moments of the float32 gene values with each
// other and with the centred labels are taken in ONE pass as SHIFTED sums: a wave subtracts from gene j the value a_j the gene has on
// the wave's first row (the pilot: in registers once the first tile is evaluated) before it squares and adds,
//     S_j = sum (g_j - a_j)    S_ij = sum (g_i - a_i)(g_j - a_j)    S_jv = sum (g_j - a_j) v    Sv = sum v      v = (double)y - ybar
// so a gene that is a large constant plus rounding noise loses nothing to cancellation.  A lane adds its rows (its tiles in ascending
// order), the 64 lanes are added by the fixed butterfly (wave_sum_d), the waves' partials are parked in LDS; one thread per tree turns
// each into (n, mean, M2, co-moments) and merges them in wave order by the pairwise update of Chan, Golub & LeVeque (1983), then runs
// the unrolled LDL^T of the contract.  No float atomics, no (pop, D, G) buffer; a tree's result depends on the tree and the dataset alone.
// Launches, all on the caller's stream, nothing synchronises with the host:
//   1. label_stats_kernel        (sr_moments.hpp) ybar, Syy: the bits linear scaling reads
//   2. sr_genes_kernel           the register interpreter (interp.hpp run_chunk<MO>), LEAN build over every tree, then the FULL build over
//                                the trees the LEAN one marked (sr_scale.hip has the scheme).  Built per gene bucket GB = 1 / 2 / 4 / 8
//                                (out_len 1 / 2 / 3-4 / 5-8): the lane partials are GB(GB+5)/2 + 1 doubles, so the rows per lane K and the
//                                trees per batch follow GB.  Genes past out_len are never written by a node, stay 0 and fall out as flat.
//   3. sr_genes_general_kernel   a wave per tree on the scratch stack (run_general<MO>): trees too deep for the registers, and every tree
//                                of a forest with more than 32 variables.  One accumulating unit, so nothing to merge.
// out_len == 1 follows batch_evaluate's single-output conventions (the gene is the tree's value), out_len > 1 the multi-output ones.
#include "interp.hpp"
#include "launch.hpp"
#include "sr_moments.hpp"
#include "sr_params.hpp"

namespace evogp {

constexpr int kGeneDepth = 16;   // register stack entries; deeper trees go to the scratch stack
constexpr int kGeneWaves = 4;    // waves per workgroup = accumulating units per tree
static_assert(EVOGP_GENES_MAX == 8, "the gene buckets end at 8");

constexpr int gene_bucket_k(int GB, int VL) { return GB == 1 ? 4 : (GB == 2 && VL <= 12) ? 4 : 2; }   // rows per lane
constexpr int gene_bucket_batch(int GB) { return GB <= 2 ? 32 : GB == 4 ? 16 : 8; }                 // trees per batch (LDS slots)

// the sums of one unit: S_j, the row-major upper triangle S_ij, S_jv, Sv
template <int GB>
struct GeneSums {
    static constexpr int TRI = GB * (GB + 1) / 2;
    static constexpr int N = GB + TRI + GB + 1;
    static constexpr int tri(int i, int j) { return GB + i * GB - i * (i - 1) / 2 + (j - i); }   // i <= j
    static constexpr int jv(int j) { return GB + TRI + j; }
    static constexpr int sv() { return GB + TRI + GB; }
};

template <int GB>
struct GeneUnit {
    double s[GeneSums<GB>::N];
    float pilot[GB], mn[GB], mx[GB];
    int n;     // rows the unit saw, >= 1
    int bad;   // some gene value is not finite
};

struct GeneParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *X;        // [D][var_len]
    const float *y;        // [D]
    float *loss;           // [pop]
    float *coef;           // [pop][1 + out_len]: intercept, weights
    double *moments;       // [pop][out_len (out_len + 5) / 2] or nullptr
    const double *stats;   // ybar, Syy (label_stats_kernel)
    unsigned *counter;     // as sr_scale.hip: [0] LEAN batch counter, [1] some tree is marked deep, [2] some is marked heavy, [3] FULL batch counter
    int pop, D, gp_len, var_len, out_len, batch, ntiles;
};

// a lane's rows into its sums; x[j] is the SHIFTED gene value, already 0 on a row past D, and so is v
template <int GB>
__device__ inline void gene_accumulate(double (&s)[GeneSums<GB>::N], const double (&x)[GB], double v) {
    using S = GeneSums<GB>;
#pragma unroll
    for (int i = 0; i < GB; ++i) {
        s[i] += x[i];
#pragma unroll
        for (int j = i; j < GB; ++j) s[S::tri(i, j)] += x[i] * x[j];
        s[S::jv(i)] += x[i] * v;
    }
    s[S::sv()] += v;
}

// lanes by the butterfly, parked by lane 0
template <int GB>
__device__ inline void gene_park(GeneUnit<GB> &u, const double (&s)[GeneSums<GB>::N], const float (&a)[GB], const float (&mn)[GB],
                                 const float (&mx)[GB], bool bad, int rows, int lane) {
    const bool any_bad = __any(bad) != 0;
#pragma unroll
    for (int i = 0; i < GeneSums<GB>::N; ++i) {
        const double tot = wave_sum_d(s[i]);
        if (lane == 0) u.s[i] = tot;
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        const float tmn = wave_min_f(mn[j]), tmx = wave_max_f(mx[j]);
        if (lane == 0) { u.pilot[j] = a[j]; u.mn[j] = tmn; u.mx[j] = tmx; }
    }
    if (lane == 0) { u.n = rows; u.bad = any_bad ? 1 : 0; }
}

__device__ inline void gene_store_nan(const GeneParams &p, int t, float lossv, bool zero_moments) {
    const float nan = __builtin_nanf("");
    const int G = p.out_len;
    p.loss[t] = lossv;
    for (int j = 0; j <= G; ++j) p.coef[(size_t)t * (G + 1) + j] = nan;
    if (zero_moments && p.moments) {
        const int nm = G * (G + 5) / 2;
        for (int j = 0; j < nm; ++j) p.moments[(size_t)t * nm + j] = 0.0;
    }
}

// ---- one thread per tree: merge the units in order, then the rules of the contract -----------------------------------------------------
template <int GB>
__device__ inline void gene_finish(const GeneParams &p, int t, const GeneUnit<GB> *u, int nu) {
    using S = GeneSums<GB>;
    const int G = p.out_len;
    // the merged means are kept as offsets ms[j] from unit 0's pilot p0[j]: a unit's mean joins as a difference of pilots (exact, or
    // rounded relative to the deviation itself) plus its shifted mean, so nothing of the size of the mean is rounded before the end
    double n = 0.0, meanv = 0.0, p0[GB], ms[GB], M2[S::TRI], cv[GB];
    float mn[GB], mx[GB];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < GB; ++j) { p0[j] = (double)u[0].pilot[j]; ms[j] = 0.0; cv[j] = 0.0; mn[j] = __builtin_inff(); mx[j] = -__builtin_inff(); }
#pragma unroll
    for (int j = 0; j < S::TRI; ++j) M2[j] = 0.0;
    for (int q = 0; q < nu; ++q) {
        const GeneUnit<GB> &b = u[q];
        bad = bad || b.bad != 0;
        const double nb = (double)b.n, nn = n + nb, fb = nb / nn, fab = n * nb / nn;
        const double sv = b.s[S::sv()];
        const double dv = sv / nb - meanv;
        double d[GB];
#pragma unroll
        for (int j = 0; j < GB; ++j) d[j] = (((double)b.pilot[j] - p0[j]) + b.s[j] / nb) - ms[j];
#pragma unroll
        for (int i = 0; i < GB; ++i) {
#pragma unroll
            for (int j = i; j < GB; ++j) {
                const int k = S::tri(i, j) - GB;
                M2[k] = (M2[k] + (b.s[S::tri(i, j)] - b.s[i] * b.s[j] / nb)) + d[i] * d[j] * fab;
            }
            cv[i] = (cv[i] + (b.s[S::jv(i)] - b.s[i] * sv / nb)) + d[i] * dv * fab;
        }
#pragma unroll
        for (int j = 0; j < GB; ++j) {
            ms[j] += d[j] * fb;
            mn[j] = fminf(mn[j], b.mn[j]);
            mx[j] = fmaxf(mx[j], b.mx[j]);
        }
        meanv += dv * fb;
        n = nn;
    }
    const double D = (double)p.D, ybar = p.stats[0], syy = p.stats[1];
    double C[S::TRI], c[GB], mean[GB];
#pragma unroll
    for (int j = 0; j < S::TRI; ++j) C[j] = M2[j] / D;
#pragma unroll
    for (int j = 0; j < GB; ++j) { c[j] = cv[j] / D; mean[j] = p0[j] + ms[j]; }
    if (p.moments) {
        double *row = p.moments + (size_t)t * (G * (G + 5) / 2);
        int o = 0;
#pragma unroll
        for (int j = 0; j < GB; ++j) if (j < G) row[o++] = mean[j];
#pragma unroll
        for (int i = 0; i < GB; ++i)
#pragma unroll
            for (int j = i; j < GB; ++j) if (j < G) row[o++] = C[S::tri(i, j) - GB];
#pragma unroll
        for (int j = 0; j < GB; ++j) if (j < G) row[o++] = c[j];
    }
    // LDL^T in index order; a gene that is flat or fails the pivot test gets an identity row (no data-dependent shape).  A tree with a
    // value that is not finite runs through it as well and is set to NaN at the one store below: no lane leaves early (Makefile, UNIFLAG)
    bool kept[GB];
    double L[GB][GB], dd[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        const double cjj = C[S::tri(j, j) - GB];
        const bool flat = j >= G || mn[j] == mx[j] || cjj <= 0.0 || p.D == 1;
        double dj = cjj;
#pragma unroll
        for (int k = 0; k < j; ++k) {
            double a = C[S::tri(k, j) - GB];
#pragma unroll
            for (int m = 0; m < k; ++m) a -= L[j][m] * L[k][m] * dd[m];   // (rows and columns of dropped genes hold 0)
            const double l = kept[k] ? a / dd[k] : 0.0;
            L[j][k] = l;
            dj -= l * l * dd[k];
        }
        kept[j] = !flat && dj > EVOGP_GENES_PIVOT_TOL * cjj;
        dd[j] = kept[j] ? dj : 1.0;
        if (!kept[j]) {
#pragma unroll
            for (int k = 0; k < j; ++k) L[j][k] = 0.0;
        }
    }
    double w[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        double z = kept[j] ? c[j] : 0.0;
#pragma unroll
        for (int k = 0; k < j; ++k) z -= L[j][k] * w[k];
        w[j] = z;
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) w[j] = w[j] / dd[j];
#pragma unroll
    for (int j = GB - 1; j >= 0; --j) {
        double z = w[j];
#pragma unroll
        for (int i = j + 1; i < GB; ++i) z -= L[i][j] * w[i];
        w[j] = kept[j] ? z : 0.0;
    }
    double b0 = ybar, loss = syy / D;
#pragma unroll
    for (int j = 0; j < GB; ++j) {
        if (kept[j]) { b0 -= w[j] * mean[j]; loss -= w[j] * c[j]; }
    }
    loss = loss > 0.0 ? loss : 0.0;
    const float lf = (float)loss, b0f = (float)b0;
    float wf[GB];
    bool ok = !bad && finite_f(b0f);
#pragma unroll
    for (int j = 0; j < GB; ++j) { wf[j] = (float)w[j]; ok = ok && finite_f(wf[j]); }
    const float nan = __builtin_nanf("");
    p.loss[t] = ok ? lf : nan;
    float *cf = p.coef + (size_t)t * (G + 1);
    cf[0] = ok ? b0f : nan;
#pragma unroll
    for (int j = 0; j < GB; ++j) if (j < G) cf[1 + j] = ok ? wf[j] : nan;
}

// ---- 2. the register interpreter ---------------------------------------------------------------------------------------------------
template <int GB, int VL, bool LEAN>
__global__ __launch_bounds__(kGeneWaves * 64, (GB <= 2 && VL <= 16) ? 2 : 1) void sr_genes_kernel(GeneParams p) {
    constexpr int K = gene_bucket_k(GB, VL), DEPTH = kGeneDepth, TILE = kWave * K, BATCH = gene_bucket_batch(GB);
    constexpr bool MO = GB > 1;
    using S = GeneSums<GB>;
    __shared__ GeneUnit<GB> part[BATCH][kGeneWaves];
    __shared__ int cls_s[BATCH];
    __shared__ unsigned next_s[2];   // (unsigned: the counter runs past pop by up to two batches per workgroup)

    if (!LEAN && uni((int)p.counter[2]) == 0) return;   // the LEAN pass marked nothing
    unsigned *const batches = p.counter + (LEAN ? 0 : 3);
    using VARS = typename VecOf<VL>::type;
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;
    const int batch = p.batch;
    const bool single = p.ntiles <= W;   // every wave owns one tile for its whole life: rows and labels are loaded once
    const double ybar = p.stats[0];

    VARS vars[K];
    float yv[K];
    bool valid[K];
    int tile_rows = 0;   // wave-uniform: rows of the tile last loaded
    auto load_tile = [&](int tile) {
        const long long first = (long long)tile * TILE;   // (64 bits, wave-uniform: D may lie within a tile of INT_MAX)
        const long long left = (long long)p.D - first;
        const int rows = left < TILE ? (int)left : TILE;  // rows of this tile, >= 1
        tile_rows = rows;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int off = k * kWave + lane;
            valid[k] = off < rows;
            const size_t dc = (size_t)first + (size_t)(valid[k] ? off : rows - 1);   // lanes past the end repeat the last row: min, max and "finite" are not disturbed
            const float *xr = p.X + dc * p.var_len;
#pragma unroll
            for (int v = 0; v < VL; ++v) vars[k][v] = v < p.var_len ? xr[v] : 0.0f;
            yv[k] = p.y[dc];
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
            if (LEAN || uni(f2bits(p.loss[t0 + b])) == kSentinelHeavy)
                c = classify_tree(p.type + row, p.value + row, len, MO, p.var_len, p.out_len, DEPTH, LEAN ? 1 : 0);
            if (lane == 0) cls_s[b] = c;
        }
        __syncthreads();

        // ---- phase 2: every wave interprets every tree of the batch on its own rows ----
        for (int b = 0; b < nb; ++b) {
            if (uni(cls_s[b]) != TREE_OK) continue;
            const size_t row = (size_t)(t0 + b) * p.gp_len;
            const float *tv = p.value + row;
            const int16_t *tt = p.type + row;
            int len = uni((int)p.size[row]);
            len = len > p.gp_len ? p.gp_len : len;

            double s[S::N];
            float a[GB], mn[GB], mx[GB];
#pragma unroll
            for (int i = 0; i < S::N; ++i) s[i] = 0.0;
#pragma unroll
            for (int j = 0; j < GB; ++j) { a[j] = 0.0f; mn[j] = __builtin_inff(); mx[j] = -__builtin_inff(); }
            bool bad = false;
            int rows = 0;
            for (int tile = w; tile < p.ntiles; tile += W) {
                if (!single) load_tile(tile);
                rows += tile_rows;
                v16f outs[K];
                RegStack<K, DEPTH> st;
                st.h = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) { st.tos[k] = 0.0f; outs[k] = 0.0f; }
                for (int base = 0; base < len; base += kWave) {
                    const int r = base + lane;
                    uint32_t opv = 0, payv = 0;
                    if (r < len) {
                        const int i = len - 1 - r;
                        const Decoded dn = decode_node(tt[i], tv[i], MO, p.var_len, p.out_len);
                        opv = dn.op; payv = dn.pay;
                    }
                    const int n = len - base < kWave ? len - base : kWave;
                    run_chunk<MO, LEAN, K, DEPTH>(opv, payv, n, st, RegVars<VL, K>{vars}, outs);
                }
                if (tile == w) {   // the pilot: the genes on the unit's first row (lane 0, row 0 of its first tile)
#pragma unroll
                    for (int j = 0; j < GB; ++j) a[j] = bits2f(uni(f2bits(MO ? outs[0][j] : st.tos[0])));
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    double x[GB];
#pragma unroll
                    for (int j = 0; j < GB; ++j) {
                        const float g = MO ? outs[k][j] : st.tos[k];
                        bad |= !finite_f(g);
                        mn[j] = fminf(mn[j], g);
                        mx[j] = fmaxf(mx[j], g);
                        x[j] = valid[k] ? (double)g - (double)a[j] : 0.0;   // (the SHIFTED value is masked: a row past D adds exactly 0)
                    }
                    gene_accumulate<GB>(s, x, valid[k] ? (double)yv[k] - ybar : 0.0);
                }
            }
            gene_park<GB>(part[b][w], s, a, mn, mx, bad, rows, lane);
        }
        __syncthreads();

        // ---- phase 3: one thread per tree merges the waves' partials in wave order and solves ----
        if ((int)threadIdx.x < nb) {
            const int b = threadIdx.x, t = t0 + b;
            const int c = cls_s[b];
            if (c == TREE_OK) {
                gene_finish<GB>(p, t, part[b], p.ntiles < W ? p.ntiles : W);
            } else if (c != TREE_SKIP) {
                gene_store_nan(p, t, c == TREE_DEEP ? bits2f(kSentinelDeep) : c == TREE_HEAVY ? bits2f(kSentinelHeavy) : __builtin_nanf(""),
                               c == TREE_BAD);
                if (c == TREE_DEEP) p.counter[1] = 1u;
                if (c == TREE_HEAVY) p.counter[2] = 1u;
            }
        }
        __syncthreads();   // (the partials and classes are single-buffered: phase 3 is over before the next batch writes them)
        par ^= 1;
    }
}

// ---- 3. the scratch-stack interpreter: one wave per tree, lanes are rows --------------------------------------------------------------
template <int GB>
__global__ __launch_bounds__(64) void sr_genes_general_kernel(GeneParams p, int only_marked) {
    constexpr bool MO = GB > 1;
    using S = GeneSums<GB>;
    __shared__ GeneUnit<GB> unit;
    const int lane = threadIdx.x & 63;
    if (only_marked && uni((int)p.counter[1]) == 0) return;   // no tree was too deep for the register stack
    float stk[kMaxStack + 2];
    float outs[GB];
    const double ybar = p.stats[0];
    auto process = [&](int t) {
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *tt = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int cls = uni(classify_tree(tt, tv, len, MO, p.var_len, p.out_len, kMaxStack));
        if (cls != TREE_OK) {
            if (lane == 0) gene_store_nan(p, t, __builtin_nanf(""), true);
            return;
        }
        double s[S::N];
        float a[GB], mn[GB], mx[GB];
#pragma unroll
        for (int i = 0; i < S::N; ++i) s[i] = 0.0;
#pragma unroll
        for (int j = 0; j < GB; ++j) { a[j] = 0.0f; mn[j] = __builtin_inff(); mx[j] = -__builtin_inff(); outs[j] = 0.0f; }
        bool bad = false;
        for (long long base = 0; base < p.D; base += kWave) {
            const long long d = base + lane;
            const bool valid = d < p.D;
            const size_t dc = valid ? (size_t)d : (size_t)p.D - 1;
            const float r = run_general<MO>(tt, tv, len, p.X + dc * p.var_len, p.var_len, p.out_len, outs, stk);
            if (!MO) outs[0] = r;
            if (base == 0) {
#pragma unroll
                for (int j = 0; j < GB; ++j) a[j] = bits2f(uni(f2bits(outs[j])));
            }
            double x[GB];
#pragma unroll
            for (int j = 0; j < GB; ++j) {
                const float g = outs[j];
                bad |= !finite_f(g);
                mn[j] = fminf(mn[j], g);
                mx[j] = fmaxf(mx[j], g);
                x[j] = valid ? (double)g - (double)a[j] : 0.0;
            }
            gene_accumulate<GB>(s, x, valid ? (double)p.y[dc] - ybar : 0.0);
        }
        gene_park<GB>(unit, s, a, mn, mx, bad, p.D, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) gene_finish<GB>(p, t, &unit, 1);
        __builtin_amdgcn_wave_barrier();
    };
    if (!only_marked) {
        for (long long t = blockIdx.x; t < p.pop; t += gridDim.x) process((int)t);
        return;
    }
    // behind the register kernel: a contiguous chunk of the population per wave, its mark words read 64 at a time (sr_scale_general_kernel)
    const long long chunk = (((long long)p.pop + gridDim.x - 1) / gridDim.x + 63) & ~63ll;   // (64 bits: pop may lie near INT_MAX)
    const long long c0 = blockIdx.x * chunk < p.pop ? blockIdx.x * chunk : p.pop;
    const long long c1 = c0 + chunk < p.pop ? c0 + chunk : p.pop;
    for (long long base = c0; base < c1; base += kWave) {
        const long long t = base + lane;
        const bool hit = t < c1 && f2bits(p.loss[t]) == kSentinelDeep;
        unsigned long long mk = __ballot(hit);
        while (mk) {
            const int b = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            process((int)(base + b));
        }
    }
}

template <int GB, int VL, bool LEAN>
static hipError_t launch_genes(GeneParams p, hipStream_t stream) {
    auto kern = sr_genes_kernel<GB, VL, LEAN>;
    constexpr int K = gene_bucket_k(GB, VL), BATCH = gene_bucket_batch(GB);
    const DeviceInfo &dev = device_info();
    p.ntiles = (int)(((long long)p.D + kWave * K - 1) / (kWave * K));
    const int W = p.ntiles < kGeneWaves ? p.ntiles : kGeneWaves;
    static int per_cu_cache[kGeneWaves + 1] = {0};   // occupancy per block size of THIS instantiation
    int per_cu = per_cu_cache[W];
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, W * 64, 0);
        if (e != hipSuccess) return e;
        if (per_cu < 1) per_cu = 1;
        per_cu_cache[W] = per_cu;
    }
    long blocks = (long)dev.num_cus * per_cu;
    long batch = p.pop / (blocks * 16);   // ~16 batches per workgroup: a short tail, rare atomics
    batch = batch < 4 ? 4 : (batch > BATCH ? BATCH : batch);
    p.batch = (int)batch;
    const long need = (p.pop + batch - 1) / batch;
    if (blocks > need) blocks = need;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(W * 64), 0, stream, p);
    return hipGetLastError();
}

template <int GB>
static int run_genes(GeneParams p, hipStream_t stream) {
    const DeviceInfo &dev = device_info();
    const bool regs = p.var_len <= 32;
    hipError_t e;
    if (regs) {
        e = p.var_len <= 12 ? launch_genes<GB, 12, true>(p, stream) : launch_genes<GB, 32, true>(p, stream);
        if (e != hipSuccess) return (int)e;
        e = p.var_len <= 12 ? launch_genes<GB, 12, false>(p, stream) : launch_genes<GB, 32, false>(p, stream);
        if (e != hipSuccess) return (int)e;
    }
    long blocks = (long)dev.num_cus * (regs ? 4 : 16);
    if (blocks > p.pop) blocks = p.pop;
    hipLaunchKernelGGL(sr_genes_general_kernel<GB>, dim3((unsigned)blocks), dim3(64), 0, stream, p, regs ? 1 : 0);
    return (int)hipGetLastError();
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_gene_fitness(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                         const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                         const float *labels, float *loss, float *coef, double *moments, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu || data_points > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (out_len > EVOGP_GENES_MAX) return EVOGP_E_UNSUPPORTED;
    if (!value || !type || !size || !variables || !labels || !loss || !coef) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    hipError_t e;
    unsigned *stats = acquire_counter(stream, &e);   // 16 bytes: the two doubles of the label statistics
    if (!stats) return (int)e;
    GeneParams p{};
    p.counter = acquire_counter(stream, &e);
    if (!p.counter) return (int)e;
    p.value = value; p.type = type; p.size = size; p.X = variables; p.y = labels; p.loss = loss; p.coef = coef; p.moments = moments;
    p.stats = (const double *)stats;
    p.pop = (int)pop_size; p.D = (int)data_points; p.gp_len = (int)gp_len; p.var_len = (int)var_len; p.out_len = (int)out_len;
    hipLaunchKernelGGL(label_stats_kernel, dim3(1), dim3(kStatsThreads), 0, stream, labels, p.D, (double *)stats);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    return out_len == 1 ? run_genes<1>(p, stream) : out_len == 2 ? run_genes<2>(p, stream) : out_len <= 4 ? run_genes<4>(p, stream)
                                                                                                           : run_genes<8>(p, stream);
}
