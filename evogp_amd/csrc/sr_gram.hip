// sr_gram.hip — the population Gram matrix of single-output SR trees on the float64 matrix cores (gfx950; no counterpart in the
// reference).  include/evogp_hip.h has the contract, DESIGN 3.31 the reasoning, sr_gram_order.hpp the order of summation.
//
// For index[0 .. n): p_i[d] the float32 prediction of tree index[i] on row d (batch_evaluate's bits), v_i[d] = (double)p_i[d] -
// (double)y[d] with `residuals`, else (double)p_i[d];  G[i][j] = sum_d v_i[d] v_j[d];  lin[i] = (sum_d v_i[d], sum_d v_i[d] y[d]).
// A tree is UNUSABLE when it is malformed, when a prediction is not finite, or when its index lies outside the forest: its row and
// column of G and its lin words are NaN.  Decided by flags: a malformed tree enters the matrix pass as a row of zeros, a non-finite
// prediction as 0.
//
// The host loops over SLABS of kGramSlab rows; per slab
//   1. gram_panel_kernel<VL, LEAN>   the register interpreter (interp.hpp run_chunk, 64 x K row tiles): a workgroup per selected tree, its
//                                    waves split the slab's tiles; the float32 predictions go to the workspace panel [n][slab rows], the
//                                    per-tree bad flag comes from a ballot.  LEAN build over every tree, then the FULL build over the
//                                    trees the LEAN one marked (transcendentals)
//      gram_panel_general_kernel     the scratch-stack interpreter (run_general) over the trees marked too deep for the register stack,
//                                    and over every tree at var_len > 32; it fills the same panel rows
//   2. gram_syrk_kernel              the upper-triangle 64 x 64 output blocks J >= I of the (n + 2) x (n + 2) matrix of the n trees and the
//                                    two virtual vectors 1 and y.  A workgroup of four waves (a 32 x 32 quadrant = 2 x 2 matrix-instruction
//                                    tiles each) moves 32-row chunks of its 64 + 64 panel rows and of y through LDS, double-buffered through
//                                    registers, converts to float64 and subtracts y on the way to the operands, and chains
//                                    v_mfma_f64_16x16x4_f64 over a segment.  With many blocks a workgroup owns every segment of the slab and
//                                    adds them to G itself in order; with few (small n) a workgroup owns ONE segment, writes its partial
//                                    block to the workspace, and
//      gram_reduce_kernel            adds the partial blocks in segment order.  Either way the mirror word is written with the word.
//   3. gram_finish_kernel            once, after the last slab: NaN rows and columns and lin words by the flags, `usable`.
// No float atomics, nothing synchronises with the host, the engine allocates nothing; a word is a function of its two trees and the data.
#include "sr_gram_panel.hpp"

namespace evogp {

// (the panel kernels, their parameters and constants: sr_gram_panel.hpp, shared with sr_neigh.hip)
constexpr int kGramDirectBlocks = 512;         // from this many output blocks on a workgroup owns every segment of the slab

__host__ __device__ inline int gram_blocks_side(int n) { return (n + 2 + kGramBlock - 1) / kGramBlock; }
__host__ __device__ inline long gram_blocks(int n) { return (long)gram_blocks_side(n) * (gram_blocks_side(n) + 1) / 2; }

__global__ void gram_init_kernel(GramParams p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < p.n + 2) p.bad[i] = 0;
}

// ---- 2. the matrix pass -------------------------------------------------------------------------------------------------------------------
// where the word of vectors (i, j), i <= j, of the (n + 2)-matrix lives: G, lin (j a virtual vector) or nowhere (i virtual, or padding)
__device__ inline double *gram_word(const GramParams &p, int i, int j) {
    if (i >= p.n || j >= p.n + 2) return nullptr;
    return j < p.n ? p.G + (size_t)i * p.n + j : p.lin + (size_t)i * 2 + (j - p.n);
}
__device__ inline void gram_store(const GramParams &p, int i, int j, double *word, double v) {
    *word = v;
    if (j < p.n && j != i) p.G[(size_t)j * p.n + i] = v;   // the mirror: G equals its transpose by construction
}

// block b of the upper triangle, row-major: (I, J), J >= I
__device__ inline void gram_block(int b, int nb, int *I, int *J) {
    int i = 0;
    while (b >= nb - i) { b -= nb - i; ++i; }
    *I = i;
    *J = i + b;
}

// One workgroup: output block blockIdx.x, the segments [blockIdx.y * spw, + spw) of the slab.  direct: add them to the words themselves
// (first: the words start from 0); else write the one segment's partial block to the workspace.
__global__ __launch_bounds__(kGramWaves * 64, 2) void gram_syrk_kernel(GramParams p, int spw, int direct, int first) {
    __shared__ __align__(16) float v_s[2][2][kGramBlock][kGramLd];   // [buffer][side I / J][vector][row of the chunk]
    __shared__ float y_s[2][kGramChunk];                // what is subtracted from a tree's predictions: y with residuals, else 0
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int wi = w >> 1, wj = w & 1;                  // the wave's 32 x 32 quadrant
    const int m = lane & 15, q = lane >> 4;
    const int nb = gram_blocks_side(p.n);
    int I, J;
    gram_block((int)blockIdx.x, nb, &I, &J);
    const bool diag = I == J;
    const int sb = diag ? 0 : 1;                        // the LDS side the B operand comes from
    const int nseg = (p.rows + kGramSegment - 1) / kGramSegment;
    const int s0 = (int)blockIdx.y * spw;
    const int s1 = s0 + spw < nseg ? s0 + spw : nseg;

    // the global side of the double buffer: 128 vectors x 8 float4 per chunk, four float4 per thread
    float4 pre[4];
    float ypre = 0.0f;
    auto fetch = [&](int r0) {   // the chunk of slab rows [r0, r0 + kGramChunk)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int item = (int)threadIdx.x + k * 256;
            const int vl = item >> 3, c4 = item & 7;
            const int side = vl >> 6;
            const int g = (side ? J : I) * kGramBlock + (vl & 63);
            const int r = r0 + c4 * 4;
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (!(side && diag) && r < p.rows) {
                if (g < p.n) {
                    const float4 x = *(const float4 *)(p.panel + (size_t)g * p.stride + r);   // r + 3 < stride: both are multiples of 4
                    e[0] = x.x; e[1] = x.y; e[2] = x.z; e[3] = x.w;
                } else if (g == p.n) {
                    e[0] = e[1] = e[2] = e[3] = 1.0f;
                } else if (g == p.n + 1 && p.y) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = r + u < p.rows ? p.y[(size_t)p.row0 + r + u] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) e[u] = r + u < p.rows ? e[u] : 0.0f;   // rows past D enter as 0
            }
            pre[k] = make_float4(e[0], e[1], e[2], e[3]);
        }
        if (threadIdx.x < kGramChunk) {
            const int r = r0 + (int)threadIdx.x;
            ypre = p.residuals && r < p.rows ? p.y[(size_t)p.row0 + r] : 0.0f;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int item = (int)threadIdx.x + k * 256;
            const int vl = item >> 3, c4 = item & 7;
            *(float4 *)&v_s[buf][vl >> 6][vl & 63][c4 * 4] = pre[k];
        }
        if (threadIdx.x < kGramChunk) y_s[buf][threadIdx.x] = ypre;
    };

    // a tree's predictions lose y, a virtual vector and the padding do not
    bool sub_a[2], sub_b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        sub_a[t] = I * kGramBlock + wi * 32 + t * 16 + m < p.n;
        sub_b[t] = J * kGramBlock + wj * 32 + t * 16 + m < p.n;
    }

    // the lane's 16 words: tile (ti, tj), register r -> vectors (I 64 + wi 32 + ti 16 + 4 r + q, J 64 + wj 32 + tj 16 + m)
    double tot[2][2][4];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                tot[ti][tj][r] = 0.0;
                if (direct && !first) {
                    const int gi = I * kGramBlock + wi * 32 + ti * 16 + 4 * r + q, gj = J * kGramBlock + wj * 32 + tj * 16 + m;
                    const double *word = gi <= gj ? gram_word(p, gi, gj) : nullptr;
                    if (word) tot[ti][tj][r] = *word;
                }
            }

    for (int s = s0; s < s1; ++s) {
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
                const double yd = (double)y_s[buf][g * kGramGroup + q];
                double a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = (double)v_s[buf][0][wi * 32 + t * 16 + m][g * kGramGroup + q] - (sub_a[t] ? yd : 0.0);
                    b[t] = (double)v_s[buf][sb][wj * 32 + t * 16 + m][g * kGramGroup + q] - (sub_b[t] ? yd : 0.0);
                }
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = gram_step(acc[ti][tj], a[ti], b[tj]);
            }
            if (c + 1 < NCHUNK) stage(buf ^ 1);
            __syncthreads();
        }
        if (direct) {
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tot[ti][tj][r] = gram_add_segment(tot[ti][tj][r], acc[ti][tj][r]);
        } else {   // spw == 1
            double *blk = p.part + ((size_t)s * gram_blocks(p.n) + blockIdx.x) * (kGramBlock * kGramBlock);
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) blk[(wi * 32 + ti * 16 + 4 * r + q) * kGramBlock + wj * 32 + tj * 16 + m] = acc[ti][tj][r];
        }
    }
    if (!direct) return;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = I * kGramBlock + wi * 32 + ti * 16 + 4 * r + q, gj = J * kGramBlock + wj * 32 + tj * 16 + m;
                double *word = gi <= gj ? gram_word(p, gi, gj) : nullptr;
                if (word) gram_store(p, gi, gj, word, tot[ti][tj][r]);
            }
}

// the partial blocks of a slab's segments, added to the words in segment order: a thread per word of a block
__global__ __launch_bounds__(256) void gram_reduce_kernel(GramParams p, int first) {
    const int nb = gram_blocks_side(p.n);
    const int b = (int)(blockIdx.x / (kGramBlock * kGramBlock / 256));
    const int e = (int)(blockIdx.x % (kGramBlock * kGramBlock / 256)) * 256 + (int)threadIdx.x;
    int I, J;
    gram_block(b, nb, &I, &J);
    const int gi = I * kGramBlock + e / kGramBlock, gj = J * kGramBlock + e % kGramBlock;
    double *word = gi <= gj ? gram_word(p, gi, gj) : nullptr;
    const int nseg = (p.rows + kGramSegment - 1) / kGramSegment;
    if (word) {
        double tot = first ? 0.0 : *word;
        for (int s = 0; s < nseg; ++s) tot = gram_add_segment(tot, p.part[((size_t)s * gram_blocks(p.n) + b) * (kGramBlock * kGramBlock) + e]);
        gram_store(p, gi, gj, word, tot);
    }
}

// ---- 3. the flags decide ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gram_finish_kernel(GramParams p) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < (size_t)p.n * p.n) {
        const int i = (int)(k / p.n), j = (int)(k % p.n);
        const double nan = __builtin_nan("");
        const bool bad_i = p.bad[i] != 0;
        if (bad_i || p.bad[j] != 0) p.G[k] = nan;
        if (j == 0) {
            p.usable[i] = bad_i ? 0 : 1;
            if (bad_i) p.lin[2 * i] = p.lin[2 * i + 1] = nan;
        }
    }
}

static int g_gram_stages = 3;   // evogp_hip_debug_sr_gram: bit 0 the panel kernels, bit 1 the matrix kernels

static int gram_stride(unsigned D) { return D >= (unsigned)kGramSlab ? kGramSlab : (int)((D + 3u) & ~3u); }

static int gram_badarg(unsigned n, unsigned data_points) {
    if (n > (unsigned)EVOGP_GRAM_MAX_TREES || data_points == 0 || data_points > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    return EVOGP_OK;
}

// the buffers of the workspace, in one order for the size query and the call
static void gram_carve(Arena &a, GramParams &p, unsigned n, unsigned D) {
    p.stride = gram_stride(D);
    p.panel = a.take<float>((size_t)n * p.stride);
    p.bad = a.take<int>((size_t)n + 2);
    p.mark = a.take<unsigned char>(n);
    const long blocks = gram_blocks((int)n);
    const int nseg = gram_segments((int)D) < kGramSlab / kGramSegment ? gram_segments((int)D) : kGramSlab / kGramSegment;
    p.part = blocks < kGramDirectBlocks ? a.take<double>((size_t)nseg * blocks * kGramBlock * kGramBlock) : nullptr;
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_debug_sr_gram(int stages) {
    if (stages < 0 || stages > 3) return EVOGP_E_BADARG;
    g_gram_stages = stages;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_gram_workspace_bytes(unsigned n, unsigned data_points, unsigned long long *bytes) {
    if (const int rc = gram_badarg(n, data_points)) return rc;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    GramParams p{};
    gram_carve(a, p, n, data_points);
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_gram(unsigned n, unsigned data_points, unsigned var_len, unsigned pop_size, unsigned gp_len, const float *value,
                                 const int16_t *type, const int16_t *size, const float *variables, const float *labels, const int *index,
                                 int residuals, double *gram_out, double *lin_out, unsigned char *usable_out, void *workspace,
                                 evogp_stream_t stream_) {
    if (const int rc = gram_badarg(n, data_points)) return rc;
    if (var_len == 0 || pop_size == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || pop_size > 0x7FFFFFFFu || var_len > 0x7FFFFFFFu ||
        (residuals && !labels))
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables) return EVOGP_E_NULLPTR;
    if (n == 0) return EVOGP_OK;   // empty outputs: nothing to launch, and nothing to point at
    if (!index || !gram_out || !lin_out || !usable_out || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    hipError_t e;
    Arena a{(char *)workspace};
    GramParams p{};
    gram_carve(a, p, n, data_points);
    p.value = value; p.type = type; p.size = size; p.pop = (int)pop_size; p.gp_len = (int)gp_len;
    p.X = variables; p.y = labels; p.index = index; p.G = gram_out; p.lin = lin_out; p.usable = usable_out;
    p.n = (int)n; p.D = (int)data_points; p.var_len = (int)var_len; p.residuals = residuals ? 1 : 0;

    hipLaunchKernelGGL(gram_init_kernel, dim3((n + 2 + 255) / 256), dim3(256), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const long blocks = gram_blocks(p.n);
    const int direct = p.part ? 0 : 1;
    const bool regs = p.var_len <= 32;
    for (long long row0 = 0; row0 < (long long)p.D; row0 += kGramSlab) {
        p.row0 = (int)row0;
        p.rows = (long long)p.D - row0 < kGramSlab ? (int)((long long)p.D - row0) : kGramSlab;
        const int first = row0 == 0 ? 1 : 0;
        if (regs && (g_gram_stages & 1)) {
            e = p.var_len <= 12 ? launch_panel<12, true>(p, stream) : launch_panel<32, true>(p, stream);
            if (e != hipSuccess) return (int)e;
            e = p.var_len <= 12 ? launch_panel<12, false>(p, stream) : launch_panel<32, false>(p, stream);
            if (e != hipSuccess) return (int)e;
        }
        if (g_gram_stages & 1) {
            hipLaunchKernelGGL(gram_panel_general_kernel, dim3(n), dim3(kGramWaves * 64), 0, stream, p, regs ? 0 : 1);
            if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        }
        if (!(g_gram_stages & 2)) continue;
        const int nseg = (p.rows + kGramSegment - 1) / kGramSegment;
        hipLaunchKernelGGL(gram_syrk_kernel, dim3((unsigned)blocks, direct ? 1u : (unsigned)nseg), dim3(kGramWaves * 64), 0, stream, p,
                           direct ? nseg : 1, direct, first);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        if (!direct) {
            hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)(blocks * (kGramBlock * kGramBlock / 256))), dim3(256), 0, stream, p, first);
            if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        }
    }
    const size_t words = (size_t)n * n;
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}
