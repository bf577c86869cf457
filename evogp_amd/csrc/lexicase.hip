// lexicase.hip — per-case SR errors and epsilon-lexicase parent selection (gfx950; no counterpart in the reference).
//
// evogp_hip_sr_case_errors: the batch evaluation (sr_fitness.hip, the interpreters of evogp_hip_batch_evaluate) into an engine-owned
// prediction buffer (one per stream, from the workspace pool of launch.hpp), then one epilogue kernel that reads the (pop, D, out)
// predictions and the labels and writes the CASE-MAJOR errors errors[d][t] = (sum_o delta_o) / out_len through a 64 x 64 LDS tile
// (reads along d, writes along t, both coalesced).
//
// evogp_hip_lexicase_select: semi-dynamic epsilon-lexicase over case-major errors E[n][pop] (include/evogp_hip.h has the contract).
// Five stages, all on the caller's stream, nothing synchronises with the host:
//   1. hash      one thread per tree hashes its key row to 64 bits (a coalesced pass over E)
//   2. classes   a stable radix sort of (hash, tree) pairs (rocPRIM), head marks, two scans: clone classes numbered in ascending order
//                of their smallest tree, each with a representative, a member count and a member list in ascending tree order
//   3. prep      one workgroup per case c: the pool an event starts from when its first case is c, as a list of class ids
//   4. events    one wave per event: the pool in the wave's LDS share while it fits (kLexCap classes), else as a bit mask over the
//                first-pool list in the wave's own slice of the workspace; each step gathers E[c][rep] for the classes still in
//                the pool, takes the minimum and maximum (a step that removes nobody costs one pass) and compacts with ballots
//   5. pick      winners[k] = member (word_k mod S) of the pool listed class by class, S = the members of the pool's classes
// A hash collision merges two classes (probability about pop^2 / 2^65).
#include "evogp_defs.hpp"
#include "group_sort.hpp"
#include "launch.hpp"

namespace evogp {

// ---- case errors ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void case_errors_kernel(const float *pred, const float *y, float *err, unsigned pop, unsigned D,
                                                          unsigned out_len, int mse) {
    __shared__ float tile[64][65];
    const unsigned tx = threadIdx.x & 63u, ty = threadIdx.x >> 6;
    const unsigned t0 = blockIdx.x * 64u;
    const float inv_scale = (float)out_len;
    for (unsigned d0 = blockIdx.y * 64u; d0 < D; d0 += gridDim.y * 64u) {
        for (unsigned tt = ty; tt < 64u; tt += 4u) {
            const unsigned t = t0 + tt, d = d0 + tx;
            if (t < pop && d < D) {
                const float *pr = pred + ((size_t)t * D + d) * out_len;
                const float *yr = y + (size_t)d * out_len;
                float s = 0.0f;
                for (unsigned o = 0; o < out_len; ++o) {
                    const float diff = pr[o] - yr[o];
                    s += mse ? diff * diff : fabsf(diff);
                }
                tile[tt][tx] = s / inv_scale;
            }
        }
        __syncthreads();
        for (unsigned dd = ty; dd < 64u; dd += 4u) {
            const unsigned t = t0 + tx, d = d0 + dd;
            if (t < pop && d < D) err[(size_t)d * pop + t] = tile[tx][dd];
        }
        __syncthreads();
    }
}

// The prediction buffer of a stream: the engine's per-stream workspace pool (launch.hpp StreamWorkspaces), as the tapes of the tape kernels.
static float *case_workspace(hipStream_t stream, size_t bytes, int *rc) { return g_case_workspaces.get(stream, bytes, rc); }

// ---- lexicase selection --------------------------------------------------------------------------------------------------------
constexpr unsigned kLexRowFeistel = (1u << 21);       // words 2^21 + r, r < 4: the round keys of event k's case permutation
constexpr unsigned kLexRowPick = (1u << 21) + 4u;     // word 2^21 + 4: the pick of event k
constexpr unsigned kLexCap = 2048;                    // classes a wave keeps in LDS (8 KiB)
constexpr unsigned kLexWavesPerBlock = 4;
constexpr unsigned kLexMaxWaves = 4096;               // 16 per CU of a 256-CU device

// epsilon of a case: NaN and negative entries count as 0
__device__ inline float lex_eps(float e) { return e > 0.0f ? e : 0.0f; }

__device__ inline unsigned wave_min_u(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ inline unsigned wave_max_u(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ inline unsigned wave_sum_u(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}
__device__ inline unsigned lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// perm_k(j): a 4-round Feistel network on 2 h bits (the smallest even width with 2^(2h) >= n), cycle-walked into [0, n)
__device__ inline unsigned lex_perm(unsigned j, unsigned n, unsigned h, const unsigned *rk) {
    if (n <= 1u) return 0u;
    const unsigned mask = (1u << h) - 1u;
    unsigned x = j;
    do {
        unsigned L = x >> h, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned f = (unsigned)(mix64(((unsigned long long)rk[r] << 32) | R) >> 32) & mask;
            const unsigned t = L ^ f;
            L = R;
            R = t;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}

__global__ __launch_bounds__(256) void lex_hash_kernel(const float *E, unsigned n, unsigned pop, unsigned long long *hash, unsigned *idx) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pop) return;
    unsigned long long h = 0x243F6A8885A308D3ull;
    for (unsigned c = 0; c < n; ++c) {
        const unsigned bits = __float_as_uint(error_key(E[(size_t)c * pop + i]));
        h = mix64((h ^ bits) + 0x9E3779B97F4A7C15ull);
    }
    hash[i] = h;
    idx[i] = i;
}

// over sorted positions s: head marks by tree (for the class numbering) and by position (for the segment starts)
__global__ __launch_bounds__(256) void lex_heads_kernel(const unsigned long long *key, const unsigned *members, unsigned pop, unsigned *flag_t,
                                                        unsigned *head_pos) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= pop) return;
    const bool head = s == 0u || key[s] != key[s - 1u];
    flag_t[members[s]] = head ? 1u : 0u;
    head_pos[s] = head ? s : 0u;
}

// at the last position of every segment: the class's start, representative (its smallest tree) and member count
__global__ __launch_bounds__(256) void lex_classes_kernel(const unsigned long long *key, const unsigned *members, const unsigned *seg,
                                                          const unsigned *flag_t, const unsigned *cls_t, unsigned pop, unsigned *rep,
                                                          unsigned *start, unsigned *count, unsigned *nclass) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= pop) return;
    if (s == pop - 1u) *nclass = cls_t[pop - 1u] + flag_t[pop - 1u];
    if (s + 1u < pop && key[s + 1u] == key[s]) return;
    const unsigned st = seg[s], h = members[st], c = cls_t[h];
    start[c] = st;
    rep[c] = h;
    count[c] = s - st + 1u;
}

struct LexPrep {
    const float *E, *eps;
    const unsigned *rep, *nclass;
    unsigned *fp, *p1;
    unsigned long long *counters;
    unsigned n, pop;
};

// one workgroup per case c: m = min_i key(E[c][i]), then the classes with key <= m + eps[c] (the minimum always stays), ascending
__global__ __launch_bounds__(1024) void lex_prep_kernel(LexPrep q) {
    __shared__ unsigned s_w[16];
    const unsigned c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const float *Ec = q.E + (size_t)c * q.pop;
    unsigned lo = ~0u;
    for (unsigned i = tid; i < q.pop; i += 1024u) lo = min(lo, float_ord(error_key(Ec[i])));
    lo = wave_min_u(lo);
    if (lane == 0) s_w[w] = lo;
    __syncthreads();
    lo = s_w[0];
    for (int k = 1; k < 16; ++k) lo = min(lo, s_w[k]);
    __syncthreads();
    const float m = float_unord(lo), thr = m + lex_eps(q.eps[c]);
    const unsigned C = *q.nclass;
    unsigned *dst = q.fp + (size_t)c * q.pop;
    unsigned out = 0;
    for (unsigned base = 0; base < C; base += 1024u) {
        const unsigned cl = base + tid;
        bool keep = false;
        if (cl < C) {
            const float k = error_key(Ec[q.rep[cl]]);
            keep = k <= thr || k == m;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_w[w] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned before = 0, all = 0;
        for (unsigned k = 0; k < 16u; ++k) {
            const unsigned v = s_w[k];
            all += v;
            before += k < w ? v : 0u;
        }
        if (keep) dst[out + before + lanes_below(bal)] = cl;
        out += all;
        __syncthreads();
    }
    if (tid == 0) {
        q.p1[c] = out;
        if (q.counters) {
            atomicAdd(q.counters + 2, (unsigned long long)out);
            atomicMax(q.counters + 3, (unsigned long long)out);
            atomicAdd(q.counters + 5, 1ull);
            if (c == 0) atomicAdd(q.counters + 4, (unsigned long long)C);
        }
    }
}

struct LexEvents {
    const float *E, *eps;
    const unsigned *members, *rep, *start, *count, *fp, *p1;
    unsigned *bits;
    int *winners;
    unsigned long long *counters;
    unsigned long long base;
    unsigned n, pop, n_events, h, words;
};

__global__ __launch_bounds__(256) void lex_events_kernel(LexEvents p) {
    __shared__ unsigned s_list[kLexWavesPerBlock][kLexCap];
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned *list = s_list[w];
    const unsigned gw = blockIdx.x * kLexWavesPerBlock + w, nw = gridDim.x * kLexWavesPerBlock;
    unsigned *bits = p.bits + (size_t)gw * p.words;
    unsigned long long steps_total = 0;
    for (unsigned k = gw; k < p.n_events; k += nw) {
        unsigned rk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) rk[r] = counter_word(p.base, kLexRowFeistel + (unsigned)r, (unsigned long long)k);
        const unsigned c0 = lex_perm(0u, p.n, p.h, rk);
        const unsigned P1 = p.p1[c0];
        const unsigned *fpl = p.fp + (size_t)c0 * p.pop;
        const unsigned nwords = (P1 + 31u) >> 5;
        bool inlist = P1 <= kLexCap;
        unsigned cnt = P1;
        if (inlist) {
            for (unsigned i = lane; i < P1; i += 64u) list[i] = fpl[i];
        } else {
            for (unsigned wd = lane; wd < nwords; wd += 64u)
                bits[wd] = (wd + 1u < nwords || (P1 & 31u) == 0u) ? ~0u : ((1u << (P1 & 31u)) - 1u);
        }
        __builtin_amdgcn_wave_barrier();
        for (unsigned j = 1; j < p.n && cnt > 1u; ++j) {
            ++steps_total;
            const unsigned c = lex_perm(j, p.n, p.h, rk);
            const float *Ec = p.E + (size_t)c * p.pop;
            unsigned lo = ~0u, hi = 0u;
            if (inlist) {
                for (unsigned i = lane; i < cnt; i += 64u) {
                    const unsigned o = float_ord(error_key(Ec[p.rep[list[i]]]));
                    lo = min(lo, o);
                    hi = max(hi, o);
                }
            } else {
                for (unsigned wd = lane; wd < nwords; wd += 64u) {
                    unsigned b = bits[wd];
                    while (b) {
                        const unsigned q = (unsigned)__builtin_ctz(b);
                        b &= b - 1u;
                        const unsigned o = float_ord(error_key(Ec[p.rep[fpl[wd * 32u + q]]]));
                        lo = min(lo, o);
                        hi = max(hi, o);
                    }
                }
            }
            lo = wave_min_u(lo);
            hi = wave_max_u(hi);
            const float m = float_unord(lo), M = float_unord(hi), thr = m + lex_eps(p.eps[c]);
            if (M <= thr) continue;   // nobody leaves the pool
            if (inlist) {
                unsigned out = 0;
                for (unsigned base = 0; base < cnt; base += 64u) {
                    const unsigned i = base + lane;
                    bool keep = false;
                    unsigned cl = 0;
                    if (i < cnt) {
                        cl = list[i];
                        const float kk = error_key(Ec[p.rep[cl]]);
                        keep = kk <= thr || kk == m;
                    }
                    const unsigned long long bal = __ballot(keep);
                    __builtin_amdgcn_wave_barrier();
                    if (keep) list[out + lanes_below(bal)] = cl;
                    __builtin_amdgcn_wave_barrier();
                    out += (unsigned)__popcll(bal);
                }
                cnt = out;
            } else {
                unsigned mine = 0;
                for (unsigned wd = lane; wd < nwords; wd += 64u) {
                    unsigned b = bits[wd], nb = b;
                    while (b) {
                        const unsigned q = (unsigned)__builtin_ctz(b);
                        b &= b - 1u;
                        const float kk = error_key(Ec[p.rep[fpl[wd * 32u + q]]]);
                        if (!(kk <= thr || kk == m)) nb &= ~(1u << q);
                    }
                    bits[wd] = nb;
                    mine += (unsigned)__popc(nb);
                }
                cnt = wave_sum_u(mine);
                if (cnt <= kLexCap) {   // small enough for LDS: the list in ascending first-pool order, i.e. ascending class id
                    unsigned out = 0;
                    for (unsigned base = 0; base < nwords; base += 64u) {
                        const unsigned wd = base + lane;
                        unsigned b = wd < nwords ? bits[wd] : 0u;
                        const int pc = __popc(b);
                        const int incl = wave_scan_incl(pc);
                        unsigned pos = out + (unsigned)(incl - pc);
                        while (b) {
                            const unsigned q = (unsigned)__builtin_ctz(b);
                            b &= b - 1u;
                            list[pos++] = fpl[wd * 32u + q];
                        }
                        out += (unsigned)__builtin_amdgcn_readlane(incl, 63);
                    }
                    __builtin_amdgcn_wave_barrier();
                    inlist = true;
                }
            }
        }
        // the pick: member (word mod S) of the pool listed class by class
        const unsigned word = counter_word(p.base, kLexRowPick, (unsigned long long)k);
        unsigned winner = 0;
        if (inlist) {
            unsigned tot = 0;
            for (unsigned i = lane; i < cnt; i += 64u) tot += p.count[list[i]];
            const unsigned r = word % wave_sum_u(tot);
            unsigned run = 0;
            for (unsigned base = 0; base < cnt; base += 64u) {
                const unsigned i = base + lane;
                const unsigned cl = i < cnt ? list[i] : 0u, cc = i < cnt ? p.count[cl] : 0u;
                const int incl = wave_scan_incl((int)cc);
                const unsigned before = run + (unsigned)incl - cc;
                const bool here = cc > 0u && r >= before && r < before + cc;
                const unsigned long long bal = __ballot(here);
                if (bal) {
                    const unsigned src = (unsigned)__builtin_ctzll(bal);
                    const unsigned v = here ? p.members[p.start[cl] + (r - before)] : 0u;
                    winner = (unsigned)__shfl((int)v, (int)src, 64);
                    break;
                }
                run += (unsigned)__builtin_amdgcn_readlane(incl, 63);
            }
        } else {
            unsigned tot = 0;
            for (unsigned wd = lane; wd < nwords; wd += 64u) {
                unsigned b = bits[wd];
                while (b) {
                    const unsigned q = (unsigned)__builtin_ctz(b);
                    b &= b - 1u;
                    tot += p.count[fpl[wd * 32u + q]];
                }
            }
            const unsigned r = word % wave_sum_u(tot);
            unsigned run = 0;
            for (unsigned base = 0; base < nwords; base += 64u) {
                const unsigned wd = base + lane;
                const unsigned b0 = wd < nwords ? bits[wd] : 0u;
                unsigned cc = 0;
                for (unsigned b = b0; b; b &= b - 1u) cc += p.count[fpl[wd * 32u + (unsigned)__builtin_ctz(b)]];
                const int incl = wave_scan_incl((int)cc);
                unsigned before = run + (unsigned)incl - cc;
                const bool here = cc > 0u && r >= before && r < before + cc;
                const unsigned long long bal = __ballot(here);
                if (bal) {
                    const unsigned src = (unsigned)__builtin_ctzll(bal);
                    unsigned v = 0;
                    if (here) {
                        for (unsigned b = b0; b; b &= b - 1u) {
                            const unsigned cl = fpl[wd * 32u + (unsigned)__builtin_ctz(b)], n_cl = p.count[cl];
                            if (r < before + n_cl) { v = p.members[p.start[cl] + (r - before)]; break; }
                            before += n_cl;
                        }
                    }
                    winner = (unsigned)__shfl((int)v, (int)src, 64);
                    break;
                }
                run += (unsigned)__builtin_amdgcn_readlane(incl, 63);
            }
        }
        if (lane == 0) p.winners[k] = (int)winner;
        __builtin_amdgcn_wave_barrier();
    }
    if (p.counters && lane == 0 && gw < p.n_events) {
        atomicAdd(p.counters + 0, steps_total);
        atomicAdd(p.counters + 1, (unsigned long long)((p.n_events - gw + nw - 1u) / nw));
    }
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------
struct LexWorkspace {
    unsigned long long *keys_a, *keys_b;
    unsigned *vals_a, *vals_b, *flag_t, *cls_t, *head_pos, *seg, *rep, *start, *count, *nclass, *p1, *fp, *bits;
    void *temp;
    size_t temp_bytes;
    unsigned waves, words;
};

static unsigned lex_waves(unsigned n, unsigned n_events) {
    unsigned long long w = n_events < kLexMaxWaves ? n_events : kLexMaxWaves;
    if (w > 32ull * n) w = 32ull * n;   // the bit-mask slices stay within E's bytes
    if (w < 1) w = 1;
    return (unsigned)((w + kLexWavesPerBlock - 1) / kLexWavesPerBlock * kLexWavesPerBlock);
}

static hipError_t lex_workspace(unsigned n, unsigned pop, unsigned n_events, Arena &a, LexWorkspace *w) {
    hipError_t e;
    w->temp_bytes = 0;
    if ((e = sort_buffers_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = scan_plus_excl_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    if ((e = scan_max_temp(pop, &w->temp_bytes)) != hipSuccess) return e;
    w->waves = lex_waves(n, n_events);
    w->words = (pop + 31u) / 32u;
    w->keys_a = a.take<unsigned long long>(pop); w->keys_b = a.take<unsigned long long>(pop);
    w->vals_a = a.take<unsigned>(pop); w->vals_b = a.take<unsigned>(pop);
    w->flag_t = a.take<unsigned>(pop); w->cls_t = a.take<unsigned>(pop);
    w->head_pos = a.take<unsigned>(pop); w->seg = a.take<unsigned>(pop);
    w->rep = a.take<unsigned>(pop); w->start = a.take<unsigned>(pop); w->count = a.take<unsigned>(pop);
    w->nclass = a.take<unsigned>(1); w->p1 = a.take<unsigned>(n);
    w->fp = a.take<unsigned>((size_t)n * pop);
    w->bits = a.take<unsigned>((size_t)w->waves * w->words);
    w->temp = a.take_bytes(w->temp_bytes);
    return hipSuccess;
}

static unsigned long long *g_lex_counters = nullptr;
static int g_lex_stop = 0;

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_case_errors(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len, int use_mse,
                                        const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                        const float *labels, float *errors, evogp_stream_t stream_) {
    if (pop_size == 0 || data_points == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0 || out_len == 0 ||
        pop_size > 0x7FFFFFFFu)
        return EVOGP_E_BADARG;
    if (!value || !type || !size || !variables || !labels || !errors) return EVOGP_E_NULLPTR;
    if (out_len > 256u) return EVOGP_E_UNSUPPORTED;   // (the batch evaluation's limit, kGeneralOuts)
    const hipStream_t stream = (hipStream_t)stream_;
    int rc = EVOGP_OK;
    float *pred = case_workspace(stream, (size_t)pop_size * data_points * out_len * sizeof(float), &rc);
    if (!pred) return rc;
    rc = evogp_hip_batch_evaluate(pop_size, data_points, gp_len, var_len, out_len, value, type, size, variables, pred, stream_);
    if (rc != EVOGP_OK) return rc;
    const unsigned gy = (data_points + 63u) / 64u;
    hipLaunchKernelGGL(case_errors_kernel, dim3((pop_size + 63u) / 64u, gy < 65535u ? gy : 65535u), dim3(256), 0, stream, pred, labels, errors,
                       pop_size, data_points, out_len, use_mse ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int evogp_hip_lexicase_workspace_bytes(unsigned n_cases, unsigned pop, unsigned n_events, unsigned long long *bytes) {
    if (n_cases == 0 || pop == 0 || pop > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (!bytes) return EVOGP_E_NULLPTR;
    Arena a{nullptr};
    LexWorkspace w;
    const hipError_t e = lex_workspace(n_cases, pop, n_events, a, &w);
    if (e != hipSuccess) return (int)e;
    *bytes = (unsigned long long)a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_lexicase_select(unsigned n_cases, unsigned pop, const float *errors, const float *eps, unsigned n_events, long long seed,
                                         long long generation, int *winners, void *workspace, evogp_stream_t stream_) {
    if (n_cases == 0 || pop == 0 || pop > 0x7FFFFFFFu || n_events > 0x7FFFFFFFu) return EVOGP_E_BADARG;
    if (n_events == 0) return EVOGP_OK;
    if (!errors || !eps || !winners || !workspace) return EVOGP_E_NULLPTR;
    const hipStream_t stream = (hipStream_t)stream_;
    Arena a{(char *)workspace};
    LexWorkspace w;
    hipError_t e = lex_workspace(n_cases, pop, n_events, a, &w);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((pop + 255u) / 256u), block(256);

    // 1-2. hash, sort, classes
    hipLaunchKernelGGL(lex_hash_kernel, grid, block, 0, stream, errors, n_cases, pop, w.keys_a, w.vals_a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    bool in_b;
    if ((e = sort_buffers(w.temp, w.temp_bytes, w.keys_a, w.keys_b, w.vals_a, w.vals_b, pop, &in_b, stream)) != hipSuccess) return (int)e;
    const unsigned long long *key = in_b ? w.keys_b : w.keys_a;
    const unsigned *members = in_b ? w.vals_b : w.vals_a;
    hipLaunchKernelGGL(lex_heads_kernel, grid, block, 0, stream, key, members, pop, w.flag_t, w.head_pos);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = scan_plus_excl(w.temp, w.temp_bytes, w.flag_t, w.cls_t, pop, stream)) != hipSuccess) return (int)e;
    if ((e = scan_max(w.temp, w.temp_bytes, w.head_pos, w.seg, pop, stream)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lex_classes_kernel, grid, block, 0, stream, key, members, (const unsigned *)w.seg, (const unsigned *)w.flag_t,
                       (const unsigned *)w.cls_t, pop, w.rep, w.start, w.count, w.nclass);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (g_lex_stop == 1) return EVOGP_OK;

    // 3. the first pool of every case
    LexPrep q{errors, eps, w.rep, w.nclass, w.fp, w.p1, g_lex_counters, n_cases, pop};
    hipLaunchKernelGGL(lex_prep_kernel, dim3(n_cases), dim3(1024), 0, stream, q);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (g_lex_stop == 2) return EVOGP_OK;

    // 4-5. the events
    unsigned b = 0;
    while (b < 32u && (1ull << b) < n_cases) ++b;
    if (b & 1u) ++b;
    LexEvents ev{errors, eps, members, w.rep, w.start, w.count, w.fp, w.p1, w.bits, winners, g_lex_counters, counter_base(seed, generation),
                 n_cases, pop, n_events, b / 2u, w.words};
    hipLaunchKernelGGL(lex_events_kernel, dim3(w.waves / kLexWavesPerBlock), dim3(64 * kLexWavesPerBlock), 0, stream, ev);
    return (int)hipGetLastError();
}

// Measurement hook (include/evogp_hip_debug.h)
extern "C" int evogp_hip_debug_lexicase(unsigned long long *device_counters, int stop_after) {
    if (stop_after < 0 || stop_after > 2) return EVOGP_E_BADARG;
    g_lex_counters = device_counters;
    g_lex_stop = stop_after;
    return EVOGP_OK;
}
