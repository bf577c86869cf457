// sr_simulate.hip — simulation fitness: a tree as the law of motion of a recurrence or an ODE, stepped T times inside ONE kernel
// (gfx950; no counterpart in the reference, whose rollouts call the one-row forward pass once per step).
//
// include/evogp_hip.h has the definition (evogp_hip_sr_simulate / evogp_hip_sr_simulation_loss).  Time is the inner loop:
//   0. sim_transpose_kernel  u (B, T, U) and target (B, T, SC) -> [t][column][b]: a wave's read of one column at one step is one
//                            coalesced 256-byte load
//   1. sr_simulate_kernel    one workgroup per tree, wave w takes the tiles w, w + W, ... of 64 trajectories, a lane per trajectory.
//                            The tree is classified and pre-decoded ONCE: up to 64 nodes stay in the (opv, payv) VGPR pair for all T
//                            steps, a longer tree's decoded words are staged in LDS once per workgroup and reloaded chunk by chunk
//                            at every interpretation.  The state, the rk4 accumulator and the float64 loss partials live in
//                            registers for all T steps; the tree reads [state | u_t] from ONE register tuple (interp.hpp TupleVars)
//                            that the few instructions of the scheme rewrite between two interpretations; the loads of step t + 1
//                            are issued before step t is interpreted.  Launched twice as sr_scale.hip's pair: the LEAN build over
//                            every tree, the FULL build over the trees the LEAN one marked as using a transcendental function or
//                            pow.  A wave whose trajectories are all dead leaves the time loop.
//   2. sr_simulate_general_kernel   a wave per tree for the trees marked too deep for the 16-entry register stack: run_general
//                            on the LDS-column stack (rows of up to 126 words) or on the scratch stack (longer rows); it leaves at
//                            once when nothing was marked.
// The loss has ONE order of summation whatever kernel takes the tree: a lane adds the float64 terms of its trajectory in time order,
// the 64 lanes of a tile are added by the fixed butterfly (wave_sum_d), the tiles in index order.  No float atomics.
#include "interp.hpp"
#include "launch.hpp"
#include "sr_moments.hpp"

namespace evogp {

constexpr int kSimWaves = 4;            // waves per workgroup: the tiles of one tree
constexpr int kSimDepth = 16;           // register stack entries; deeper trees go to the general kernel
constexpr int kSimMaxState = EVOGP_SIM_MAX_STATE;
constexpr int kSimMaxVars = 32;
constexpr int kSimFoldMaxLen = 126;     // (gp_len + 2) * 256 B of LDS for the column stack: 32 KB

struct SimParams {
    const float *value;
    const int16_t *type;
    const int16_t *size;
    const float *x0;      // [B][S]
    const float *ut;      // [T][U][B]  (sim_transpose_kernel)
    const float *tt;      // [T][SC][B] (the loss only)
    float *states;        // [pop][B][T][S], or nullptr: the loss
    double *loss;         // [pop][SC], or nullptr: the states
    int *cls;             // [pop]: TreeClass as the LEAN pass saw it; the FULL pass turns TREE_HEAVY into TREE_DEEP where it applies
    unsigned *flags;      // [1] != 0: some tree is TREE_DEEP, [2] != 0: some tree is TREE_HEAVY
    int pop, gp_len, B, T, S, U, SC, ntiles, scheme;
    float dt, h2, h6;
};

// ---- 0. the transposition ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sim_transpose_kernel(const float *u, float *ut, int U, const float *target, float *tt, int SC, int B, int T) {
    const size_t nu = (size_t)B * T * U, nt = target ? (size_t)B * T * SC : 0;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < nu + nt; o += (size_t)gridDim.x * blockDim.x) {
        const bool first = o < nu;
        const size_t e = first ? o : o - nu;
        const int C = first ? U : SC;
        const size_t b = e % (size_t)B, r = e / (size_t)B, c = r % (size_t)C, t = r / (size_t)C;
        const size_t from = (b * T + t) * C + c;
        if (first) ut[e] = u[from];
        else tt[e] = target[from];
    }
}

__device__ inline void sim_store_nan(const SimParams &p, int t) {
    const float nan = __builtin_nanf("");
    const size_t n = (size_t)p.B * p.T * p.S;
    if (p.states)
        for (size_t i = threadIdx.x; i < n; i += blockDim.x) p.states[(size_t)t * n + i] = nan;
    if (p.loss && (int)threadIdx.x < p.SC) p.loss[(size_t)t * p.SC + threadIdx.x] = __builtin_nan("");
}

// ---- 1. the register interpreter with time as the inner loop ---------------------------------------------------------------------------
template <int VL, bool MO, bool LEAN, int SCHEME>
__global__ __launch_bounds__(kSimWaves * 64) void sr_simulate_kernel(SimParams p) {
    using VARS = typename VecOf<VL>::type;
    constexpr bool NARX = SCHEME == EVOGP_SIM_NARX, RK4 = SCHEME == EVOGP_SIM_RK4;
    constexpr int NS = (MO || NARX) ? kSimMaxState : 1;   // state registers
    constexpr int NK = MO ? kSimMaxState : 1;             // values of one interpretation
    constexpr int NSTAGE = RK4 ? 4 : 1;
    __shared__ uint32_t dec_s[2][kMaxStack];              // a tree of more than 64 nodes, decoded once: handler ids, payloads, in execution order
    __shared__ double part_s[2][kSimWaves][kSimMaxState]; // the tile sums of one round of tiles, double-buffered by round parity
    __shared__ int dead_s[2][kSimWaves];

    if (!LEAN && uni((int)p.flags[2]) == 0) return;   // the LEAN pass marked nothing
    const int lane = threadIdx.x & 63;
    const int w = uni((int)(threadIdx.x >> 6));
    const int W = blockDim.x >> 6;
    const int S = p.S, SC = p.SC, T = p.T, B = p.B;
    const int var_len = S + p.U, out_len = MO ? S : 1;
    const float nan = __builtin_nanf("");

    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        if (!LEAN && uni(p.cls[t]) != TREE_HEAVY) continue;
        const size_t row = (size_t)t * p.gp_len;
        const float *tv = p.value + row;
        const int16_t *ty = p.type + row;
        int len = uni((int)p.size[row]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        const int c = uni(classify_tree(ty, tv, len, MO, var_len, out_len, kSimDepth, LEAN ? 1 : 0));   // (every wave: the same answer)
        if (LEAN && threadIdx.x == 0) p.cls[t] = c;
        if (c != TREE_OK) {
            if (c == TREE_BAD) sim_store_nan(p, t);
            else if (threadIdx.x == 0) {
                if (c == TREE_DEEP) { p.cls[t] = TREE_DEEP; p.flags[1] = 1u; }
                else p.flags[2] = 1u;
            }
            continue;
        }

        // ---- decode once per tree ----
        uint32_t opv = 0, payv = 0;
        const bool in_regs = len <= kWave;
        if (in_regs) {
            if (lane < len) {
                const int i = len - 1 - lane;
                const Decoded dn = decode_node(ty[i], tv[i], MO, var_len, out_len);
                opv = dn.op; payv = dn.pay;
            }
        } else {
            for (int r = threadIdx.x; r < len; r += blockDim.x) {
                const int i = len - 1 - r;
                const Decoded dn = decode_node(ty[i], tv[i], MO, var_len, out_len);
                dec_s[0][r] = dn.op; dec_s[1][r] = dn.pay;
            }
            __syncthreads();
        }
        auto interpret = [&](const VARS &tup, float (&k)[NK]) {
            RegStack<1, kSimDepth> st;
            st.h = 0;
            st.tos[0] = 0.0f;
            v16f outs[1];
            if (MO) outs[0] = 0.0f;
            for (int base = 0; base < len; base += kWave) {
                uint32_t o = opv, q = payv;
                if (!in_regs) {
                    const int r = base + lane;
                    o = r < len ? dec_s[0][r] : 0u;
                    q = r < len ? dec_s[1][r] : 0u;
                }
                const int n = len - base < kWave ? len - base : kWave;
                run_chunk<MO, LEAN, 1, kSimDepth>(o, q, n, st, TupleVars<VL>{tup}, outs);
            }
            if (MO) {
#pragma unroll
                for (int s = 0; s < NK; ++s) k[s] = outs[0][s];
            } else {
                k[0] = st.tos[0];
            }
        };

        double tot = 0.0;   // thread s < SC: the sum of state s over the tiles so far, in index order
        int any_dead = 0;
        const int rounds = (p.ntiles + W - 1) / W;
        for (int r = 0; r < rounds; ++r) {
            const int tile = r * W + w, par = r & 1;
            if (tile < p.ntiles) {
                const long long b = (long long)tile * kWave + lane;
                const bool valid = b < B;
                const size_t bc = (size_t)(valid ? b : B - 1);   // lanes past the end repeat the last trajectory: they die with it
                float x[NS], tg[NS], tgn[NS];
                double acc[NS];
                VARS tup, nxt;
#pragma unroll
                for (int v = 0; v < VL; ++v) { tup[v] = 0.0f; nxt[v] = 0.0f; }
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    x[s] = s < S ? p.x0[bc * S + s] : 0.0f;
                    acc[s] = 0.0; tg[s] = 0.0f; tgn[s] = 0.0f;
                }
                auto load_step = [&](int ts) {
#pragma unroll
                    for (int v = 0; v < VL; ++v)
                        if (v >= S && v < var_len) nxt[v] = p.ut[((size_t)ts * p.U + (v - S)) * B + bc];
                    if (p.tt) {
#pragma unroll
                        for (int s = 0; s < NS; ++s)
                            if (s < SC) tgn[s] = p.tt[((size_t)ts * SC + s) * B + bc];
                    }
                };
                load_step(0);
                bool alive = true;
                int ts = 0;
                for (; ts < T; ++ts) {
#pragma unroll
                    for (int v = 0; v < VL; ++v)
                        if (v >= S && v < var_len) tup[v] = nxt[v];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        tg[s] = tgn[s];
                        if (s < S) tup[s] = x[s];
                    }
                    if (ts + 1 < T) load_step(ts + 1);   // in flight while this step is interpreted
                    float xn[NS], sum[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) { xn[s] = 0.0f; sum[s] = 0.0f; }
#pragma unroll 1
                    for (int stage = 0; stage < NSTAGE; ++stage) {
                        float k[NK];
                        interpret(tup, k);
                        if constexpr (SCHEME == EVOGP_SIM_MAP) {
#pragma unroll
                            for (int s = 0; s < NS; ++s) xn[s] = k[s];
                        } else if constexpr (SCHEME == EVOGP_SIM_EULER) {
#pragma unroll
                            for (int s = 0; s < NS; ++s) xn[s] = __fadd_rn(x[s], __fmul_rn(p.dt, k[s]));
                        } else if constexpr (NARX) {
                            xn[0] = k[0];
#pragma unroll
                            for (int s = 1; s < NS; ++s) xn[s] = x[s - 1];
                        } else {
                            const float h = stage == 2 ? p.dt : p.h2;
#pragma unroll
                            for (int s = 0; s < NS; ++s) {
                                const float ks = k[s < NK ? s : 0];
                                sum[s] = stage == 0 ? ks : __fadd_rn(sum[s], stage == 3 ? ks : __fmul_rn(2.0f, ks));
                                if (stage < 3) { if (s < S) tup[s] = __fadd_rn(x[s], __fmul_rn(h, ks)); }
                                else xn[s] = __fadd_rn(x[s], __fmul_rn(p.h6, sum[s]));
                            }
                        }
                    }
                    bool fin = true;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        if (s < S) fin = fin && finite_f(xn[s]);
                        x[s] = xn[s];
                    }
                    alive = alive && fin;
                    if (p.states) {
                        if (valid) {
                            float *out = p.states + (((size_t)t * B + (size_t)b) * T + ts) * S;
#pragma unroll
                            for (int s = 0; s < NS; ++s)
                                if (s < S) out[s] = alive ? xn[s] : nan;
                        }
                    } else if (alive && valid) {
#pragma unroll
                        for (int s = 0; s < NS; ++s)
                            if (s < SC) {
                                const double d = (double)xn[s] - (double)tg[s];
                                acc[s] += d * d;
                            }
                    }
                    if (!__any(alive)) { ++ts; break; }   // every trajectory of the tile is dead: the result is decided
                }
                if (p.states) {
                    if (valid)
                        for (; ts < T; ++ts) {
                            float *out = p.states + (((size_t)t * B + (size_t)b) * T + ts) * S;
                            for (int s = 0; s < S; ++s) out[s] = nan;
                        }
                } else {
                    const bool dead = __any(!alive) != 0;
#pragma unroll
                    for (int s = 0; s < NS; ++s)
                        if (s < SC) {
                            const double sum_s = wave_sum_d(acc[s]);
                            if (lane == 0) part_s[par][w][s] = sum_s;
                        }
                    if (lane == 0) dead_s[par][w] = dead ? 1 : 0;
                }
            }
            if (p.loss) {
                __syncthreads();
                if ((int)threadIdx.x < SC) {
                    const int left = p.ntiles - r * W;
                    const int nw = left < W ? left : W;
                    for (int i = 0; i < nw; ++i) {
                        tot += part_s[par][i][threadIdx.x];
                        any_dead |= dead_s[par][i];
                    }
                }
            }
        }
        if (p.loss && (int)threadIdx.x < SC)
            p.loss[(size_t)t * SC + threadIdx.x] = any_dead ? __builtin_nan("") : tot / ((double)B * (double)T);
        __syncthreads();   // dec_s and part_s are rewritten for the next tree
    }
}

// ---- 2. the stack interpreter: one wave per tree, the scheme a runtime switch ----------------------------------------------------------
// STRIDE 64: the operand stack is the lane's column of an LDS block [gp_len + 2][64]; STRIDE 1: a private array (rows of more than
// kSimFoldMaxLen words, whose columns LDS does not hold).
template <bool MO, int STRIDE>
__global__ __launch_bounds__(64) void sr_simulate_general_kernel(SimParams p) {
    extern __shared__ float sim_stack_lds[];
    if (uni((int)p.flags[1]) == 0) return;   // no tree was too deep for the register stack
    const int lane = threadIdx.x & 63;
    float stk_priv[STRIDE == 1 ? kMaxStack + 2 : 1];
    float *const stk = STRIDE == 1 ? stk_priv : sim_stack_lds + lane;
    const int S = p.S, SC = p.SC, T = p.T, B = p.B, scheme = p.scheme;
    const int var_len = S + p.U, out_len = MO ? S : 1;
    const float nan = __builtin_nanf("");
    for (int t = blockIdx.x; t < p.pop; t += gridDim.x) {
        if (uni(p.cls[t]) != TREE_DEEP) continue;
        const size_t trow = (size_t)t * p.gp_len;
        const float *tv = p.value + trow;
        const int16_t *ty = p.type + trow;
        int len = uni((int)p.size[trow]);
        len = len < 0 ? 0 : (len > p.gp_len ? p.gp_len : len);
        if (uni(classify_tree(ty, tv, len, MO, var_len, out_len, kMaxStack)) != TREE_OK) {
            sim_store_nan(p, t);
            continue;
        }
        double tot[kSimMaxState];
        for (int s = 0; s < kSimMaxState; ++s) tot[s] = 0.0;
        bool any_dead = false;
        for (int tile = 0; tile < p.ntiles; ++tile) {
            const long long b = (long long)tile * kWave + lane;
            const bool valid = b < B;
            const size_t bc = (size_t)(valid ? b : B - 1);
            float x[kSimMaxState], xn[kSimMaxState], sum[kSimMaxState], k[kSimMaxState], rowv[kSimMaxVars];
            double acc[kSimMaxState];
            for (int s = 0; s < kSimMaxState; ++s) {
                x[s] = s < S ? p.x0[bc * S + s] : 0.0f;
                xn[s] = 0.0f; sum[s] = 0.0f; k[s] = 0.0f; acc[s] = 0.0;
            }
            bool alive = true;
            int ts = 0;
            for (; ts < T; ++ts) {
                for (int s = 0; s < S; ++s) rowv[s] = x[s];
                for (int v = S; v < var_len; ++v) rowv[v] = p.ut[((size_t)ts * p.U + (v - S)) * B + bc];
                const int nstage = scheme == EVOGP_SIM_RK4 ? 4 : 1;
                for (int stage = 0; stage < nstage; ++stage) {
                    const float root = run_general<MO, STRIDE>(ty, tv, len, rowv, var_len, out_len, k, stk);
                    if (!MO) k[0] = root;
                    if (scheme == EVOGP_SIM_MAP) {
                        for (int s = 0; s < S; ++s) xn[s] = k[s];
                    } else if (scheme == EVOGP_SIM_EULER) {
                        for (int s = 0; s < S; ++s) xn[s] = __fadd_rn(x[s], __fmul_rn(p.dt, k[s]));
                    } else if (scheme == EVOGP_SIM_NARX) {
                        xn[0] = k[0];
                        for (int s = 1; s < S; ++s) xn[s] = x[s - 1];
                    } else {
                        const float h = stage == 2 ? p.dt : p.h2;
                        for (int s = 0; s < S; ++s) {
                            sum[s] = stage == 0 ? k[s] : __fadd_rn(sum[s], stage == 3 ? k[s] : __fmul_rn(2.0f, k[s]));
                            if (stage < 3) rowv[s] = __fadd_rn(x[s], __fmul_rn(h, k[s]));
                            else xn[s] = __fadd_rn(x[s], __fmul_rn(p.h6, sum[s]));
                        }
                    }
                }
                bool fin = true;
                for (int s = 0; s < S; ++s) { fin = fin && finite_f(xn[s]); x[s] = xn[s]; }
                alive = alive && fin;
                if (p.states) {
                    if (valid) {
                        float *out = p.states + (((size_t)t * B + (size_t)b) * T + ts) * S;
                        for (int s = 0; s < S; ++s) out[s] = alive ? xn[s] : nan;
                    }
                } else if (alive && valid) {
                    for (int s = 0; s < SC; ++s) {
                        const double d = (double)xn[s] - (double)p.tt[((size_t)ts * SC + s) * B + bc];
                        acc[s] += d * d;
                    }
                }
                if (!__any(alive)) { ++ts; break; }
            }
            if (p.states) {
                if (valid)
                    for (; ts < T; ++ts) {
                        float *out = p.states + (((size_t)t * B + (size_t)b) * T + ts) * S;
                        for (int s = 0; s < S; ++s) out[s] = nan;
                    }
            } else {
                any_dead = any_dead || __any(!alive) != 0;
                for (int s = 0; s < SC; ++s) tot[s] += wave_sum_d(acc[s]);
            }
        }
        if (p.loss && lane == 0)
            for (int s = 0; s < SC; ++s) p.loss[(size_t)t * SC + s] = any_dead ? __builtin_nan("") : tot[s] / ((double)B * (double)T);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
template <int VL, bool MO, int SCHEME>
static hipError_t launch_sim_pair(const SimParams &p, unsigned blocks, unsigned threads, hipStream_t stream) {
    hipLaunchKernelGGL((sr_simulate_kernel<VL, MO, true, SCHEME>), dim3(blocks), dim3(threads), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((sr_simulate_kernel<VL, MO, false, SCHEME>), dim3(blocks), dim3(threads), 0, stream, p);
    return hipGetLastError();
}

template <int VL>
static hipError_t launch_sim_width(const SimParams &p, bool mo, unsigned blocks, unsigned threads, hipStream_t stream) {
    switch (p.scheme) {
    case EVOGP_SIM_MAP: return mo ? launch_sim_pair<VL, true, EVOGP_SIM_MAP>(p, blocks, threads, stream) : launch_sim_pair<VL, false, EVOGP_SIM_MAP>(p, blocks, threads, stream);
    case EVOGP_SIM_EULER: return mo ? launch_sim_pair<VL, true, EVOGP_SIM_EULER>(p, blocks, threads, stream) : launch_sim_pair<VL, false, EVOGP_SIM_EULER>(p, blocks, threads, stream);
    case EVOGP_SIM_RK4: return mo ? launch_sim_pair<VL, true, EVOGP_SIM_RK4>(p, blocks, threads, stream) : launch_sim_pair<VL, false, EVOGP_SIM_RK4>(p, blocks, threads, stream);
    default: return launch_sim_pair<VL, false, EVOGP_SIM_NARX>(p, blocks, threads, stream);
    }
}

static int sim_check(unsigned pop, unsigned gp_len, unsigned B, unsigned T, unsigned S, unsigned U, int scheme) {
    if (pop == 0 || gp_len == 0 || gp_len > (unsigned)kMaxStack || B == 0 || T == 0 || T > 65535u || S == 0 || S > (unsigned)kSimMaxState ||
        U > (unsigned)kSimMaxVars || S + U > (unsigned)kSimMaxVars || scheme < EVOGP_SIM_MAP || scheme > EVOGP_SIM_NARX || pop > 0x7FFFFFFFu ||
        B > 0x7FFFFFFFu || (unsigned long long)B * T > 0x7FFFFFFFull)
        return EVOGP_E_BADARG;
    return EVOGP_OK;
}

static void sim_workspace(Arena &a, unsigned pop, unsigned B, unsigned T, unsigned U, unsigned SC, float **ut, float **tt, int **cls) {
    *ut = a.take<float>((size_t)B * T * U);
    *tt = a.take<float>((size_t)B * T * SC);   // (SC == 0: the states op has no target)
    *cls = a.take<int>(pop);
}

static int sim_run(unsigned pop, unsigned gp_len, unsigned B, unsigned T, unsigned S, unsigned U, int scheme, float dt, float h2, float h6,
                   const float *value, const int16_t *type, const int16_t *size, const float *x0, const float *u, const float *target,
                   float *states, double *loss, void *workspace, hipStream_t stream) {
    const unsigned SC = loss ? (scheme == EVOGP_SIM_NARX ? 1u : S) : 0u;
    SimParams p{};
    float *ut, *tt;
    Arena a{(char *)workspace};
    sim_workspace(a, pop, B, T, U, SC, &ut, &tt, &p.cls);
    hipError_t e;
    p.flags = acquire_counter(stream, &e);
    if (!p.flags) return (int)e;
    p.value = value; p.type = type; p.size = size; p.x0 = x0; p.ut = ut; p.tt = loss ? tt : nullptr; p.states = states; p.loss = loss;
    p.pop = (int)pop; p.gp_len = (int)gp_len; p.B = (int)B; p.T = (int)T; p.S = (int)S; p.U = (int)U; p.SC = (int)SC;
    p.ntiles = (int)((B + kWave - 1) / kWave); p.scheme = scheme; p.dt = dt; p.h2 = h2; p.h6 = h6;
    const DeviceInfo &dev = device_info();
    const size_t moved = (size_t)B * T * (U + SC);
    if (moved) {
        size_t tb = (moved + 255) / 256;
        if (tb > (size_t)dev.num_cus * 16) tb = (size_t)dev.num_cus * 16;
        hipLaunchKernelGGL(sim_transpose_kernel, dim3((unsigned)tb), dim3(256), 0, stream, u, ut, (int)U, loss ? target : nullptr, tt, (int)SC, (int)B, (int)T);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    const bool mo = scheme != EVOGP_SIM_NARX && S > 1;
    const unsigned threads = (unsigned)(p.ntiles < kSimWaves ? p.ntiles : kSimWaves) * 64u;
    long blocks = (long)dev.num_cus * 64;
    if (blocks > (long)pop) blocks = (long)pop;
    const unsigned vl = S + U;
    e = vl <= 9 ? launch_sim_width<9>(p, mo, (unsigned)blocks, threads, stream)
      : vl <= 10 ? launch_sim_width<10>(p, mo, (unsigned)blocks, threads, stream)
      : vl <= 12 ? launch_sim_width<12>(p, mo, (unsigned)blocks, threads, stream)
      : vl <= 16 ? launch_sim_width<16>(p, mo, (unsigned)blocks, threads, stream)
                 : launch_sim_width<32>(p, mo, (unsigned)blocks, threads, stream);
    if (e != hipSuccess) return (int)e;
    long gblocks = (long)dev.num_cus * 8;
    if (gblocks > (long)pop) gblocks = (long)pop;
    if (gp_len <= (unsigned)kSimFoldMaxLen) {
        const size_t lds = (size_t)(gp_len + 2) * kWave * sizeof(float);
        if (mo) hipLaunchKernelGGL((sr_simulate_general_kernel<true, 64>), dim3((unsigned)gblocks), dim3(64), lds, stream, p);
        else hipLaunchKernelGGL((sr_simulate_general_kernel<false, 64>), dim3((unsigned)gblocks), dim3(64), lds, stream, p);
    } else {
        if (mo) hipLaunchKernelGGL((sr_simulate_general_kernel<true, 1>), dim3((unsigned)gblocks), dim3(64), 0, stream, p);
        else hipLaunchKernelGGL((sr_simulate_general_kernel<false, 1>), dim3((unsigned)gblocks), dim3(64), 0, stream, p);
    }
    return (int)hipGetLastError();
}

}  // namespace evogp

using namespace evogp;

extern "C" int evogp_hip_sr_simulate_workspace_bytes(unsigned pop_size, unsigned trajectories, unsigned steps, unsigned state_len, unsigned input_len,
                                                     int scheme, int with_target, unsigned long long *bytes) {
    if (!bytes) return EVOGP_E_NULLPTR;
    const int rc = sim_check(pop_size, 1, trajectories, steps, state_len, input_len, scheme);
    if (rc != EVOGP_OK) return rc;
    Arena a{nullptr};
    float *ut, *tt;
    int *cls;
    sim_workspace(a, pop_size, trajectories, steps, input_len, with_target ? (scheme == EVOGP_SIM_NARX ? 1u : state_len) : 0u, &ut, &tt, &cls);
    *bytes = a.off;
    return EVOGP_OK;
}

extern "C" int evogp_hip_sr_simulate(unsigned pop_size, unsigned gp_len, unsigned trajectories, unsigned steps, unsigned state_len, unsigned input_len,
                                     int scheme, float dt, float h2, float h6, const float *value, const int16_t *type, const int16_t *size,
                                     const float *x0, const float *u, float *states_out, void *workspace, evogp_stream_t stream) {
    const int rc = sim_check(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme);
    if (rc != EVOGP_OK) return rc;
    if ((unsigned long long)pop_size * trajectories * steps * state_len * sizeof(float) > (1ull << 31)) return EVOGP_E_BADARG;
    if (!value || !type || !size || !x0 || (!u && input_len) || !states_out || !workspace) return EVOGP_E_NULLPTR;
    return sim_run(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme, dt, h2, h6, value, type, size, x0, u, nullptr, states_out,
                   nullptr, workspace, (hipStream_t)stream);
}

extern "C" int evogp_hip_sr_simulation_loss(unsigned pop_size, unsigned gp_len, unsigned trajectories, unsigned steps, unsigned state_len,
                                            unsigned input_len, int scheme, float dt, float h2, float h6, const float *value, const int16_t *type,
                                            const int16_t *size, const float *x0, const float *u, const float *target, double *loss_out,
                                            void *workspace, evogp_stream_t stream) {
    const int rc = sim_check(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme);
    if (rc != EVOGP_OK) return rc;
    if (!value || !type || !size || !x0 || (!u && input_len) || !target || !loss_out || !workspace) return EVOGP_E_NULLPTR;
    return sim_run(pop_size, gp_len, trajectories, steps, state_len, input_len, scheme, dt, h2, h6, value, type, size, x0, u, target, nullptr, loss_out,
                   workspace, (hipStream_t)stream);
}
