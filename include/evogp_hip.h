/*
 * evogp_hip.h — C ABI of the MI355X (gfx950) tree-evaluation / genetic-operation engine.
 *
 * This is the drop-in boundary.  Each entry point replaces one of the five host launchers
 * the reference declares in  src/evogp/cuda/kernel.h:23-97  and calls from
 * src/evogp/cuda/torch_wrapper.cu  (generate :68, mutate :121, crossover :173,
 * evaluate :220, SR_fitness :267).  Argument order, meaning and units are the
 * reference's; the differences are deliberate and minimal:
 *
 *   - every function takes the HIP stream to enqueue on as its last argument
 *     (the reference uses the legacy default stream, SURVEY.md §8b "Threading / streams");
 *   - every function returns an int: 0 on success, a hipError_t value when the launch
 *     failed, or a negative EVOGP_E_* code for an argument the kernels cannot honour
 *     (the reference's launchers return void and never check, torch_wrapper.cu:84,135,188,231,282);
 *   - evogp_hip_generate has one extra argument, tree_index_offset, added to the
 *     tree index before it is hashed into the per-tree RNG seed (reference: generate.cu:35,40
 *     uses the local thread index).  0 reproduces the reference; a rank offset makes a
 *     population sharded over several GPUs bit-identical to the single-GPU one.
 *
 * All pointers are DEVICE pointers (HBM), row-major, contiguous, exactly the layouts of
 * the reference's Forest tensors (src/evogp/tree/forest.py:13-40):
 *     value  float32 [pop][gp_len]   node payload (var index / constant / function id / OUT bits)
 *     type   int16   [pop][gp_len]   NodeType, bit 7 = OUT_NODE
 *     size   int16   [pop][gp_len]   subtree size, size[t][0] = live length of tree t
 * Output rows are written on [0, len) and zero-filled on [len, gp_len) (the reference leaves
 * the tail uninitialised: torch_wrapper.cu:64-66, generate.cu:167-172).  Words of an INPUT row behind
 * size[t][0] may hold anything, and no result depends on them; where a function copies a row "as it is"
 * or "unchanged", those words travel with it (tests/forest_invariance.py).
 *
 * No torch types, no C++ types: this header is plain C and is what a cgo / JNI / ctypes /
 * libtorch binding includes (INTEGRATION.md shows the libtorch and ctypes stubs).
 */
#ifndef EVOGP_HIP_H
#define EVOGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* encodings shared with the reference (src/evogp/cuda/defs.h:5-57) */
#define EVOGP_MAX_STACK 1024      /* defs.h:5  — upper bound on gp_len                     */
#define EVOGP_MAX_FULL_DEPTH 10   /* defs.h:5  — length of depth2leaf_probs                */
#define EVOGP_NUM_FUNCS 29        /* defs.h:56 — Function::END, length of roulette_funcs   */
#define EVOGP_LM_MAX_CONSTS 8     /* K: constants per tree evogp_hip_sr_normal_eq / evogp_hip_sr_lm_step optimise */
#define EVOGP_LM_NORMAL_WORDS (EVOGP_LM_MAX_CONSTS * (EVOGP_LM_MAX_CONSTS + 1) / 2 + EVOGP_LM_MAX_CONSTS) /* 44: a row of `normal` */

/* negative return codes (argument errors detected on the host before any launch) */
#define EVOGP_E_BADARG (-1)       /* size/shape argument out of the range the reference's wrapper accepts */
#define EVOGP_E_NULLPTR (-2)      /* a required pointer is NULL */
#define EVOGP_E_UNSUPPORTED (-3)  /* var_len/out_len larger than the interpreter's staging area */

typedef void *evogp_stream_t; /* a hipStream_t; NULL = the null stream */

/* kernel.h:23-38 `generate`.  keys: u32[2]; depth2leaf_probs: f32[10]; roulette_funcs: f32[29]
 * (cumulative); const_samples: f32[const_samples_len].  Outputs: [pop_size][gp_len]. */
int evogp_hip_generate(unsigned pop_size, unsigned gp_len, unsigned var_len, unsigned out_len,
                       unsigned const_samples_len, float out_prob, float const_prob,
                       const unsigned *keys, const float *depth2leaf_probs,
                       const float *roulette_funcs, const float *const_samples,
                       float *value_res, int16_t *type_res, int16_t *size_res,
                       unsigned tree_index_offset, evogp_stream_t stream);

/* kernel.h:40-53 `mutate`.  out[n] = old[n] with the subtree at mutate_indices[n] replaced by the
 * whole tree new[n]; old[n] is copied when the index is outside [0, len(old[n])) or the result
 * would exceed gp_len (mutation.cu:150-160,170-180). */
int evogp_hip_mutate(int pop_size, int gp_len,
                     const float *value_ori, const int16_t *type_ori, const int16_t *size_ori,
                     const int *mutate_indices,
                     const float *value_new, const int16_t *type_new, const int16_t *size_new,
                     float *value_res, int16_t *type_res, int16_t *size_res,
                     evogp_stream_t stream);

/* kernel.h:55-69 `crossover`.  out[n] = ori[left_idx[n]] with the subtree at left_node_idx[n]
 * replaced by subtree right_node_idx[n] of ori[right_idx[n]]; the left tree is copied when
 * right_idx[n] is outside [0, pop_size_ori) or the result would exceed gp_len
 * (mutation.cu:256-266,279-289).  Node indices outside the live tree (undefined behaviour in the
 * reference) also produce a copy of the left tree. */
int evogp_hip_crossover(int pop_size_ori, int pop_size_new, int gp_len,
                        const float *value_ori, const int16_t *type_ori, const int16_t *size_ori,
                        const int *left_idx, const int *right_idx,
                        const int *left_node_idx, const int *right_node_idx,
                        float *value_res, int16_t *type_res, int16_t *size_res,
                        evogp_stream_t stream);

/* kernel.h:71-81 `evaluate`.  results[n][:] = tree_n(variables[n][:]);
 * variables: f32[pop][var_len], results: f32[pop][out_len]. */
int evogp_hip_evaluate(unsigned pop_size, unsigned gp_len, unsigned var_len, unsigned out_len,
                       const float *value, const int16_t *type, const int16_t *size,
                       const float *variables, float *results, evogp_stream_t stream);

/* kernel.h:83-97 `SR_fitness`.  fitnesses[t] = (1/D) * sum_d sum_o err(labels[d][o] - tree_t(X[d])_o),
 * err = square (use_mse != 0) or abs.  variables: f32[D][var_len], labels: f32[D][out_len].
 * kernel_type 0..4 is accepted for compatibility (forward.cu:827-856); every value runs the same
 * fused kernel. */
int evogp_hip_sr_fitness(unsigned pop_size, unsigned data_points, unsigned gp_len,
                         unsigned var_len, unsigned out_len, int use_mse,
                         const float *value, const int16_t *type, const int16_t *size,
                         const float *variables, const float *labels, float *fitnesses,
                         unsigned kernel_type, evogp_stream_t stream);

/* Gradient of the SR loss with respect to the constants (no counterpart in the reference).  loss: f32[pop_size], the quantity
 * evogp_hip_sr_fitness returns, from this call's own forward pass; grad: f32[pop_size][gp_len], grad[t][i] = d loss[t] / d value[t][i]
 * for every CONST node i of tree t, exactly 0.0f at every other node and on the tail [len, gp_len).  Forward semantics are those of
 * evogp_hip_sr_fitness in both output modes; the derivative of every function, its edge cases included, is DESIGN.md's
 * "Constant gradients" table.  A malformed tree gets a NaN loss and a zero row.  Sums run in a fixed order (bit-identical results
 * from run to run).  out_len <= 16 (else EVOGP_E_UNSUPPORTED).  Rows of more than 64 nodes keep their tapes in an engine-owned
 * buffer per stream (2 x gp_len x 256 B per resident wave, 256 MiB at gp_len 1024 on a 256-CU device), allocated by the first such
 * call on the stream outside a stream capture (inside one: EVOGP_E_UNSUPPORTED) and freed by evogp_hip_release_workspaces. */
int evogp_hip_sr_gradient(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                          int use_mse, const float *value, const int16_t *type, const int16_t *size,
                          const float *variables, const float *labels, float *loss, float *grad, evogp_stream_t stream);

/* One iteration of the per-tree constant descent ("bold driver") on the device, with no host synchronisation.  Per tree t:
 * value / loss / grad hold the current constants, their loss and their gradient (evogp_hip_sr_gradient), step the step length h_t.
 *   phase & 1  accept: if loss_cand[t] < loss[t] (a NaN never accepts) the CONST words of value_cand's live prefix are copied to
 *              value, loss[t] = loss_cand[t], the grad row = the grad_cand row and h_t doubles; otherwise h_t halves.
 *   phase & 2  propose (after the accept): value_cand row = value row with every CONST node c_i -> c_i - h_t * g_i / |g|_2, or the
 *              value row unchanged when loss[t] or |g|_2 is not finite or is 0.
 * Neither type nor size nor any non-constant word of value is written.  A descent of S steps: evogp_hip_sr_gradient on value,
 * phase 2, then S times {evogp_hip_sr_gradient on value_cand -> loss_cand / grad_cand, phase 3 (the last one: phase 1)}.
 * loss_cand / grad_cand may be NULL when phase is 2. */
int evogp_hip_sr_const_step(unsigned pop_size, unsigned gp_len, unsigned out_len, int phase, float *value, const int16_t *type,
                            const int16_t *size, float *value_cand, float *loss, float *grad, const float *loss_cand,
                            const float *grad_cand, float *step, evogp_stream_t stream);

/* Gauss-Newton normal equations of the MSE loss in the constants of every single-output tree (no counterpart in the reference;
 * DESIGN.md section 3.11).  Inputs as evogp_hip_sr_gradient with out_len == 1 (any other out_len: EVOGP_E_BADARG).  The OPTIMISED
 * CONSTANTS of a tree are its first min(nc, K) CONST nodes in prefix order within the live prefix, K = EVOGP_LM_MAX_CONSTS = 8; any
 * further constant is held fixed.  With J_j[d] = d pred[d] / d c_j (one reverse walk seeded with 1, the adjoint rules of the
 * "Constant gradients" table) and r[d] = pred[d] - y[d]:
 *   loss[t]    = (1 / D) * sum_d r[d]^2, summed in the order of evogp_hip_sr_gradient's loss;
 *   normal[t]  = f32[44]: the 36 entries A_ij = (1 / D) * sum_d J_i[d] * J_j[d], i <= j < K, row-major (A_00 .. A_07, A_11 .. A_17,
 *                ..., A_77), then the 8 entries b_i = (1 / D) * sum_d J_i[d] * r[d] (half the gradient of the loss).  Every entry
 *                that involves an absent constant (index >= nc) is exactly 0.0f.
 * A malformed tree gets a NaN loss and a zero row.  Sums run in a fixed order (bit-identical results from run to run).  Rows of more
 * than 64 nodes use the per-stream tape buffer of evogp_hip_sr_gradient, under the same rules. */
int evogp_hip_sr_normal_eq(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                           const float *value, const int16_t *type, const int16_t *size, const float *variables,
                           const float *labels, float *loss, float *normal, evogp_stream_t stream);

/* One iteration of the per-tree Levenberg-Marquardt optimisation of the constants on the device, with no host synchronisation
 * (out_len != 1: EVOGP_E_BADARG).  Per tree t: value / loss / normal hold the current constants, their loss and their normal
 * equations (evogp_hip_sr_normal_eq), damping the factor lambda_t (f32[pop_size]).  phase as in evogp_hip_sr_const_step:
 *   phase & 1  accept: if loss_cand[t] < loss[t] (a NaN never accepts) the optimised constants of value_cand are copied to value,
 *              loss[t] = loss_cand[t], the normal row = the normal_cand row and lambda_t = max(lambda_t / 10, 1e-10); otherwise
 *              lambda_t = min(10 * lambda_t, 1e10).
 *   phase & 2  propose (after the accept): value_cand row = value row with the optimised constants c -> c + delta, where delta solves
 *              (A + lambda_t * diag(A)) delta = -b over the constants with A_ii != 0 (Cholesky in float64; a constant with
 *              A_ii == 0 has no influence and keeps its value).  The row is copied unchanged when loss[t] is not finite or is 0, an
 *              entry of A or b among those constants is not finite, a pivot is <= 0, or some c + delta is not finite in float32.
 * Neither type nor size nor any other word of value is written; every word of the value_cand row is.  An optimisation of S steps:
 * evogp_hip_sr_normal_eq on value, phase 2, then S times {evogp_hip_sr_normal_eq on value_cand -> loss_cand / normal_cand, phase 3
 * (the last one: phase 1)}.  loss_cand / normal_cand may be NULL when phase is 2. */
int evogp_hip_sr_lm_step(unsigned pop_size, unsigned gp_len, unsigned out_len, int phase, float *value, const int16_t *type,
                         const int16_t *size, float *value_cand, float *loss, float *normal, const float *loss_cand,
                         const float *normal_cand, float *damping, evogp_stream_t stream);

/* The loss of every SUBTREE of every single-output tree as a model of its own, and whether the subtree is constant over the dataset
 * (no counterpart in the reference).  Inputs as evogp_hip_sr_gradient with out_len == 1 (any other out_len:
 * EVOGP_E_BADARG).  Both outputs f32[pop_size][gp_len]:
 *   node_err[t][i]    (1 / D) * sum_d err(y[d] - v_i(X[d])) for i < len, v_i the value of the subtree rooted at node i: what
 *                     evogp_hip_sr_fitness returns for that subtree as a row of its own (NaN and inf propagate as there);
 *                     node_err[t][0] is the loss evogp_hip_sr_gradient returns, bit for bit;
 *   node_const[t][i]  c when v_i(X[d]) has the bit pattern of c on every row d and c is not a NaN (so -0.0 and 0.0 differ, and a
 *                     CONST leaf reports its value, a VAR leaf only that of a constant column); NaN otherwise.
 * Tail entries [len, gp_len) and every entry of a malformed tree (the trees evogp_hip_sr_gradient gives a NaN loss) are NaN.  Sums run
 * in a fixed order (bit-identical results from run to run).  Rows of more than 64 nodes use the per-stream tape buffer of
 * evogp_hip_sr_gradient, under the same rules. */
int evogp_hip_sr_subtree_errors(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                int use_mse, const float *value, const int16_t *type, const int16_t *size,
                                const float *variables, const float *labels, float *node_err, float *node_const,
                                evogp_stream_t stream);

/* Rewrite every single-output tree into a tree that is no larger and, on the data node_err / node_const were computed from, no worse
 * (out_len != 1: EVOGP_E_BADARG).  The rule reads only its inputs, in integer and fp32 comparisons (tests/subtree_ref.py restates it):
 *   s(i)    = size[t][i] kept inside [1, len - i];  a node "folds" when `fold` is set, its type is neither VAR nor CONST and
 *             node_const[t][i] is finite;
 *   hoist   r = the node of [0, len) whose node_err is finite and least, then of least s, then of least index; 0 when `hoist` is
 *             not set or no node has a finite error;
 *   fold    inside [r, r + s(r)) every node strictly inside the span of a folding node is dropped (the outermost folding node wins) and
 *             every folding node that is left becomes one CONST node of value node_const[t][i] and size 1;
 *   output  the nodes that are left, in order from position 0; the size of a kept node = the number of nodes left in its old span;
 *           [new_len, gp_len) is zero in all three arrays; root_pos[t] = r; loss[t] = node_err[t][r].
 * A malformed tree's row is copied as it is, with root_pos 0 and a NaN loss.  The outputs must not alias the inputs. */
int evogp_hip_prune_rows(unsigned pop_size, unsigned gp_len, unsigned out_len, int hoist, int fold, const float *value,
                         const int16_t *type, const int16_t *size, const float *node_err, const float *node_const,
                         float *out_value, int16_t *out_type, int16_t *out_size, int *root_pos, float *loss, evogp_stream_t stream);

/* evogp_hip_generate restricted to the trees n with (unsigned)active_word[n] < active_below (active_word == NULL: all of
 * them).  Rows of the other trees are not touched.  Used by the fused generation step: donors are only produced for
 * the offspring that will mutate. */
int evogp_hip_generate_masked(unsigned pop_size, unsigned gp_len, unsigned var_len, unsigned out_len,
                              unsigned const_samples_len, float out_prob, float const_prob,
                              const unsigned *keys, const float *depth2leaf_probs,
                              const float *roulette_funcs, const float *const_samples,
                              float *value_res, int16_t *type_res, int16_t *size_res,
                              unsigned tree_index_offset, const int *active_word, unsigned active_below,
                              evogp_stream_t stream);

/* The default generation step in one pass (replaces the PyTorch composition of
 * src/evogp/algorithm/genetic_programming.py:105-124 with selection/default.py, crossover/default.py and
 * mutation/default.py):
 *     res[0 .. n_elite)      = forest[order[0 .. n_elite)]
 *     child_i                = crossover(forest[order[r0 % n_surv]] at r2 % size, forest[order[r1 % n_surv]] at r3 % size)
 *     res[n_elite + i]       = r4 < mutate_below ? mutate(child_i, (r5 % 1024) % size(child_i), donor_i) : child_i
 * order: i32[n_surv] (descending fitness order), rnd: i32[6][pop_size - n_elite] raw words in [0, 2^31 - 1),
 * donors: [pop_size - n_elite][gp_len] (only the rows with r4 < mutate_below are read), decisions: optional
 * i32[pop_size - n_elite][6] = {left, right, p, q, mutated, mutate position} for tests, or NULL.
 * Fallback rules of the subtree replacement: mutation.cu:150-160,170-180,256-266,279-289. */
int evogp_hip_breed_default(int pop_size, int gp_len, int n_elite, int n_surv,
                            const float *value, const int16_t *type, const int16_t *size,
                            const int *order, const int *rnd, unsigned mutate_below,
                            const float *donor_value, const int16_t *donor_type, const int16_t *donor_size,
                            float *value_res, int16_t *type_res, int16_t *size_res,
                            int *decisions, evogp_stream_t stream);

/* evogp_hip_breed_default restricted to the rows [row_begin, row_begin + row_count) of the next generation (a rank's
 * slice of a sharded population).  value_res/type_res/size_res, the donor arrays and `decisions` hold
 * exactly row_count rows: row k of each belongs to next-generation row row_begin + k (donor rows of elite rows and of
 * offspring that do not mutate are never read). */
int evogp_hip_breed_default_rows(int pop_size, int gp_len, int n_elite, int n_surv,
                                 const float *value, const int16_t *type, const int16_t *size,
                                 const int *order, const int *rnd, unsigned mutate_below,
                                 const float *donor_value, const int16_t *donor_type, const int16_t *donor_size,
                                 float *value_res, int16_t *type_res, int16_t *size_res,
                                 int *decisions, int row_begin, int row_count, evogp_stream_t stream);

/* The same pass when value / type / size hold only the trees that `order` can name — `table_rows` rows, e.g. the
 * survivor table a sharded run gathers (evogp_amd/parallel.py) — instead of the whole population of `pop_size` trees;
 * `order` then holds table rows.  evogp_hip_breed_default_rows is this call with table_rows = pop_size. */
int evogp_hip_breed_default_table(int pop_size, int table_rows, int gp_len, int n_elite, int n_surv, const float *value,
                                  const int16_t *type, const int16_t *size, const int *order, const int *rnd,
                                  unsigned mutate_below, const float *donor_value, const int16_t *donor_type,
                                  const int16_t *donor_size, float *value_res, int16_t *type_res, int16_t *size_res,
                                  int *decisions, int row_begin, int row_count, evogp_stream_t stream);

/* The same pass for ANY selection operator (src/evogp/algorithm/genetic_programming.py:110-122 with e.g.
 * selection/tournament.py:59-133): the elites and the parents are two separate lists of table rows,
 *     res[0 .. n_elite)  = table[elite_rows[0 .. n_elite)]
 *     child_i            = crossover(table[parent_rows[r0 % n_surv]] at r2 % size, table[parent_rows[r1 % n_surv]] at r3 % size)
 * parent_rows: i32[n_surv], repeats allowed (a tournament winner that won k times is k entries, exactly the
 * `forest[survivor_indices]` gather of crossover/default.py:37; n_surv is not bounded by pop_size); elite_rows: i32[n_elite]
 * (may be NULL when n_elite == 0).  evogp_hip_breed_default_table is this call with both lists = order. */
int evogp_hip_breed_lists(int pop_size, int table_rows, int gp_len, int n_elite, int n_surv, const float *value,
                          const int16_t *type, const int16_t *size, const int *elite_rows, const int *parent_rows,
                          const int *rnd, unsigned mutate_below, const float *donor_value, const int16_t *donor_type,
                          const int16_t *donor_size, float *value_res, int16_t *type_res, int16_t *size_res,
                          int *decisions, int row_begin, int row_count, evogp_stream_t stream);

/* evogp_hip_sr_fitness for a caller that knows which functions can occur in the forest: bit f of function_mask = function id f
 * (defs.h:10-57) may occur, 0 = unknown.  A fitness call is up to five launches of which three usually find nothing to do; a
 * forest of + - * / and the unary functions of at most 64 nodes per tree cannot leave a tree for the general compiler, so that
 * launch need not be made (5 -> 4 launches: 5-11 us per call).  Whatever a tree carries that the mask did not promise is still
 * evaluated correctly by the last follow-up kernel: a wrong mask costs speed, never a result.  (tree_generate emits the
 * invalid function id 29 when its uniform draw is exactly 1.0 -- generate.cu:77-84, one tree in the 1 M-tree headline forest; the
 * compiler takes such nodes itself, so they do not break the promise.)  EVOGP_TC_FUNC_MASK=0 makes the engine ignore the mask.  evogp_amd.tree.Forest derives the mask from the GenerateDescriptors its trees came from. */
int evogp_hip_sr_fitness_hinted(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                int use_mse, const float *value, const int16_t *type, const int16_t *size,
                                const float *variables, const float *labels, float *fitnesses, unsigned kernel_type,
                                unsigned function_mask, evogp_stream_t stream);
/* (Rounds 3-4 also shipped two opt-in experiments -- program records compiled ahead by the breeding pass under a stamp protocol
 * (evogp_hip_breed_lists_compiled, evogp_hip_sr_fitness_stamped, evogp_hip_set_breed_compile) and history-driven launch skipping
 * (EVOGP_TC_HINTS) -- that gained nothing measurable and, switched on globally, failed tests.  Round 5 removed both: ABI version 4.) */

/* The same two passes with their random words computed in the kernels (no counterpart in the reference): word k of offspring i is
 * hash(seed, generation, k, i) -- exactly the numbers evogp_hip_random_words writes -- so no array of words is drawn, written and read
 * (one launch and 24 B per offspring less per generation), and the two generation keys are words (7, 0) and (7, 1) modulo 10^6.
 * evogp_hip_generate_masked_hashed generates the trees n whose word (4, n + tree_index_offset) is below active_below;
 * evogp_hip_breed_lists_hashed is evogp_hip_breed_lists without `rnd`.  Results equal those of the array forms fed with
 * evogp_hip_random_words(seed, generation, ...) bit for bit (tests/test_gpu_breed.py). */
int evogp_hip_generate_masked_hashed(unsigned pop_size, unsigned gp_len, unsigned var_len, unsigned out_len,
                                     unsigned const_samples_len, float out_prob, float const_prob, const float *depth2leaf_probs,
                                     const float *roulette_funcs, const float *const_samples, float *value_res, int16_t *type_res,
                                     int16_t *size_res, unsigned tree_index_offset, long long seed, long long generation,
                                     unsigned active_below, evogp_stream_t stream);
int evogp_hip_breed_lists_hashed(int pop_size, int table_rows, int gp_len, int n_elite, int n_surv, const float *value,
                                 const int16_t *type, const int16_t *size, const int *elite_rows, const int *parent_rows,
                                 long long seed, long long generation, unsigned mutate_below, const float *donor_value,
                                 const int16_t *donor_type, const int16_t *donor_size, float *value_res, int16_t *type_res,
                                 int16_t *size_res, int *decisions, int row_begin, int row_count, evogp_stream_t stream);

/* The reference's structural and point mutations, drawn and applied in one launch each (no counterpart in the
 * reference's ABI, whose operators are torch programs around tree_crossover: src/evogp/algorithm/mutation/hoist.py:43-75,
 * delete.py:44-105, single_point.py:43-126, multi_point.py:46-143, single_const.py:39-98, multi_const.py:43-95).  The random numbers are the
 * counter-based words of evogp_hip_random_words under (seed, call): word 0 of tree n decides whether it mutates (u < rate), words 1 and 2
 * the nodes; words 8-12 of node n * gp_len + i its new payload.  Trees below skip_rows (the elites of a generation step) are copied.
 *   evogp_hip_structural_mutate  mode 0 = DeleteMutation (a function node whose subtree has at most max_size nodes -- 0: any -- is replaced by
 *       its child number trunc(1 + u (arity - 1)), the reference's draw), 1 = HoistMutation (node trunc(u S) is replaced by node
 *       trunc(u' size) taken as an absolute index, or as an offset into the subtree with inner_is_offset); the fall-back rules of
 *       tree_crossover apply (mutation.cu:256-266, 279-289).  decisions: optional i32[pop][2] = {replaced node or -1, donor node}.
 *   evogp_hip_point_mutate       mode 0 = MultiPointMutation, 1 = SinglePointMutation, 2 = MultiConstMutation, 3 = SingleConstMutation;
 *       only the value array changes.  roulette_*funcs: the descriptor's cumulative per-arity tables, f32[29] each. */
int evogp_hip_structural_mutate(int pop_size, int gp_len, int mode, float rate, int max_size, int inner_is_offset, int skip_rows,
                                long long seed, long long call, const float *value, const int16_t *type, const int16_t *size,
                                float *value_res, int16_t *type_res, int16_t *size_res, int *decisions, evogp_stream_t stream);
/* InsertMutation (mutation/insert.py:45-85): tree n mutates when counter word (4, n) of (seed, call) lies below mutate_below (of 2^31) -- the
 * rule under which evogp_hip_generate_masked_hashed(seed, call, mutate_below) generated the fresh trees handed in as donor_* (row n for tree n).
 * decisions (optional, [pop][2]): node of the tree that was replaced (-1: the tree was copied), position inside the fresh tree. */
int evogp_hip_insert_mutate(int pop_size, int gp_len, unsigned mutate_below, int skip_rows, long long seed, long long call,
                            const float *value, const int16_t *type, const int16_t *size, const float *donor_value,
                            const int16_t *donor_type, const int16_t *donor_size, float *value_res, int16_t *type_res, int16_t *size_res,
                            int *decisions, evogp_stream_t stream);
int evogp_hip_point_mutate(int pop_size, int gp_len, int mode, float rate, float intensity, int per_node, int modify_output,
                           int fix_roulette, int skip_rows, int input_len, int output_len, int n_consts, long long seed, long long call,
                           const float *value, const int16_t *type, const int16_t *size, const float *roulette_ufuncs,
                           const float *roulette_bfuncs, const float *roulette_tfuncs, const float *const_samples, float *value_res,
                           evogp_stream_t stream);

/* Counter-based random words for the breeding pass of a sharded run (no counterpart in the reference, which draws with
 * torch's generator): out[k][i] for k < rows, i in [lo, hi) = hash(seed, generation, k, i) mapped to [0, 2^31 - 1), the value
 * evogp_amd/parallel.py random_words computes on any device; out: i32[rows][n_cols], only columns [lo, hi) are written.  Every
 * rank fills the columns of its own offspring; equal arguments give equal words on every rank and for every world size. */
int evogp_hip_random_words(long long seed, long long generation, int rows, long long n_cols, long long lo, long long hi,
                           int *out, evogp_stream_t stream);

/* scores[i] = -inf where errors[i] is NaN, else -errors[i] (negate != 0) or errors[i] (no counterpart in the reference's ABI: its
 * SymbolicRegression.evaluate negates in torch, problem/symbolic_regression.py:82-96, and its pipeline scrubs NaN with a boolean-mask
 * assignment, pipeline/standard.py:41-43 -- four small launches and a host sync per generation).  errors and scores may be the same array. */
int evogp_hip_fitness_scores(unsigned n, int negate, const float *errors, float *scores, evogp_stream_t stream);

/* Selection in one launch (no counterpart in the reference, whose DefaultSelection sorts the whole fitness vector,
 * src/evogp/algorithm/selection/default.py:21-39): order[0 .. n_elite) = the n_elite trees of highest fitness, order[n_elite ..
 * n_keep) = the next n_keep - n_elite, each group in ascending tree index.  Ties at a threshold go to the lower index, so both
 * SETS are those of a stable descending sort; NaN is the worst fitness.  n_elite <= n_keep <= n.  `zeroed_workspace`:
 * evogp_hip_select_workspace_bytes() bytes, all zero (the kernel's grid barrier and histograms live there). */
size_t evogp_hip_select_workspace_bytes(void);
int evogp_hip_select(unsigned n, unsigned n_elite, unsigned n_keep, const float *fitness, int *order, void *zeroed_workspace,
                     evogp_stream_t stream);
/* The same launch for a caller that alternates between two workspaces on one stream: `next_workspace` (the other one, used by the
 * previous call on that stream) is zeroed by this launch, so the steady state needs no memset per call (3-4 us). */
int evogp_hip_select_alternating(unsigned n, unsigned n_elite, unsigned n_keep, const float *fitness, int *order,
                                 void *zeroed_workspace, void *next_workspace, evogp_stream_t stream);

/* Tournament selection in one launch (no counterpart in the reference's ABI; src/evogp/algorithm/selection/tournament.py:59-133 with its
 * default arguments, which is also the setting of example/uci_sr.py:73-75: contenders drawn WITH replacement, the best contender
 * wins): winners[i] = the tree of highest fitness among t_size contenders, contender k of tournament i being tree
 * hash(seed, generation, 16 + k, i) % n -- the counter-based words of evogp_hip_random_words, so every rank of a sharded run names
 * the same contenders (evogp_amd/parallel.py random_words gives the same numbers on any device).  NaN is the worst fitness; of
 * equal contenders the first drawn wins (torch.argmax).  winners: i32[n_tournaments]. */
int evogp_hip_tournament_select(unsigned n, unsigned n_tournaments, unsigned t_size, long long seed, long long generation,
                                const float *fitness, int *winners, evogp_stream_t stream);

/* Per-case errors of symbolic regression (no counterpart in the reference), CASE-MAJOR:
 *     errors[d][t] = (sum_o delta_o) / out_len   in float32, o ascending,   delta_o = (tree_t(X[d])_o - y[d][o])^2 (use_mse) or |...|
 * with the predictions of evogp_hip_batch_evaluate (the same interpreters): the errors are bit-identical to this formula applied to
 * Forest.batch_forward's outputs, and NaN stays NaN.  variables: f32[D][var_len], labels: f32[D][out_len], errors: f32[D][pop_size].
 * Argument contract and limits of evogp_hip_batch_evaluate.  The (pop_size, D, out_len) predictions go to an engine-owned buffer per
 * stream (pop_size x D x out_len x 4 bytes), allocated by the first call of that size on the stream outside a stream capture (inside
 * one: EVOGP_E_UNSUPPORTED) and freed by evogp_hip_release_workspaces. */
int evogp_hip_sr_case_errors(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                             int use_mse, const float *value, const int16_t *type, const int16_t *size,
                             const float *variables, const float *labels, float *errors, evogp_stream_t stream);

/* Semi-dynamic epsilon-lexicase parent selection (no counterpart in the reference; La Cava, Helmuth, Spector & Moore 2019) over
 * case-major errors E f32[n_cases][pop]:
 *     key(x) = +inf if x is NaN, +0 if x is -0, else x;  eps[c]: NaN or negative counts as 0
 *     trees i and j are CLONES when key(E[c][i]) == key(E[c][j]) bitwise for every case c
 *     event k:  pool = all trees;  for j = 0, 1, ..., n_cases - 1 while the pool holds more than one clone class:
 *                   c = perm_k(j);  m = min over the pool of key(E[c][i]);
 *                   pool = {i in pool : key(E[c][i]) <= m + eps[c] (float32 add) or key(E[c][i]) == m}
 *               L = the pool class by class (classes in ascending order of their smallest tree, each in ascending tree order)
 *               winners[k] = L[word_k % len(L)]
 * ("or == m" only matters when m + eps[c] is NaN, m = -inf and eps = +inf: the minimum always stays.)  perm_k is a 4-round Feistel
 * network on the smallest even bit width w with 2^w >= n_cases, cycle-walked into [0, n_cases), evaluated position by position; its
 * round key r is counter word (2^21 + r, k) of (seed, generation) and word_k is counter word (2^21 + 4, k) (the words of
 * evogp_hip_random_words; the tournament uses rows 16 + k, k < 2^20).  Clones are found by a 64-bit hash of the key rows: a collision
 * (probability about pop^2 / 2^65) merges two classes.  The result is deterministic; nothing synchronises with the host.
 * n_events may be 0 (nothing is launched).  workspace: evogp_hip_lexicase_workspace_bytes bytes of device memory owned by the caller
 * (no zeroing needed), at most about 2 x 4 n_cases pop + 60 pop bytes plus the radix sort's scratch; the engine allocates nothing.
 * evogp_hip_lexicase_workspace_bytes queries the sort's scratch size on the current device. */
int evogp_hip_lexicase_workspace_bytes(unsigned n_cases, unsigned pop, unsigned n_events, unsigned long long *bytes);
int evogp_hip_lexicase_select(unsigned n_cases, unsigned pop, const float *errors, const float *eps, unsigned n_events,
                              long long seed, long long generation, int *winners, void *workspace, evogp_stream_t stream);

/* Pareto ranking of a population on two objectives, both "lower is better" (no counterpart in the reference; Deb, Pratap, Agarwal &
 * Meyarivan 2002): err f32[pop] and an integer complexity cx i32[pop] meant to lie in [0, cx_bound].  cx_bound <= 65535 is a HOST-side
 * bound (max_tree_len for tree size); the kernels size their bucket table by it.
 *     key(e) = +inf if e is NaN, +0 if e is -0, else e.  A tree is RANKED iff its key is finite and 0 <= cx <= cx_bound; a tree
 *         outside the bound cannot be reported without a host sync, so it is unranked like a NaN tree
 *     ranked q DOMINATES ranked p iff key_q <= key_p and cx_q <= cx_p and at least one is strict
 *     front[p] = 0 if no ranked tree dominates p, else 1 + the largest front among the trees that dominate p; unranked: 0x7FFFFFFF
 *     trees with bitwise equal (key, cx) are one POINT, its representative the lowest tree index
 *     crowding[p], over the distinct points of p's front sorted by cx ascending (their keys then descend strictly): +inf for the
 *         first and the last point; point j in between:
 *             (cx[j+1] - cx[j-1]) / (cx_last - cx_first) + (key[j-1] - key[j+1]) / (key_first - key_last)
 *         every operand float32, every operation one IEEE float32 operation in the order written, a NaN result counts as +inf.
 *         Only the representative carries the distance: its clones and the unranked trees get 0
 *     order i32[pop]: all trees by front ascending, then crowding descending, then tree index ascending (the crowded-comparison
 *         operator as a total order); the unranked trees come last, in index order
 * The result is deterministic and bit-identical from run to run (integer atomic maxima only); nothing synchronises with the host and
 * the number of launches is fixed.  workspace: evogp_hip_pareto_rank_workspace_bytes(pop) bytes of device memory owned by the caller
 * (no zeroing needed), about 84 pop bytes plus the radix sort's scratch; the engine allocates nothing. */
int evogp_hip_pareto_rank_workspace_bytes(unsigned pop, unsigned long long *bytes);
int evogp_hip_pareto_rank(unsigned pop, unsigned cx_bound, const float *err, const int *cx, int *front, float *crowding, int *order,
                          void *workspace, evogp_stream_t stream);

/* NSGA-II's binary (t_size-ary) tournament on an order of evogp_hip_pareto_rank: tournament i draws t_size contenders with replacement
 * from the first `pool` trees of the order and the best by crowded comparison wins,
 *     winners[i] = order[min over k < t_size of (word(seed, generation, 2^22 + k, i) mod pool)]
 * with the counter words of evogp_hip_random_words (rows 2^22 + k collide with neither the tournaments' 16 + k nor lexicase's
 * 2^21 + 0..5).  1 <= pool <= pop, 1 <= t_size <= 2^20; n_tournaments may be 0 (nothing is launched).  winners: i32[n_tournaments]. */
int evogp_hip_nsga2_select(unsigned pop, const int *order, unsigned pool, unsigned n_tournaments, unsigned t_size, long long seed,
                           long long generation, int *winners, evogp_stream_t stream);

/* Structural duplicates of a forest (no counterpart in the reference).  n = size[t][0]; a row with n < 1 or n > gp_len is OUT OF RANGE: a
 * class of its own, hash 0.  Two in-range rows are EQUAL when their n are equal and, for every i < n, the fp32 bit pattern of value[i],
 * the 16 bits of type[i] and size[i] are equal (-0.0 != 0.0, NaNs compare by bits, the OUT flag counts; words at i >= n are never read).
 *     hash(t) = mix64((sum_{i<n} mix64(w_i ^ ((i + 1) * 0x9E3779B97F4A7C15))) + n),  w_i = (uint64)(uint16)type[i] << 32 | bits(value[i])
 * mod 2^64, mix64 the splitmix64 finaliser of evogp_hip_random_words.  evogp_hip_tree_hash writes hash_out u64[pop].
 * evogp_hip_tree_classes writes class_id_out i32[pop]: class_id[t] = the SMALLEST tree index whose row equals row t (so class_id[t] <= t
 * and class_id[class_id[t]] == class_id[t]).  hash_in u64[pop] only decides which rows are compared -- equality alone decides a class --
 * and may be any array in which equal rows carry equal words (evogp_hip_tree_hash's, normally): the result does not depend on it.
 * Rows are compared inside a run of equal hash words, each with the rows before it in ascending tree order: without a collision the
 * first comparison decides, a run of r distinct colliding rows costs O(r^2) comparisons.  Deterministic, no atomics, nothing
 * synchronises with the host.  workspace: evogp_hip_tree_classes_workspace_bytes(pop) bytes of device memory owned by the caller (no
 * zeroing needed), about 32 pop bytes plus the radix sort's scratch; the engine allocates nothing. */
int evogp_hip_tree_hash(unsigned pop, unsigned gp_len, const float *value, const int16_t *type, const int16_t *size,
                        unsigned long long *hash_out, evogp_stream_t stream);
int evogp_hip_tree_classes_workspace_bytes(unsigned pop, unsigned long long *bytes);
int evogp_hip_tree_classes(unsigned pop, unsigned gp_len, const float *value, const int16_t *type, const int16_t *size,
                           const unsigned long long *hash_in, int *class_id_out, void *workspace, evogp_stream_t stream);

/* Semantic duplicates of a single-output forest on a dataset (no counterpart in the reference; csrc/sr_semantic.hip): different trees
 * that are the same model.  p[t][d] is the float32 prediction of tree t on row d of variables (data_points, var_len), the bits
 * evogp_hip_batch_evaluate stores.  Its KEY is that bit pattern with -0.0 -> +0.0 and every NaN -> 0x7FC00000 (+-inf and everything else
 * keep their bits).  A row is WELL FORMED when the structural pre-pass of the SR kernels accepts it (the rows for which
 * evogp_hip_sr_linear_scaling evaluates anything: length clamped to [0, gp_len], not empty, no stack underflow, one value left).
 * Two trees are EQUAL when both are well formed and their keys agree on every row; a malformed row is a class of its own.
 *     sig(t) = mix64((sum_{d<D} mix64((uint64)key[t][d] ^ ((d + 1) * 0x9E3779B97F4A7C15))) + D)  mod 2^64,   sig = 0 for a malformed row
 * with the mix64 of evogp_hip_tree_hash.  The sum is position-keyed and modular: no order of lanes, tiles or waves changes it.
 * evogp_hip_sr_semantic_hash writes sig_out u64[pop]: the kernels of evogp_hip_sr_linear_scaling (register interpreter, LEAN then FULL
 * build, then the scratch-stack kernel for deep trees and for var_len > 32) with an integer epilogue; the (pop, D) predictions are never
 * stored.  workspace: evogp_hip_sr_semantic_hash_workspace_bytes(pop) bytes (a mark byte per tree; no zeroing needed).
 * evogp_hip_sr_semantic_classes writes class_id_out i32[pop]: class_id[t] = the SMALLEST index of a tree equal to tree t (class_id[t] <= t,
 * class_id[class_id[t]] == class_id[t]).  hash_in u64[pop] only decides which trees are compared -- equality alone decides a class -- and
 * may be any array in which equal trees carry equal words (evogp_hip_sr_semantic_hash's, normally): the result does not depend on it.
 * Trees are compared inside a run of equal hash words, each with the trees before it in ascending index order, and the first equal one
 * wins.  A comparison first compares the live prefixes word for word (equal programs are equal models: no evaluation), and otherwise
 * evaluates both trees 64 rows at a time and stops at the first chunk with a differing key.  Without a collision every member of a class
 * pays one comparison; a run of r distinct colliding trees costs O(r^2) comparisons of up to 2 D tree evaluations each.  workspace:
 * evogp_hip_sr_semantic_classes_workspace_bytes(pop) bytes (what evogp_hip_tree_classes takes).
 * Both: deterministic and bit-identical from run to run, no float atomics, everything on the caller's stream, nothing synchronises with
 * the host, the engine allocates nothing.  Any gp_len <= 1024, var_len and data_points; out_len != 1 returns EVOGP_E_UNSUPPORTED. */
int evogp_hip_sr_semantic_hash_workspace_bytes(unsigned pop_size, unsigned long long *bytes);
int evogp_hip_sr_semantic_hash(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                               const float *value, const int16_t *type, const int16_t *size, const float *variables,
                               unsigned long long *sig_out, void *workspace, evogp_stream_t stream);
int evogp_hip_sr_semantic_classes_workspace_bytes(unsigned pop_size, unsigned long long *bytes);
int evogp_hip_sr_semantic_classes(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                  const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                  const unsigned long long *hash_in, int *class_id_out, void *workspace, evogp_stream_t stream);

/* Interval arithmetic over single-output trees (Keijzer 2003; no counterpart in the reference; csrc/sr_interval.hip).  For every node i
 * of the live prefix (n = size[t][0] clamped to [0, gp_len]) of every tree: lo[t][i], hi[t][i] (float32 in [-inf, +inf]) and flags[t][i]
 * (bit 0 EVOGP_ITV_MAY_NAN, bit 1 EVOGP_ITV_MALFORMED) such that for ANY float32 input x with lower[v] <= x[v] <= upper[v] the float32
 * value V the interpreters compute for the subtree rooted at i is either a NaN with MAY_NAN set or satisfies lo <= V <= hi.  The
 * bounds are on the values as computed in fp32: + - * neg abs max min sqrt take their endpoints from the same correctly rounded
 * operations on the operands' endpoints (exact: rounding is monotone), the divisions move the quotients of the endpoints one ulp
 * outward, the library functions move their own results at the relevant endpoints outward by 2 E + 1 ulps (E the documented bound:
 * sin cos 4, tan 5, sinh cosh tanh 5, log exp 3, pow 16); the extrema of sin / cos and the poles of tan are placed in float64.  The
 * complete rule set is the numpy restatement tests/interval_ref.py, which the kernel follows operation by operation.
 * A row whose type words fail the stack discipline, or one of whose live size words is not the size of its subtree, has lo = hi = NaN
 * and flags = 3 on every live word (on word 0 when it has none).  Words past the live prefix are 0, 0, 0.
 * lower / upper: float32[var_len] on the device, finite, lower <= upper (the caller checks).  One lane per tree, no dataset, no
 * workspace, no atomics, nothing synchronises with the host; bit-identical from run to run.  Any gp_len <= 1024 and var_len >= 1.
 * lo, hi, flags must not alias the inputs. */
#define EVOGP_ITV_MAY_NAN 1
#define EVOGP_ITV_MALFORMED 2
int evogp_hip_tree_intervals(unsigned pop, unsigned gp_len, unsigned var_len, const float *value, const int16_t *type,
                             const int16_t *size, const float *lower, const float *upper, float *lo, float *hi, unsigned char *flags,
                             evogp_stream_t stream);

/* Interval bounds on the partial derivatives of single-output trees (shape constraints, Kronberger et al. 2022; no counterpart in the
 * reference; csrc/sr_deriv.hip).  Two quantities for every node i of the live prefix of every tree, over the box lower[v] <= x[v] <= upper[v].
 * R(i) = [vlo[t][i], vhi[t][i]] with vflags[t][i] (EVOGP_ITV_*): an enclosure of the REAL value of the subtree rooted at i: the rules of
 * evogp_hip_tree_intervals with the round-to-nearest endpoints of + - * sqrt loose_sqrt moved one ulp outward (not where the operation
 * is exact: an endpoint sum with a zero term, a point-zero or point-one operand of *, a zero endpoint of * that is no underflow, the
 * square root of 0); it contains the interval evogp_hip_tree_intervals
 * gives, so it bounds the fp32 value too.
 * D_v(i) = [dlo[k][t][i], dhi[k][t][i]] with dflags[k][t][i] for v = wrt[k]:  (a) at every real x of the box at which every node of the
 * subtree has a defined finite real value and the subtree is differentiable in x_v, d subtree_i / d x_v lies in [dlo, dhi];  (b) if
 * EVOGP_DRV_JUMP is clear and vflags[t][i] is 0, the subtree is continuous in x_v on the box, so dlo >= 0 means nondecreasing in x_v and
 * dhi <= 0 nonincreasing.  EVOGP_DRV_DEPENDS: x_v occurs in a branch that can be taken; a subtree without it has exactly [0, 0] and
 * flags 0.  The rules are forward-mode differentiation in outward-rounded interval arithmetic (the 0 x inf corner is 0, an unbounded
 * derivative is [-inf, +inf]); pow and loose_pow give [-inf, +inf] wherever they depend on x_v.  The complete rule set is the numpy
 * restatement tests/derivative_ref.py, which the kernels follow operation by operation.
 * A malformed row (evogp_hip_tree_intervals's rule) has vlo = vhi = NaN, vflags = 3 and dlo = dhi = NaN, dflags = EVOGP_DRV_MALFORMED on
 * every live word (on word 0 when it has none).  Words past the live prefix are 0 in all six outputs.
 * lower / upper: float32[var_len] on the device, finite, lower <= upper; wrt: int32[n_wrt] on the device, each in [0, var_len) (the caller
 * checks both); 1 <= n_wrt <= 65535; a repeated index gives equal slices.  vlo, vhi, vflags: [pop][gp_len]; dlo, dhi, dflags:
 * [n_wrt][pop][gp_len].  Two launches (one lane per tree, then one lane per (tree, k)), no dataset, no workspace, no atomics, nothing
 * synchronises with the host; bit-identical from run to run.  The outputs must not alias the inputs or one another. */
#define EVOGP_DRV_JUMP 1
#define EVOGP_DRV_MALFORMED 2
#define EVOGP_DRV_DEPENDS 4
int evogp_hip_tree_derivative_intervals(unsigned pop, unsigned gp_len, unsigned var_len, const float *value, const int16_t *type,
                                        const int16_t *size, const float *lower, const float *upper, unsigned n_wrt, const int *wrt,
                                        float *vlo, float *vhi, unsigned char *vflags, float *dlo, float *dhi, unsigned char *dflags,
                                        evogp_stream_t stream);

/* Dimensional analysis over single-output trees (physical units; no counterpart in the reference; csrc/sr_dims.hip).  A unit is n_dims
 * int32 numerators over the fixed denominator EVOGP_DIM_DEN (2^4 3^2 5^2 7: four nested square roots and two cube roots of integer powers
 * stay exact); a numerator is in range when |n| <= EVOGP_DIM_MAX_NUM; all zeros is "dimensionless".  Variables carry var_units[v], a CONST
 * node is FREE: it may carry whatever unit makes the tree consistent.  violations[t] == 0 iff the constants of tree t can be given units
 * such that every operation is dimensionally consistent and (check_root != 0) the root has label_units -- always sound; complete for every
 * tree without a pow / loose_pow over a free base, within the in-range units -- and units[t][i][:] then holds the unit of every node i of
 * one such assignment (that of a CONST node is the unit of the constant).  Otherwise violations[t] counts the violating nodes (plus one
 * for a root mismatch) and units holds pass 1's: the fixed units, 0 at free and violating nodes.  flags[t][i]: EVOGP_DIM_FREE (the node
 * was free in pass 1), EVOGP_DIM_VIOLATION, EVOGP_DIM_MALFORMED, EVOGP_DIM_ROOT_MISMATCH (node 0 only).  The complete rule set -- pass 1
 * bottom-up, pass 2 top-down -- is the integer restatement tests/dimension_ref.py, which the kernel reproduces word for word.
 * A malformed row (evogp_hip_tree_intervals's rule) has flags EVOGP_DIM_MALFORMED and unit 0 on every live word (on word 0 when it has
 * none) and violations = -1.  Words past the live prefix are 0 in units and flags.
 * var_units: int32[var_len][n_dims], label_units: int32[n_dims], on the device, every numerator in range (the caller checks); label_units
 * is read only when check_root != 0 but must not be null.  units: int32[pop][gp_len][n_dims], flags: uint8[pop][gp_len], violations:
 * int32[pop].  One lane per tree, both passes in one launch, no dataset, no workspace, no atomics, nothing synchronises with the host;
 * bit-identical from run to run.  Any gp_len <= 1024, var_len >= 1, 1 <= n_dims <= EVOGP_DIM_MAX_DIMS.  The outputs must not alias the
 * inputs or one another. */
#define EVOGP_DIM_DEN 25200
#define EVOGP_DIM_MAX_NUM 16777216
#define EVOGP_DIM_MAX_DIMS 8
#define EVOGP_DIM_FREE 1
#define EVOGP_DIM_VIOLATION 2
#define EVOGP_DIM_MALFORMED 4
#define EVOGP_DIM_ROOT_MISMATCH 8
int evogp_hip_tree_dimensions(unsigned pop, unsigned gp_len, unsigned var_len, unsigned n_dims, const float *value, const int16_t *type,
                              const int16_t *size, const int *var_units, const int *label_units, int check_root, int *units,
                              unsigned char *flags, int *violations, evogp_stream_t stream);

/* Structural constraints over single-output trees (depth, weighted complexity, operand limits, nesting limits; no counterpart in the
 * reference; csrc/sr_structure.hip).  Every live node has a symbol in [0, EVOGP_STRUCT_SYMBOLS): the function ids 0 .. 28 (a ternary-typed
 * node is IF, 0, whatever its id), EVOGP_STRUCT_SYM_VAR, EVOGP_STRUCT_SYM_CONST, and EVOGP_STRUCT_SYM_UNKNOWN for a unary or binary node
 * whose id is no function of its class.  Bottom-up: complexity[t][i] = cost[s_i] + the children's; height[t][i] = 1 + the largest child
 * height (a leaf: 1); for rule r, below = the largest nest[..][r] of the children and nest[t][i][r] = min(255, below + [s_i in
 * rule_inner[r]]); node i gets EVOGP_STRUCT_NEST when s_i is in rule_outer[r] and below > rule_limit[r] for some r, and
 * EVOGP_STRUCT_OPERAND when operand_limit[s_i][k] >= 0 and the complexity of operand k exceeds it (operand order as the interpreters').
 * Node 0 gets EVOGP_STRUCT_DEPTH when max_depth >= 0 and height[t][0] > max_depth, EVOGP_STRUCT_COMPLEXITY when max_complexity >= 0 and
 * complexity[t][0] > max_complexity.  Top-down: depth[t][0] = 0, a child's depth is its parent's + 1.  violations[t] = the nodes with
 * NEST or OPERAND (each once) + [DEPTH] + [COMPLEXITY].  The complete rule set is the integer restatement tests/structure_ref.py, which
 * the kernel reproduces word for word.  A malformed row (evogp_hip_tree_intervals's rule) has flags EVOGP_STRUCT_MALFORMED on every live
 * word (on word 0 when it has none), 0 in every other output and violations = -1.  Words past the live prefix are 0 in every output.
 * cost: int32[32], each in [0, 65535]; operand_limit: int32[32][3], -1 for none; rule_outer, rule_inner: int32[n_rules], sets of symbols
 * (bit s = symbol s); rule_limit: int32[n_rules], each in [0, 254] -- on the device, the caller checks the ranges; the three rule
 * pointers and nest may be null only when n_rules == 0, and nest must then be 8-byte aligned (EVOGP_E_BADARG otherwise: the counters of
 * a node are accessed as one word); n_rules <= EVOGP_STRUCT_MAX_RULES; max_depth, max_complexity: -1 for none.
 * complexity: int32[pop][gp_len], height, depth: int16[pop][gp_len], nest: uint8[pop][gp_len][n_rules], flags: uint8[pop][gp_len],
 * violations: int32[pop].  One lane per tree, both passes in one launch, no dataset, no workspace, no atomics, nothing synchronises
 * with the host; bit-identical from run to run.  Any gp_len <= 1024.  The outputs must not alias the inputs or one another. */
#define EVOGP_STRUCT_SYMBOLS 32
#define EVOGP_STRUCT_SYM_VAR 29
#define EVOGP_STRUCT_SYM_CONST 30
#define EVOGP_STRUCT_SYM_UNKNOWN 31
#define EVOGP_STRUCT_MAX_RULES 8
#define EVOGP_STRUCT_NEST 1
#define EVOGP_STRUCT_OPERAND 2
#define EVOGP_STRUCT_MALFORMED 4
#define EVOGP_STRUCT_DEPTH 8
#define EVOGP_STRUCT_COMPLEXITY 16
int evogp_hip_tree_structure(unsigned pop, unsigned gp_len, unsigned n_rules, const float *value, const int16_t *type, const int16_t *size,
                             const int *cost, const int *operand_limit, const int *rule_outer, const int *rule_inner,
                             const int *rule_limit, int max_depth, int max_complexity, int *complexity, int16_t *height, int16_t *depth,
                             unsigned char *nest, unsigned char *flags, int *violations, evogp_stream_t stream);

/* Non-replicating batch evaluation (replaces the repeat_interleave + tree_evaluate
 * composition of src/evogp/tree/forest.py:143-176): results[t][d][:] = tree_t(variables[d][:]),
 * variables: f32[D][var_len], results: f32[pop][D][out_len]. */
int evogp_hip_batch_evaluate(unsigned pop_size, unsigned data_points, unsigned gp_len,
                             unsigned var_len, unsigned out_len,
                             const float *value, const int16_t *type, const int16_t *size,
                             const float *variables, float *results, evogp_stream_t stream);

/* Fused epilogue of the Classification problem (src/evogp/problem/classification.py:62-75) on top of the batch
 * evaluation: counts[t] = number of rows d with argmax_o tree_t(variables[d])_o == labels[d], where the arg-max is the
 * one torch.argmax(clip(softmax(outputs))) returns (first maximum; index 0 when an output is NaN or the maximum is
 * infinite).  out_len in [2, 16]; labels: i32[data_points]; counts: u32[pop_size] (zeroed here).  The
 * (pop, data_points, out_len) output tensor is never materialised. */
int evogp_hip_batch_argmax_count(unsigned pop_size, unsigned data_points, unsigned gp_len,
                                 unsigned var_len, unsigned out_len,
                                 const float *value, const int16_t *type, const int16_t *size,
                                 const float *variables, const int *labels, unsigned *counts,
                                 evogp_stream_t stream);

/* Classification statistics and the soft-max cross-entropy of a multi-output forest in one interpretation (csrc/cls_stats.hip): for
 * every tree t, every row split g < n_groups (1 <= n_groups <= 8, else EVOGP_E_BADARG) and every class c < out_len (2 <= out_len <= 16)
 *   hits[t][g][c]      i32  rows of split g with label c that tree t predicts as c
 *   predicted[t][g][c] i32  rows of split g that tree t predicts as c
 *   loss[t][g]         f64  mean soft-max cross-entropy of tree t over the counted rows of split g
 * Rows: groups is i32[data_points] or NULL (every row in split 0).  Row d belongs to split groups[d] when 0 <= groups[d] < n_groups and is
 * COUNTED when besides 0 <= labels[d] < out_len; a row that is not counted is looked at in no output (a tree may be NaN there).
 * Prediction: the rule of evogp_hip_batch_argmax_count -- first maximum, index 0 when an output is NaN or the maximum is infinite,
 * near-ties as torch.argmax(clip(softmax(.))) settles them -- so the sum of hits[t] equals its counts[t] when every row is counted.
 * Cross-entropy of a counted row with float32 outputs x_o and label y, in float32: m = max_o x_o; a NaN output or an infinite m POISONS
 * the row: loss[t][g] of its split, and only of its split, is NaN; otherwise s = sum_o expf(x_o - m) with o ascending and
 * l = logf(s) - (x_y - m) clamped to [0, 34.538776] (= -log(1e-15)).  loss[t][g] = (sum of l in float64) / (number of counted rows of g
 * = sum_c predicted[t][g][c]); an empty split gives NaN.  A malformed tree has every output NaN: class 0 on every counted row, loss NaN.
 * Sums: the counts by integer atomics; the float64 sums without atomics -- a lane's rows ascending, the 64 lanes by the fixed wave
 * reduction, the row tiles in tile order -- and every l enters as a part on the 2^-20 grid plus its remainder, so that both column sums are
 * exact for data_points < 2^26: the loss is bit-identical from run to run, independent of the population around the tree, and a split's
 * column equals that of a call on the split's rows alone.  No (pop, data_points, out_len) array is written, nothing synchronises with the
 * host; the partial sums (16 bytes per tree, tile of 64 or 128 rows and split, the population in slices of at most 128 MiB) live in the
 * stream's workspace (evogp_hip_release_workspaces), so a call of a new shape cannot be captured into a graph before one eager call.
 * The outputs must not alias the inputs or one another.  Errors as evogp_hip_batch_argmax_count: BADARG, NULLPTR, UNSUPPORTED. */
int evogp_hip_batch_class_stats(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                const int *labels, const int *groups /* may be NULL */, unsigned n_groups, int *hits, int *predicted,
                                double *loss, evogp_stream_t stream);

/* Prepared forward pass of a MULTI-OUTPUT population (no counterpart in the reference's ABI).  The
 * reference's rollout problems call `evaluate` once per environment step on the same forest, 1000 times per generation
 * (src/evogp/problem/brax_problem.py:54-93).  In multi-output mode only nodes flagged OUT are observable and their operands
 * are leaves (forward.cu:237-243: every function hands its last operand on), so a tree reduces to a short list of
 * "outs[o] += f(leaf, leaf)".  _prepare builds the lists once per forest into `workspace` (device memory,
 * >= evogp_hip_evaluate_workspace_bytes, 16-byte aligned; the last 64 bytes hold an int: the number of trees the lists cannot
 * express); _prepared evaluates results[n][:] = tree_n(variables[n][:]) from them — same values as evogp_hip_evaluate, bit for
 * bit (same operations in the same order) — and, when with_fallback != 0, runs the stack interpreter on the trees counted
 * above (pass 0 only if that count, read back after _prepare, is 0).  out_len in [2, 32], var_len <= 255. */
size_t evogp_hip_evaluate_workspace_bytes(unsigned pop_size, unsigned gp_len);
int evogp_hip_evaluate_prepare(unsigned pop_size, unsigned gp_len, unsigned var_len, unsigned out_len,
                               const float *value, const int16_t *type, const int16_t *size,
                               void *workspace, size_t workspace_bytes, evogp_stream_t stream);
int evogp_hip_evaluate_prepared(unsigned pop_size, unsigned gp_len, unsigned var_len, unsigned out_len,
                                const float *value, const int16_t *type, const int16_t *size,
                                const void *workspace, int with_fallback,
                                const float *variables, float *results, evogp_stream_t stream);

/* Linear scaling (Keijzer 2003; no counterpart in the reference): the mean squared error of  a + b * T(x)  with the least-squares
 * a, b of every single-output tree T, from three float64 sums per tree taken in the evaluation kernel's epilogue (csrc/sr_scale.hip):
 * no (pop, D) prediction matrix exists.  With p_d the float32 prediction on row d (the bits evogp_hip_batch_evaluate stores),
 * ybar the float64 mean of the labels, v_d = (double)y_d - ybar, Syy = sum v_d^2, and per tree Sp = sum p_d, Spp = sum p_d^2,
 * Spv = sum p_d v_d (float64), var = Spp/D - (Sp/D)^2, cov = Spv/D:
 *   malformed tree, or a p_d that is not finite      loss = intercept = slope = NaN
 *   min_d p_d == max_d p_d, or var <= 0, or D == 1   slope = 0, intercept = ybar, loss = Syy/D
 *   otherwise                                        slope = cov/var, intercept = ybar - slope*Sp/D, loss = max(0, Syy/D - slope*cov),
 *                                                    in float64, rounded once to float32; all three NaN if a rounded coefficient is not finite
 * coef is (pop, 2): intercept, slope.  Sums have a fixed order (lane partials over the wave's row tiles in ascending order, the 64
 * lanes by a fixed butterfly, the waves in ascending order): the output is bit-identical from run to run and does not depend on the
 * other rows of the forest.  ybar and Syy come from a one-workgroup kernel in front and stay on the device: nothing synchronises with
 * the host, and the call can be captured into a HIP graph once one eager call on the stream has been made.
 * Any gp_len <= 1024, var_len and data_points; out_len != 1 returns EVOGP_E_UNSUPPORTED. */
int evogp_hip_sr_linear_scaling(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                const float *labels, float *loss, float *coef, evogp_stream_t stream);

/* Row t (length len) becomes the prefix tree ADD(MUL(T, slope), intercept): word 0 = ADD (size len + 4), word 1 = MUL (size len + 2: the tree and the slope),
 * words 2 .. len + 1 the old tree, then CONST slope and CONST intercept, zero tail words, applied[t] = 1.  The output rows have
 * out_gp_len >= gp_len words.  A row whose len + 4 exceeds out_gp_len, whose coefficients are not both finite or which is malformed
 * is copied unchanged (tail words beyond gp_len zero) with applied[t] = 0.  coef is (pop, 2): intercept, slope.  Not in place. */
int evogp_hip_wrap_linear(unsigned pop_size, unsigned gp_len, unsigned out_gp_len, const float *value, const int16_t *type,
                          const int16_t *size, const float *coef, float *out_value, int16_t *out_type, int16_t *out_size,
                          unsigned char *applied, evogp_stream_t stream);

/* Multi-gene SR fitness (GPTIPS; Arnaldo et al. 2014 "MRGP"; no counterpart in the reference): linear scaling above generalised from one
 * column to G.  The G = out_len outputs of a tree are FEATURES g_1 .. g_G, the model is  yhat = b0 + sum_j w_j g_j(x)  with the
 * least-squares b0, w of every tree, and the loss is its mean squared error (csrc/sr_genes.hip): one pass over the dataset per tree,
 * G(G+5)/2 sums, no (pop, D, G) matrix.  1 <= G <= EVOGP_GENES_MAX, else EVOGP_E_UNSUPPORTED; labels is (D,).
 * g_jd is the float32 value evogp_hip_batch_evaluate stores in output j on row d: for G = 1 the tree's value, for G > 1 the
 * multi-output conventions (the sum of the nodes flagged for output j, 0 when none is, an output index >= G ignored).  ybar,
 * v_d = (double)y_d - ybar and Syy = sum v_d^2 are those of linear scaling, bit for bit.
 * Moments, float64:  m_j = mean_d g_j,  C_ij = mean_d (g_i - m_i)(g_j - m_j),  c_j = mean_d (g_j - m_j) v_d;  per gene also the float32
 * minimum and maximum and "some value is not finite".  They are taken in one pass as SHIFTED sums: every wave that accumulates on
 * its own subtracts from gene j the value a_j the gene has on the first row the wave sees before it multiplies and adds (a row past D
 * contributes exactly 0: the shifted value is masked), and the waves' (n, mean, M2, co-moments) are merged in wave order by the pairwise
 * update of Chan, Golub & LeVeque (1983).  The uncentred Spp/D - (Sp/D)^2 of linear scaling is not good enough here: a gene that is a
 * constant plus float32 rounding noise has mean(g^2)/var up to 1e16.
 * Rules, one thread per tree, float64:
 *   malformed tree, or a gene value that is not finite            loss and every coefficient NaN
 *   gene j with min_d == max_d (exactly), C_jj <= 0, or D == 1    FLAT: weight exactly 0, no part in the solve
 *   the other genes, in index order, through an unrolled LDL^T    d_j = C_jj - sum over kept k < j of l_jk^2 d_k;  gene j is KEPT iff
 *                                                                 d_j > EVOGP_GENES_PIVOT_TOL * C_jj, else its weight is exactly 0 and
 *                                                                 it is left out of the later columns: it is collinear with the
 *                                                                 earlier genes up to float32 rounding
 *   kept set K                                                    C_KK w = c_K;  b0 = ybar - sum w_j m_j;
 *                                                                 loss = max(0, Syy/D - sum_K w_j c_j);  K empty: b0 = ybar, loss = Syy/D
 * rounded once to float32; if a rounded coefficient is not finite every output of the tree is NaN.  The tolerance is part of the
 * definition, not a tuning knob: an untruncated least-squares fit spends weights on rounding noise.
 * loss (pop,);  coef (pop, 1 + G): the intercept, then the weights;  moments (pop, G(G+5)/2) float64 or NULL: the means, the row-major
 * upper triangle of C, then c -- the very values the solve read.  A malformed tree has a NaN loss and a zero moments row.
 * Bit-identical from run to run; a tree's result does not depend on the other rows of the forest or on its position; nothing
 * synchronises with the host, and the call can be captured into a HIP graph once one eager call on the stream has been made.
 * Any gp_len <= 1024, var_len and data_points. */
#define EVOGP_GENES_MAX 8
#define EVOGP_GENES_PIVOT_TOL 9.313225746154785e-10 /* 2^-30 */
int evogp_hip_sr_gene_fitness(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                              const float *value, const int16_t *type, const int16_t *size, const float *variables,
                              const float *labels, float *loss, float *coef, double *moments /* nullable */, evogp_stream_t stream);

/* Weighted, robust and held-out losses (no counterpart in the reference, whose loss is the unweighted mean of squared or absolute errors
 * over every row): for every single-output tree t and each of K = n_weights weight rows, in one pass over the dataset
 * (csrc/sr_wloss.hip; no (pop, D) matrix exists),
 *     loss[t][k] = ( sum_d W[k][d] * rho(p_td - y_d) ) / sum_d W[k][d]
 * with p_td the float32 prediction on row d (the bits evogp_hip_batch_evaluate stores), r = (double)p_td - (double)y_d, and rho
 * evaluated in float64:
 *   EVOGP_LOSS_MSE      r^2
 *   EVOGP_LOSS_MAE      |r|
 *   EVOGP_LOSS_HUBER    r^2 / 2 for |r| <= delta, else delta (|r| - delta / 2);   loss_param = delta, finite and > 0
 *   EVOGP_LOSS_PINBALL  tau r_y for r_y >= 0, else (tau - 1) r_y, r_y = y - p;     loss_param = tau in (0, 1): the fit sits at the tau-quantile
 *   EVOGP_LOSS_LOGCOSH  |r| + log1p(exp(-2 |r|)) - log 2  (log cosh r in a form that cannot overflow)
 * weights is f32[K][D], 1 <= K <= EVOGP_WLOSS_MAX_WEIGHTS, or NULL with n_weights == 1: every weight is 1 and no weight is loaded.  One
 * sample-weight row, two 0/1-masked rows (training and validation), K folds or bootstrap replicates are all this call.
 * Rules that decide a value exactly:
 *   - a row with W[k][d] == 0 is NOT LOOKED AT in column k: it adds exactly 0 whatever p_td is, NaN and inf included (which
 *     case_errors @ W cannot give: 0 * NaN is NaN);
 *   - loss[t][k] is NaN when some row with W[k][d] != 0 has a prediction that is not finite, or when the tree is malformed (the rule
 *     of evogp_hip_sr_linear_scaling: length clamped to [0, gp_len], not empty, no stack underflow, one value left);
 *   - a weight row that holds a negative or non-finite weight, or whose sum is 0, gives NaN for every tree.  A one-workgroup kernel in
 *     front decides that on the device and leaves sum_d W[k][d] (float64, fixed order: thread i of 256 adds rows i, i + 256, ..., the
 *     lanes by the fixed butterfly, the waves in ascending order) and the flag there: nothing synchronises with the host;
 *   - the result is (float)(S / Wsum) from float64, and may be +inf;
 *   - column k depends on the tree, the dataset, W[k], the kind and the parameter only: not on K, the other weight rows, the other
 *     trees or the run.  It is bit-identical from run to run, and weights == NULL gives the bits of a row of ones.
 * No float atomics.  Sums have the fixed order of evogp_hip_sr_linear_scaling: lane partials over the wave's row tiles in ascending
 * order, the 64 lanes by a fixed butterfly, the waves in ascending order.  loss is f32[pop][K].  The call can be captured into a HIP
 * graph once one eager call on the stream has been made.
 * EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024, n_weights outside 1 .. 8 or != 1 with weights == NULL, an unknown
 * kind, a NaN loss_param, a delta that is not finite and positive, a tau outside (0, 1).  Then out_len != 1: EVOGP_E_UNSUPPORTED; then a
 * NULL pointer other than weights: EVOGP_E_NULLPTR.  Any gp_len <= 1024, var_len and data_points. */
#define EVOGP_WLOSS_MAX_WEIGHTS 8
#define EVOGP_LOSS_MSE 0
#define EVOGP_LOSS_MAE 1
#define EVOGP_LOSS_HUBER 2
#define EVOGP_LOSS_PINBALL 3
#define EVOGP_LOSS_LOGCOSH 4
int evogp_hip_sr_weighted_loss(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                               const float *value, const int16_t *type, const int16_t *size, const float *variables,
                               const float *labels, const float *weights /* nullable */, unsigned n_weights, int loss_kind,
                               double loss_param, float *loss, evogp_stream_t stream);

/* Constant tuning under sample weights, robust losses and held-out rows (no counterpart in the reference):
 * evogp_hip_sr_gradient and evogp_hip_sr_normal_eq for the loss evogp_hip_sr_weighted_loss scores by, on the rows it scores.  Single-
 * output trees, one label column, ONE weight row w = f32[D], or NULL: every weight is 1.  p_d is the float32 prediction of the tape's
 * forward walk, r_d = (double)p_d - (double)y_d, Wsum = sum_d w_d in float64 in the fixed order of evogp_hip_sr_weighted_loss (D without w).
 *   loss[t]     = (float)( sum over the rows with w_d != 0 of w_d * rho(r_d) / Wsum ), rho in float64 as in evogp_hip_sr_weighted_loss;
 *   grad[t][i]  = d loss[t] / d value[t][i] at every CONST node i, exactly 0.0f elsewhere and on the tail: the reverse walk of
 *                 evogp_hip_sr_gradient seeded per row with (float)(w_d * rho'(r_d) / Wsum),
 *                     mse 2 r;  mae sign(r), 0 at r == 0;  huber r for |r| <= delta, else delta * sign(r);
 *                     pinball -tau for r < 0, 1 - tau for r > 0, 0 at r == 0;  logcosh tanh(r).
 *                 Adjoints and their accumulators are float32, as in evogp_hip_sr_gradient;
 *   normal[t]   (evogp_hip_sr_weighted_normal_eq, MSE) the 44 words of evogp_hip_sr_normal_eq over the same optimised constants:
 *                 A_ij = sum_d w_d J_i J_j / Wsum, b_i = sum_d w_d J_i r_d / Wsum, with loss[t] = sum_d w_d r_d^2 / Wsum.
 * Rules that decide a value exactly:
 *   - a row with w_d == 0 is NOT LOOKED AT: the tree may be NaN, infinite or divide by zero there, and nothing of that row reaches the
 *     loss, the gradient, A or b (a 64-row tile without a weighted row is not walked at all);
 *   - the loss is NaN and the grad / normal row all zero when the tree is malformed, when a row WITH weight has a prediction that is
 *     not finite (the rule of evogp_hip_sr_weighted_loss; evogp_hip_sr_gradient lets inf through), or when the weight row holds a
 *     negative or non-finite weight or sums to 0 -- then for every tree.  The last is decided on the device by the one-workgroup kernel
 *     of evogp_hip_sr_weighted_loss; nothing synchronises with the host.  evogp_hip_sr_const_step and evogp_hip_sr_lm_step never
 *     accept a NaN loss and propose no move from one: such trees keep their constants;
 *   - no float atomics: the same inputs give the same bits.  Rows are split among the waves as in evogp_hip_sr_gradient (the same plan),
 *     a lane's loss terms are added in float64 in ascending tile order, the 64 lanes by the fixed butterfly, the waves in wave order;
 *     the two calls see the same rows in the same order, so for EVOGP_LOSS_MSE their losses are equal bit for bit;
 *   - multiplying every weight by a power of two changes no bit of any result (barring overflow and underflow).
 * EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024, an unknown kind, a NaN loss_param, a delta that is not finite and
 * positive, a tau outside (0, 1).  Then out_len != 1: EVOGP_E_UNSUPPORTED; then a NULL pointer other than weights: EVOGP_E_NULLPTR.
 * Rows of more than 64 nodes use the per-stream tape buffer of evogp_hip_sr_gradient, under the same rules. */
int evogp_hip_sr_weighted_gradient(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                   const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                   const float *labels, const float *weights /* nullable */, int loss_kind, double loss_param,
                                   float *loss, float *grad, evogp_stream_t stream);
int evogp_hip_sr_weighted_normal_eq(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                    const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                    const float *labels, const float *weights /* nullable */, float *loss, float *normal,
                                    evogp_stream_t stream);

/* Linear scaling under sample weights with held-out scoring, in ONE pass over the dataset (no counterpart in the reference; DESIGN.md
 * section 3.22).  Single-output trees, one label column, squared error.  weights is f32[K][D], 1 <= K <= EVOGP_WLOSS_MAX_WEIGHTS, or
 * NULL with n_weights == 1: every weight is 1 and no weight is loaded.  Row 0 is the FIT row, rows 1 .. K-1 are SCORE rows: the
 * least-squares a + b * T(x) is fitted on row 0 and every row, row 0 included, is scored with those coefficients -- a training row and a
 * validation row of 0/1 masks give the held-out error of the model fitted without the held-out rows.
 * p_d is the float32 prediction on row d (the bits evogp_hip_batch_evaluate stores).  All arithmetic is float64, the outputs are
 * rounded once to float32.  With W_k = sum_d W[k][d],
 *     ybar0 = sum_d W[0][d] y_d / W_0,        v_d = (double)y_d - ybar0,
 * and per row k, over the data rows with W[k][d] != 0:  m_k the weighted mean of p,  M_k = sum w (p - m_k)^2,
 * vbar_k = sum w v / W_k,  c_k = sum w (p - m_k)(v - vbar_k),  V_k = sum w (v - vbar_k)^2:
 *   fit     b = c_0 / M_0,   a = ybar0 + vbar_0 - b m_0                                                  coef[t] = { a, b }
 *   score   delta_k = b (m_k - m_0) - (vbar_k - vbar_0),
 *           loss[t][k] = max(0, b^2 M_k - 2 b c_k + V_k + W_k delta_k^2) / W_k,   which is sum_d W[k][d] (a + b p_d - y_d)^2 / W_k with
 *           the unrounded a, b; for k = 0 it is max(0, V_0 - b c_0) / W_0.
 * Rules that decide a value exactly:
 *   - flat: a tree is flat when min p == max p over the rows with W[0][d] != 0 (decided on the float32 values), or M_0 <= 0, or
 *     exactly one row has weight in row 0.  Then b = 0, a = ybar0 + vbar_0, and every column uses the formula above with b = 0;
 *   - a data row with W[k][d] == 0 is NOT LOOKED AT in column k: its prediction may be NaN or infinite, in the sums and in the
 *     minimum and maximum of the flat rule alike;
 *   - loss[t][k] is NaN when some row with W[k][d] != 0 has a prediction that is not finite.  If k == 0, the coefficients and every
 *     column of that tree are NaN.  A malformed tree (the rule of evogp_hip_sr_linear_scaling) is NaN everywhere, and so is a tree whose
 *     a or b is not finite as float32;
 *   - a weight row that holds a negative or non-finite weight, or whose sum is 0, may not be used: if it is row 0, everything is NaN for
 *     every tree; if it is row k > 0, column k is NaN for every tree and the rest is untouched.  A one-workgroup kernel in front decides
 *     that on the device and leaves W_k (the order and the bits of evogp_hip_sr_weighted_loss), ybar0, vbar_k and V_k there:
 *     nothing synchronises with the host;
 *   - the sums are uncentred (sum w p, sum w p^2, sum w p v per column), every term carries the weight as a factor and enters its sum
 *     by one fused multiply-add (a prediction that is not finite enters as 0: its columns are NaN by the rule above), so multiplying a
 *     weight row by a power of two changes no bit of any output, barring overflow and underflow; any other positive factor changes
 *     the outputs by rounding only;
 *   - column k depends on the tree, the dataset, W[0] and W[k] only: not on K, the other weight rows, the other trees or the run.  It is
 *     bit-identical from run to run, and weights == NULL gives the bits of a row of ones.
 * No float atomics, no (pop, D) buffer.  Sums have the fixed order of evogp_hip_sr_linear_scaling: lane partials over the wave's row
 * tiles in ascending order, the 64 lanes by a fixed butterfly, the waves in ascending order.  loss is f32[pop][K], coef f32[pop][2]
 * (intercept, slope: what evogp_hip_wrap_linear takes).  The call can be captured into a HIP graph once one eager call on the stream
 * has been made.
 * EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024, n_weights outside 1 .. 8 or != 1 with weights == NULL.  Then
 * out_len != 1: EVOGP_E_UNSUPPORTED; then a NULL pointer other than weights: EVOGP_E_NULLPTR.  Any gp_len <= 1024, var_len and
 * data_points. */
int evogp_hip_sr_weighted_scaling(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                  const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                  const float *labels, const float *weights /* nullable */, unsigned n_weights, float *loss /* [pop][K] */,
                                  float *coef /* [pop][2]: intercept, slope */, evogp_stream_t stream);

/* Input gradients of single-output trees on the rows of the dataset, and the derivative loss computed from them (no counterpart in the
 * reference; csrc/sr_xgrad.hip).  p_d is the float32 prediction of the tape's forward walk on row d (the walk of
 * evogp_hip_sr_gradient), g_{k,d} = d tree / d x_{wrt[k]} at X[d]: the reverse walk of evogp_hip_sr_gradient seeded with 1.0f at the root,
 * adjoints in float32 by the same rules (DESIGN.md "Constant gradients"; an IF gives 0 to its condition, its adjoint to the branch it
 * took and 0 to the other).  g_{k,d} is the float32 sum, starting from +0.0f, of the adjoints of the VAR nodes that hold variable wrt[k],
 * in prefix order: +0.0f exactly for a variable the tree does not hold, 1.0f for a root that is that variable.
 * NaN: the rules are the constant gradient's and are not repaired.  0 * NaN is NaN, so a NaN or infinite value in a branch that was NOT
 * taken (IF, max, min) can make a derivative NaN on a row whose prediction is finite.
 *   evogp_hip_sr_input_gradient   pred f32[pop][D] = p_d, dpred f32[n_wrt][pop][D] = g_{k,d}.  A malformed tree (the rule of
 *                                 evogp_hip_sr_gradient) has NaN in every word of its rows of both.
 *   evogp_hip_sr_derivative_loss  writes no (pop, D) array.  loss f32[pop][1 + n_wrt], violations i32[pop][n_wrt]:
 *       loss[t][0]     = (float)( sum_d ((double)p_d - (double)labels[d])^2 / D ): equal bit for bit to the loss of
 *                        evogp_hip_sr_weighted_gradient with weights == NULL and EVOGP_LOSS_MSE (same plan, same walk, same order);
 *       loss[t][1 + k] = (float)( sum_d ((double)g_{k,d} - (double)dlabels[d][k])^2 / D ); dlabels f32[D][n_wrt], or NULL: every label
 *                        is 0 and the column is the mean squared sensitivity of the tree to the variable;
 *       a column is NaN exactly when one of its row terms is not finite (sqrt(x0) at x0 == 0: column 0 finite, the x0 column NaN);
 *       violations[t][k] = the number of rows with !(dmin[k] <= g_{k,d} && g_{k,d} <= dmax[k]); a NaN derivative counts.  dmin / dmax:
 *                        f32[n_wrt] on the device, or NULL: -inf / +inf, and then only NaN counts;
 *       a malformed tree has NaN in every column and violations = D.
 *     Sums are float64 per lane over the wave's row tiles in ascending order, the 64 lanes by the fixed butterfly, the waves in wave
 *     order; violations are counted per tile by ballot and added as integers in the same order.
 * wrt: int32[n_wrt] ON THE HOST, read before the call returns (unlike evogp_hip_tree_derivative_intervals, whose wrt lives on the device
 * and is the caller's to check: here the entries are checked before any launch and nothing synchronises with the host); 1 <= n_wrt <=
 * EVOGP_XGRAD_MAX_VARS, entries distinct and in [0, var_len).
 * EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024, var_len >= 2^28, n_wrt outside 1 .. 8, an entry of wrt out of range or
 * repeated.  Then a NULL pointer other than dlabels, dmin, dmax: EVOGP_E_NULLPTR; then out_len != 1: EVOGP_E_UNSUPPORTED.
 * One launch each, no float atomics: bit-identical from run to run.  Rows of more than 64 nodes use the per-stream tape buffer of
 * evogp_hip_sr_gradient, under the same rules.  Any data_points and var_len; the outputs must not alias the inputs or one another. */
#define EVOGP_XGRAD_MAX_VARS 8
int evogp_hip_sr_input_gradient(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                const float *value, const int16_t *type, const int16_t *size, const float *variables, unsigned n_wrt,
                                const int *wrt /* host */, float *pred /* [pop][D] */, float *dpred /* [n_wrt][pop][D] */,
                                evogp_stream_t stream);
int evogp_hip_sr_derivative_loss(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                 const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                 const float *labels, const float *dlabels /* nullable */, unsigned n_wrt, const int *wrt /* host */,
                                 const float *dmin /* nullable */, const float *dmax /* nullable */, float *loss /* [pop][1 + n_wrt] */,
                                 int *violations /* [pop][n_wrt] */, evogp_stream_t stream);

/* Semantic backpropagation over single-output trees on the rows of the dataset (Pawlak, Wieloch & Krawiec 2015; no counterpart in the
 * reference; csrc/sr_backprop.hip, DESIGN.md section 3.24, which holds the rule table; tests/backprop_ref.py restates it).  pos i32[pop]
 * names one node per tree.  The tree is inverted from the root down to that node: per row d a target t and a state, (labels[d], REQUIRED)
 * at the root, one float32 operation per function node on the path, the other operands' values taken from the tape of the forward walk
 * of evogp_hip_sr_gradient.  States: 0 REQUIRED (the subtree must return t), 1 FREE (any value reproduces the label), 2 IMPOSSIBLE (none
 * does); FREE and IMPOSSIBLE are absorbing.  status i32[pop]: 0 ok; 1 the row is malformed (the rule of evogp_hip_sr_gradient); 2 pos is
 * outside [0, length); 3 BLOCKED: a function on the path has no rule (the loose variants, pow, the comparisons, the trigonometric and
 * hyperbolic functions, unknown ids, and an IF entered through its condition).  With status != 0 nothing is inverted and every row counts
 * as IMPOSSIBLE.  The ancestors of pos are those the subtree sizes of a well-formed row give; they are taken from the node types, so no
 * size word but the root's is read.
 *   evogp_hip_sr_desired          desired f32[pop][D]: t where the state is REQUIRED, NaN elsewhere; state u8[pop][D]; status.
 *   evogp_hip_sr_backprop_match   writes no (pop, D) array.  lib_t f32[D][n_lib]: the semantics of a library of n_lib subtrees, TRANSPOSED
 *                                 (entry k on row d at lib_t[d][k]), 1 <= n_lib <= EVOGP_BACKPROP_MAX_LIB.
 *       dist f64[pop][n_lib]   sum over the REQUIRED rows of ((double)t_d - (double)lib_t[d][k])^2; +inf when lib_t[d][k] is not finite on
 *                              a REQUIRED row; 0 without a REQUIRED row;
 *       best i32[pop]          the entry of least dist, the smallest on ties; -1 with status != 0, without a REQUIRED row, or when every
 *                              dist is +inf;
 *       cnst f32[pop], const_dist f64[pop]   the mean of t over the REQUIRED rows and their centred sum of squares (what a constant
 *                              subtree would cost), from float64 sums shifted by a REQUIRED value of the tree; NaN without a REQUIRED row;
 *       counts i32[pop][3]     the REQUIRED, FREE and IMPOSSIBLE rows; status as above.
 *     Sums are float64: a lane owns the entries lane, lane + 64, ... and adds the REQUIRED rows of the wave's tiles in ascending order,
 *     the waves are added in wave order.
 * EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024, n_lib outside 1 .. 1024.  Then a NULL pointer: EVOGP_E_NULLPTR; then
 * out_len != 1: EVOGP_E_UNSUPPORTED.  One launch each, no float atomics, nothing synchronises with the host: bit-identical from run to run.
 * Rows of more than 64 nodes use the per-stream tape buffer of evogp_hip_sr_gradient, under the same rules.  The outputs must not alias
 * the inputs or one another. */
#define EVOGP_BACKPROP_MAX_LIB 1024
int evogp_hip_sr_desired(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len, const float *value,
                         const int16_t *type, const int16_t *size, const float *variables, const float *labels, const int *pos,
                         float *desired /* [pop][D] */, unsigned char *state /* [pop][D] */, int *status /* [pop] */, evogp_stream_t stream);
int evogp_hip_sr_backprop_match(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                const float *value, const int16_t *type, const int16_t *size, const float *variables, const float *labels,
                                const int *pos, unsigned n_lib, const float *lib_t /* [D][n_lib] */, double *dist /* [pop][n_lib] */,
                                int *best, float *cnst, double *const_dist, int *counts /* [pop][3] */, int *status, evogp_stream_t stream);

/* Approximately geometric semantic crossover (AGX, the second operator of the same paper; tests/agx_ref.py restates
 * it): the two entries above with the labels replaced by a MATE.  The mates are a second forest of n_mates rows of the same gp_len and
 * var_len, one output; mate i32[pop] names the mate's row of every tree.  With a = T_t(x_d) and b = T_mate[t](x_d) as
 * evogp_hip_sr_gradient's forward walk computes them, the root target on row d is mid = 0.5f * a + 0.5f * b (two scalings and one float32
 * addition): (mid, REQUIRED) where mid is finite, IMPOSSIBLE from the root down where it is not (a NaN or an infinity in either parent,
 * inf - inf).  From there the rule table of section 3.24 applies unchanged, so at pos = 0 the desired values are the midpoints.  status
 * gains 4: mate[t] is outside [0, n_mates), or the mate's row is malformed; the codes are decided in the order 1, 2, 4, 3.  No mate size
 * word but the root's is read.  The outputs, the library, the order of summation and the order of the argument checks are those of the
 * two entries above; n_mates == 0 is EVOGP_E_BADARG.  One launch each, no (pop, D) array, no float atomics, no host synchronisation. */
int evogp_hip_sr_desired_mid(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len, const float *value,
                             const int16_t *type, const int16_t *size, const float *variables, unsigned n_mates, const float *mvalue,
                             const int16_t *mtype, const int16_t *msize, const int *mate /* [pop] */, const int *pos,
                             float *desired /* [pop][D] */, unsigned char *state /* [pop][D] */, int *status /* [pop] */, evogp_stream_t stream);
int evogp_hip_sr_agx_match(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len, const float *value,
                           const int16_t *type, const int16_t *size, const float *variables, unsigned n_mates, const float *mvalue,
                           const int16_t *mtype, const int16_t *msize, const int *mate /* [pop] */, const int *pos, unsigned n_lib,
                           const float *lib_t /* [D][n_lib] */, double *dist /* [pop][n_lib] */, int *best, float *cnst, double *const_dist,
                           int *counts /* [pop][3] */, int *status, evogp_stream_t stream);

/* The semantic signature of EVERY SUBTREE, and a library of semantically distinct subtrees chosen from those signatures (the
 * population-based library of the same paper; csrc/sr_subtree_sig.hip; tests/sublib_ref.py restates both).
 * evogp_hip_sr_subtree_signatures, single-output forests only: with v_i the float32 value of the subtree rooted at node i as
 * evogp_hip_sr_subtree_errors' forward walk computes it and sig() the signature of evogp_hip_sr_semantic_hash above (same key, same
 * terms, same last mix),
 *     sig_out[t][i] = sig of the row of values v_i(X[0]), ..., v_i(X[D - 1])        for i < len(t), tree t well formed
 *     sig_out[t][i] = 0                    on the tail [len, gp_len) and on every entry of a malformed tree
 * so sig_out[t][0] is evogp_hip_sr_semantic_hash's word of tree t and sig_out[t][i] is its word for the row that holds the nodes
 * [i, i + size[t][i]) from position 0, bit for bit.  One launch with the plan of the tape passes (a workgroup per tree, its waves split
 * the 64-row tiles); the per-node sum is integer and modular, so no order of lanes, tiles or waves changes it.  No atomics, no labels,
 * nothing synchronises with the host.  Rows of more than 64 nodes use the per-stream tape buffer of evogp_hip_sr_gradient, under the same
 * rules.  EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024, out_len != 1; then a NULL pointer: EVOGP_E_NULLPTR.
 *
 * evogp_hip_subtree_library_select: sig u64[pop][gp_len] (the entry above, or any array in which equal words mean "the same"), size
 * i16[pop][gp_len] (the forest's subtree sizes), 1 <= min_size <= max_size, 1 <= k <= EVOGP_BACKPROP_MAX_LIB, pop * gp_len < 2^31.
 *     ELIGIBLE         the flat index f = t * gp_len + i with sig[f] != 0 and min_size <= size[f] <= max_size.  A live subtree whose
 *                      signature happens to be exactly 0 is dropped (one word in 2^64).
 *     CLASS            the eligible nodes of one signature; its COUNT is their number
 *     REPRESENTATIVE   the member with the smallest (size, f)
 *     ORDER            the classes by (count descending, representative's f ascending) -- a total order
 *     member_out i32[k]   the representative's flat index of the j-th class in that order, -1 past the last class
 *     count_out i32[k]    its count, 0 there
 *     n_classes_out i32[1]   the number of classes (it may exceed k)
 * The outputs are fully determined by the inputs: bit-identical from run to run.  Signatures CHOOSE the classes and nothing verifies
 * them: a collision merges two semantics into one class and costs the library one member, never a wrong result -- whoever uses the
 * library recomputes its semantics from the extracted trees.  Two stable sorts over the pop * gp_len words with 64-bit integer atomics
 * (minimum) for the representatives; everything on the caller's stream, nothing synchronises with the host, the engine allocates nothing.
 * workspace: evogp_hip_subtree_library_select_workspace_bytes(pop, gp_len) bytes, no zeroing needed.  EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024,
 * pop * gp_len >= 2^31, min_size < 1, max_size < min_size, k outside 1 .. 1024; then a NULL pointer: EVOGP_E_NULLPTR. */
int evogp_hip_sr_subtree_signatures(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                    const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                    unsigned long long *sig_out /* [pop][gp_len] */, evogp_stream_t stream);
int evogp_hip_subtree_library_select_workspace_bytes(unsigned pop_size, unsigned gp_len, unsigned long long *bytes);
int evogp_hip_subtree_library_select(unsigned pop_size, unsigned gp_len, const unsigned long long *sig, const int16_t *size, int min_size,
                                     int max_size, int k, int *member_out /* [k] */, int *count_out /* [k] */, int *n_classes_out /* [1] */,
                                     void *workspace, evogp_stream_t stream);

/* Exact semantic intron removal (no counterpart in the reference; csrc/sr_introns.hip; tests/intron_ref.py
 * restates both entries), single-output forests only: a node whose subtree takes the value of one of its own descendants on EVERY data
 * row computes nothing (x + 0, 1 * x, max(x, x), neg(neg(x)), IF(c, a, a), (x * 2) / 2, ...) and is replaced by that descendant.
 *     E(a, b)     two float32 values are EQUAL when they have one bit pattern or are both NaN; +0.0 and -0.0 are NOT equal
 *     n, span(i)  the live length size[t][0] kept inside [0, gp_len], and size[t][i] kept inside [1, n - i] (evogp_hip_prune_rows' reading)
 * evogp_hip_sr_subtree_introns: sig u64[pop][gp_len] is evogp_hip_sr_subtree_signatures' output for the same forest and rows -- or any
 * array whatever: SIGNATURES PROPOSE, THE TAPE VERIFIES.  For a well-formed tree (classify_tree == TREE_OK) and i < n
 *     cand(i)        sig[t][i] != 0: the j with i < j < i + span(i) and sig[t][j] == sig[t][i] of smallest (span(j), j); i if there is
 *                    none or sig[t][i] == 0
 *     rep_out[t][i]  cand(i) when cand(i) != i and E(v_i(X[d]), v_cand(i)(X[d])) on every row d < D, v_i the float32 value of the subtree
 *                    at node i as evogp_hip_sr_subtree_signatures' forward walk computes it; otherwise i.  A candidate that fails is
 *                    NOT replaced by the next one (the causes: -0 against +0, or a collision of two 64-bit words; a known miss)
 *     rep_out[t][i]  i on the tail [n, gp_len) and on every entry of a malformed tree
 * Every function of the interpreter decides by comparison or propagates NaN (max / min are a >= b ? a : b), so a subtree replaced by one
 * that is E-equal on every row leaves every ancestor E-equal on every row.  One launch with the plan of the tape passes and one tape word
 * per node and lane; a tree without any candidate walks nothing.  No atomics, no float reductions, nothing synchronises with the host,
 * bit-identical from run to run.  Rows of more than 64 nodes use the per-stream tape buffer of evogp_hip_sr_gradient, under the same
 * rules.  EVOGP_E_BADARG before any launch: a zero size, gp_len > 1024, out_len != 1; then a NULL pointer: EVOGP_E_NULLPTR.
 *
 * evogp_hip_remove_introns: the rewrite.  rep i16[pop][gp_len] is trusted in nothing: an entry with rep[t][i] <= i or rep[t][i] >= i +
 * span(i) counts as i.  For a well-formed tree, R(i) emits node rep[i] and then R(c) for each child c of rep[i] (the children of a node
 * r are found by their spans from r + 1); the new tree is R(0).  The decision is hierarchical: the rep of a node that is itself dropped
 * deletes nothing.  A kept node's new size is the number of kept nodes in its span; [new_len, gp_len) is zero in all three arrays;
 * removed_out[t] = n - new_len.  A malformed row is copied as it is, with removed_out[t] = 0.  Not in place: an output array that is its
 * input is EVOGP_E_BADARG, as are a zero size and gp_len > 1024; then a NULL pointer: EVOGP_E_NULLPTR.  One wave per tree, nothing
 * synchronises with the host. */
int evogp_hip_sr_subtree_introns(unsigned pop_size, unsigned data_points, unsigned gp_len, unsigned var_len, unsigned out_len,
                                 const float *value, const int16_t *type, const int16_t *size, const float *variables,
                                 const unsigned long long *sig /* [pop][gp_len] */, int16_t *rep_out /* [pop][gp_len] */,
                                 evogp_stream_t stream);
int evogp_hip_remove_introns(unsigned pop_size, unsigned gp_len, const float *value, const int16_t *type, const int16_t *size,
                             const int16_t *rep /* [pop][gp_len] */, float *value_out, int16_t *type_out, int16_t *size_out,
                             int *removed_out /* [pop] */, evogp_stream_t stream);

/* Pairwise semantic moments (no counterpart in the reference; csrc/sr_pair.hip; tests/pair_ref.py restates it):
 * how far apart two single-output models are on a dataset, and what combining them gives.  For `events` events, one FIRST tree of forest
 * A (pop_a rows of gp_len_a words) against n_cand <= EVOGP_PAIR_MAX_CANDIDATES CANDIDATE trees of forest B (pop_b rows of gp_len_b
 * words; the same arrays as A, or others of the same var_len): first i32[events] indexes A, candidates i32[events][n_cand] indexes B.
 *     p_t[d]   the float32 prediction of tree t on row d of variables (data_points, var_len): evogp_hip_batch_evaluate's bits
 *     r_t[d]   (double)p_t[d] - (double)labels[d]; labels == NULL: every label is 0, the moments are those of the predictions
 * With a = first[e], b = candidates[e][m]:
 *     own_out[e]            = sum_d r_a[d]^2                                   f64[events]
 *     moments_out[e][m][0]  = sum_d r_b[d]^2                                   f64[events][n_cand][3]
 *     moments_out[e][m][1]  = sum_d r_a[d] * r_b[d]
 *     moments_out[e][m][2]  = sum_d ((double)p_a[d] - (double)p_b[d])^2        (taken directly, not as Saa - 2 Sab + Sbb)
 * A tree is UNUSABLE when it is malformed (the structural pre-pass of the SR kernels refuses it), when its prediction is not finite on
 * some row, or when its index lies outside its forest.  An unusable first tree makes own_out[e] and every word of moments_out[e] NaN; an
 * unusable candidate makes its three words NaN.  Decided on the device by flags; a word of usable trees is always finite.
 * The D terms of a word are added in ONE order that depends on data_points alone (csrc/sr_pair_order.hpp: the rows of a lane in a tile
 * of 256, the 64 lanes, the tiles of a wave slot, the wave slots), in explicit fma / add calls, in every kernel of the pass.  So the
 * words of a pair are a function of its two trees, variables and labels: bit for bit the same in another event or slot, under another
 * n_cand or events, next to other candidates, in other populations, whichever kernel takes it; Sab and Sdd of (a, b) equal those of
 * (b, a); moments_out[e][m][0] equals own_out[e'] where candidates[e][m] and first[e'] are one tree; run to run.
 * Launches: the register interpreter (LEAN then FULL build) over batches of events, a first tree interpreted once per row tile and its
 * candidates after it (n_cand + 1 interpretations per event and tile), then the scratch-stack kernel over the events with a tree deeper
 * than 16 operands; var_len > 32: the scratch-stack kernel alone, a wave per pair.  No float atomics, no (pop, D) array, everything on
 * the caller's stream, nothing synchronises with the host, the engine allocates nothing.  workspace:
 * evogp_hip_sr_pair_moments_workspace_bytes(events, n_cand) bytes (a mark byte per event; no zeroing needed).
 * Before any launch: EVOGP_E_BADARG for n_cand == 0 or > 16, a zero data_points / var_len / pop / gp_len, gp_len > 1024, a size
 * >= 2^31; then EVOGP_E_NULLPTR for a NULL pointer other than labels.  events == 0 is EVOGP_OK and launches nothing (first, candidates,
 * the outputs and the workspace may then be NULL).  The ABI is single-output by construction: there is no out_len. */
#define EVOGP_PAIR_MAX_CANDIDATES 16
int evogp_hip_sr_pair_moments_workspace_bytes(unsigned events, unsigned n_cand, unsigned long long *bytes);
int evogp_hip_sr_pair_moments(unsigned events, unsigned n_cand, unsigned data_points, unsigned var_len, unsigned pop_a, unsigned gp_len_a,
                              const float *value_a, const int16_t *type_a, const int16_t *size_a, unsigned pop_b, unsigned gp_len_b,
                              const float *value_b, const int16_t *type_b, const int16_t *size_b, const float *variables,
                              const float *labels /* [data_points] or NULL */, const int *first /* [events] */,
                              const int *candidates /* [events][n_cand] */, double *own_out /* [events] */,
                              double *moments_out /* [events][n_cand][3] */, void *workspace, evogp_stream_t stream);

/* Engine-owned device memory (no counterpart in the reference, whose kernels keep a private copy of the tree per thread,
 * forward.cu:284-287).  evogp_hip_sr_fitness compiles every tree into PROGRAM RECORDS that its interpreter kernel reads: one
 * buffer per device, allocated with hipMalloc on first use, grown on demand (never while a HIP graph is being captured),
 * reused by every later eager call on that device and invisible to the caller's allocator; calls recorded into HIP graphs share a
 * second buffer of the same law that eager calls never touch (at most two population-sized buffers per device: round 5).  Size law:
 *     bytes = ceil(pop_size * 256 / 4096) * 4096 * max(2, ceil((gp_len + 2) / 31))    (+ 1/8 slack when it grows)
 * i.e. 768 MB for 1 M trees of gp_len 64 (three arrays of records; two up to gp_len 60), 8.7 GB for 1 M trees of gp_len 1024.
 * A single-output forest of gp_len <= 64 whose function mask (evogp_hip_sr_fitness_hinted) holds no unary function has programs of at
 * most 32 words: ONE array, 256 MB at 1 M trees (round 4).  Round 6: evogp_hip_sr_fitness -- the call WITHOUT a mask, the reference's
 * own operator (torch_wrapper.cu:235-284) -- is given the mask the engine observes on the device: the first call on a population
 * shape (pop_size, gp_len) looks at its forest (one pass over the nodes, waited for once per shape; not inside a stream capture,
 * where the call takes the law above), every later call reads what the last completed call on that shape observed.  The observation
 * decides which kernels run and how many arrays are held, never a result: a tree the chosen compiler cannot take is evaluated by the
 * register kernels (the value up to the order of the sum over the rows), and the call's own observation corrects the next call.
 * EVOGP_TC_LEARN=0 switches the observations off (unmasked calls then always hold three arrays).
 *   evogp_hip_set_program_buffer_limit  caps the buffer (default 16 GiB): a call that would need more runs on the register
 *                                       interpreters instead (same results, 3-6x slower); 0 disables the compiled path.
 *   evogp_hip_program_buffer_bytes      bytes currently held on the current device (the eager buffer + the graphs').
 *   evogp_hip_release_workspaces        waits for the current device and frees the buffer (and the rings below); the next
 *                                       fitness call allocates again.
 * Round 4: a call whose trees cannot need the general program compiler (single output, gp_len <= 64, a dataset that fits LDS, and
 * a function mask that says so: evogp_hip_sr_fitness_hinted) runs as ONE kernel whose waves compile the batch of eight trees they
 * are about to interpret into a RING of records of their own -- no population-sized buffer at all.  A ring is
 *     bytes = compute units * 16 waves * 2 arrays * 16 records * 256     (32 MiB on a 256-CU device, whatever the population)
 * and lives in L2; every stream that makes such calls gets one (plus one spare per device, which the first call on a CAPTURING
 * stream takes: nothing is allocated inside a capture), they are never freed or moved before evogp_hip_release_workspaces, so a
 * HIP graph that holds such a call stays valid while later calls grow or shrink the population.
 *   evogp_hip_record_ring_bytes         bytes of rings currently held on the current device. */
int evogp_hip_set_program_buffer_limit(unsigned long long bytes);
/* Where that memory comes from (round 5): by default hipMalloc / hipFree; a caller with an allocator of its own hands in a pair of functions
 * (alloc returns NULL on failure) and the buffers become visible in its statistics -- the libtorch binding installs torch's caching
 * allocator when it is loaded, so torch.cuda.memory_allocated() counts them.  The engine synchronises the device before it first touches a
 * block from a caller's pool.  Only while the engine holds no memory (evogp_hip_release_workspaces first), else EVOGP_E_BADARG; NULL, NULL
 * restores hipMalloc / hipFree. */
typedef void *(*evogp_alloc_fn)(size_t bytes);
typedef void (*evogp_free_fn)(void *ptr);
int evogp_hip_set_allocator(evogp_alloc_fn alloc, evogp_free_fn free_fn);
unsigned long long evogp_hip_program_buffer_bytes(void);
unsigned long long evogp_hip_record_ring_bytes(void);
int evogp_hip_release_workspaces(void);

/* Timers, per-stage profiling, compiler / twin selection for A/B runs, handler histograms and the test entries of the native mutation
 * kernels are not part of this boundary: include/evogp_hip_debug.h. */

/* Human-readable text for a return code of any function above. */
const char *evogp_hip_error_string(int code);

/* Division in the threaded-code SR-fitness path (no counterpart in the reference's ABI: the reference fixes its division
 * at BUILD time -- setup.py:55 compiles the kernels with -use_fast_math, i.e. CUDA's approximate 2-ulp division).
 *   EVOGP_DIV_SHORT (default)  the IEEE sequence with all of its range and special-case handling (v_div_scale,
 *                   v_div_fmas, v_div_fixup) but ONE residual correction instead of a refined reciprocal plus two: 9
 *                   operations per quotient instead of 13.  Faithfully rounded; it is the correctly rounded quotient
 *                   except for about 1 operand pair in 4e9 (1 of 2^32 random mantissa pairs, scripts/ubench/
 *                   div_faithful.hip), where it is the neighbouring float.  Fitness vectors of 200 k trees x 1024 rows
 *                   were bit-identical to the IEEE mode (scripts/div_modes.py).  A block of 64 lanes x K rows whose operands
 *                   all lie in [2^-46, 2^46] -- where the range scaling does nothing -- runs the same four operations
 *                   without it (same quotients, bit for bit; docs/DESIGN_history_r01_r03.md section 3.1d).
 *                   Round 5: under SHORT and FAST a launch whose whole dataset lies in [2^-46, 2^46] (NaN allowed) keeps the correctly
 *                   rounded reciprocals of the variables' columns in LDS, and a division BY A VARIABLE reads its reciprocal instead of
 *                   computing it with v_rcp_f32 (1 ulp); the residual correction against the divisor stays, so the quotient is
 *                   faithfully rounded as before but need not be the same float in the rare pairs where SHORT and IEEE differ
 *                   (EVOGP_TC_RECIP=0 switches it off).
 *   EVOGP_DIV_IEEE  every quotient is the correctly rounded IEEE-754 quotient, as the CPU oracle computes it (+45 % time).
 *   EVOGP_DIV_FAST  as SHORT, but a block with an operand outside [2^-46, 2^46] takes rows without range scaling:
 *                   |b| > 2^126 gives 0 and |a/b| >= 2^128 gives NaN instead of inf (-2 % time against SHORT).
 * A NaN fitness is always the canonical quiet NaN 0x7FC00000 on this path.
 * Affects only tree_SR_fitness with one output on the + - * / function set (the threaded-code path); every other
 * kernel (evaluate, batch_evaluate, the register interpreters) divides with the IEEE sequence.
 * Environment: EVOGP_SR_DIV=ieee|short|fast selects the mode of a process that never calls the setter. */
#define EVOGP_OK 0
#define EVOGP_DIV_IEEE 0
#define EVOGP_DIV_FAST 1
#define EVOGP_DIV_SHORT 2
int evogp_hip_set_sr_division(int mode);
int evogp_hip_get_sr_division(void);

/* ABI version of this header (9): bumped when a signature changes or an entry point is added (5: the debug hooks moved to evogp_hip_debug.h;
 * 6: evogp_hip_sr_gradient, evogp_hip_sr_const_step; 7: evogp_hip_sr_case_errors, evogp_hip_lexicase_workspace_bytes,
 * evogp_hip_lexicase_select; 8: evogp_hip_pareto_rank_workspace_bytes, evogp_hip_pareto_rank, evogp_hip_nsga2_select;
 * 9: evogp_hip_sr_subtree_errors, evogp_hip_prune_rows; evogp_hip_sr_normal_eq and evogp_hip_sr_lm_step, then evogp_hip_tree_hash,
 * evogp_hip_tree_classes_workspace_bytes and evogp_hip_tree_classes, then evogp_hip_sr_linear_scaling and evogp_hip_wrap_linear, then evogp_hip_tree_intervals,
 * then evogp_hip_tree_derivative_intervals, then evogp_hip_sr_gene_fitness, then evogp_hip_tree_dimensions, then evogp_hip_sr_semantic_hash, evogp_hip_sr_semantic_classes and their
 * _workspace_bytes, then evogp_hip_tree_structure, then evogp_hip_sr_weighted_loss, then evogp_hip_sr_weighted_gradient and evogp_hip_sr_weighted_normal_eq, then evogp_hip_sr_weighted_scaling, then evogp_hip_sr_input_gradient and evogp_hip_sr_derivative_loss, then evogp_hip_sr_desired and evogp_hip_sr_backprop_match, then evogp_hip_sr_desired_mid and evogp_hip_sr_agx_match, then evogp_hip_sr_subtree_signatures and evogp_hip_subtree_library_select with its _workspace_bytes, then evogp_hip_sr_subtree_introns and evogp_hip_remove_introns, then evogp_hip_sr_pair_moments and its _workspace_bytes were added to 9 without a bump: purely additive, no existing signature or behaviour changed). */
int evogp_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* EVOGP_HIP_H */
