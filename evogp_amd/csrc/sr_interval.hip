// sr_interval.hip — interval arithmetic over SR trees (gfx950; no counterpart in the reference): for every node of the live prefix of
// every single-output tree a float32 interval [lo, hi] and a flag byte that bound the float32 value the interpreters compute for that
// subtree on ANY input inside a box lower[v] <= x[v] <= upper[v] (Keijzer 2003, the companion of linear scaling).  The definition --
// every rule, every choice, the claim -- is the numpy restatement tests/interval_ref.py; the device functions of
// sr_interval_rules.hpp (shared with sr_deriv.hip; this file instantiates them with OUT = false) follow it name by name, in the same
// order of float32 operations and comparisons, so that every rule without a library call gives the same bits.
//
// ONE LANE PER TREE.  The walk goes from the last live node to node 0; child 1 of node i is i + 1 (its interval, size and NaN-constant
// mark are still in registers from the previous step), child 2 is i + 1 + size[i + 1] and child 3 follows it: their intervals are read
// back from the lane's own output row, which is the product, not scratch.  The work is O(live nodes) with a dependent chain along
// every path of the tree, so a wave per tree would leave most lanes waiting for children; a forest offers pop independent chains,
// which is the parallelism this layout takes.  The words of node i - 1 are loaded before node i is resolved.  A size word is verified
// (it must be the size of its subtree) before any parent uses it, and the stack discipline of the type words is checked on the way
// (classify_tree's rule), so no child index leaves the live prefix; a row that fails either check is rewritten as MALFORMED.
// The words past the live prefix are zeroed by the workgroup, one row after the other with the lanes along the row.
// No dataset, no atomics, no host synchronisation, no workspace; the result does not depend on the other rows.
#include "sr_interval_rules.hpp"

using namespace evogp;

extern "C" int evogp_hip_tree_intervals(unsigned pop, unsigned gp_len, unsigned var_len, const float *value, const int16_t *type,
                                        const int16_t *size, const float *lower, const float *upper, float *lo, float *hi,
                                        unsigned char *flags, evogp_stream_t stream_) {
    if (pop == 0 || pop > 0x7FFFFFFFu || gp_len == 0 || gp_len > (unsigned)kMaxStack || var_len == 0) return EVOGP_E_BADARG;
    if (!value || !type || !size || !lower || !upper || !lo || !hi || !flags) return EVOGP_E_NULLPTR;
    hipLaunchKernelGGL(tree_intervals_kernel<false>, dim3((pop + (unsigned)kWave - 1u) / (unsigned)kWave), dim3(kWave), 0, (hipStream_t)stream_, value,
                       type, size, lower, upper, pop, gp_len, var_len, lo, hi, flags);
    return (int)hipGetLastError();
}
