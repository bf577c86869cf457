// dedup.hpp — stages 1-3 of the class passes (dedup.hip defines them; sr_semantic.hip runs them in front of its own stage 4).
#pragma once
#include <hip/hip_runtime.h>

namespace evogp {

// (hash_in[t], t) pairs, their stable sort and the run starts, out of a caller's workspace of evogp_hip_tree_classes_workspace_bytes(pop)
// bytes: members[s] is the tree at sorted position s (tree indices ascend within a run of equal hash words), seg[s] the position at
// which the run of s starts.  Both point into the workspace.  Three launches and rocPRIM's on `stream`, nothing synchronises with the host.
hipError_t dedup_sorted_runs(const unsigned long long *hash_in, unsigned pop, void *workspace, const unsigned **members, const unsigned **seg,
                             hipStream_t stream);

}  // namespace evogp
