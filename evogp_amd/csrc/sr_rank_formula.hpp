// sr_rank_formula.hpp — THE score of one segment from its exact integer words (sr_rank.hip's epilogue and nothing else).
// include/evogp_hip.h has the definitions: S1 = sum R2 q, S2 = sum R2^2 over the segment's n rows (R2 the doubled mid-rank of a
// prediction), Q = sum q, Q2 = sum q^2.  Every product below is exact in int64 (S1, S2 < 2^42, n <= 2^13, Q <= 2^27, Q2 <= 2^41); the
// three float64 operations of a score are explicit correctly rounded calls, so no compiler flag changes them.
#pragma once
#include <hip/hip_runtime.h>

namespace evogp {

constexpr int kRankSpearman = 0, kRankAuc = 1;

// false: the segment's score is undefined (a tree or labels constant on it, n == 1; for AUC one class only)
__device__ inline bool rank_segment_score(int metric, long long n, long long S1, long long S2, long long Q, long long Q2, double *score) {
    if (metric == kRankAuc) {
        if (Q == 0 || Q == n) return false;
        *score = __ddiv_rn((double)(S1 - Q * (Q + 1)), (double)(2 * Q * (n - Q)));
        return true;
    }
    const long long nn = n * (n + 1);
    const long long A = n * S1 - nn * Q;
    const long long Bp = n * S2 - nn * nn;
    const long long Bl = n * Q2 - Q * Q;
    if (Bp == 0 || Bl == 0) return false;
    *score = __ddiv_rn((double)A, __dsqrt_rn(__dmul_rn((double)Bp, (double)Bl)));
    return true;
}

}  // namespace evogp
