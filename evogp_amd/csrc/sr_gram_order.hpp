// sr_gram_order.hpp — THE order in which the D terms of a word of the population Gram matrix are added (sr_gram.hip).
//
// The rows are cut into SEGMENTS of kGramSegment rows.  A word G[i][j] = sum_d v_i[d] * v_j[d] is
//     word    = (((0 + S_0) + S_1) + ...) + S_{segments - 1}                                  the segments in order              (gram_add_segment)
//     S_s     = step(... step(step(0, group_0), group_1) ..., group_{kGramSegment / 4 - 1})   the groups of a segment in order   (gram_step)
//     step    = one v_mfma_f64_16x16x4_f64: acc + v_i[4 g .. 4 g + 3] . v_j[4 g .. 4 g + 3], the four rows of a group inside the instruction
// with a row past D entering as v = 0.  The order depends on D alone: not on n, on the place of the two trees in the index list, on the
// output block or the 16 x 16 tile a word falls in, nor on how the segments are spread over workgroups and launches (a workgroup that
// owns several segments and the kernel that adds the partial blocks of several workgroups both go through gram_add_segment).
// lin[i] = (sum v_i, sum v_i y) are the words of tree i against two virtual vectors, 1 and y, in the same pass.
#pragma once
#include "evogp_defs.hpp"

namespace evogp {

constexpr int kGramGroup = 4;        // rows per matrix instruction (the K of 16 x 16 x 4)
constexpr int kGramSegment = 1024;   // rows per segment: one chain of 256 matrix instructions from a zero accumulator
constexpr int kGramSlab = 4096;      // rows per panel slab (a launch detail, not part of the order): four segments

typedef double gram_acc __attribute__((ext_vector_type(4)));   // the lane's four words of a 16 x 16 tile

__host__ __device__ inline int gram_segments(int D) { return (int)(((long long)D + kGramSegment - 1) / kGramSegment); }

// acc + A . B for one group of four rows.  Operands: the lane holds A[lane % 16][lane / 16] and B[lane / 16][lane % 16], that is row
// 4 g + lane / 16 of vector lane % 16 of either side; acc[r] is the word of vectors (4 r + lane / 16, lane % 16).
__device__ inline gram_acc gram_step(gram_acc acc, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
#else
    return acc;
#endif
}

__device__ inline double gram_add_segment(double word, double segment) { return __dadd_rn(word, segment); }

}  // namespace evogp
