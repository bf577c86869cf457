// sr_pair_order.hpp — THE order in which the D terms of a pair moment are added (sr_pair.hip).  Both kernels of the pass, the
// register interpreter and the scratch-stack one, add through pair_add_tile and nothing else, so a word is a function of its two
// trees, X and y alone: not of the event or slot it stands in, of M, of E, of the other candidates or of the kernel that took it.
//
// The rows are cut into tiles of 64 x kPairK; row k * 64 + lane of a tile is row k of lane `lane`.  W = pair_waves(D) wave slots; slot w
// owns the tiles w, w + W, ...  A word is
//     total = (((0 + word_0) + word_1) + ...) + word_{W-1}                                   the wave slots in order            (pair_add_wave)
//     word_w = ((0 + tile_w) + tile_{w+W}) + ...                                               the tiles of a slot in order       (pair_add_tile)
//     tile   = wave_sum_d(lane)                                                                the 64 lanes by the fixed butterfly
//     lane   = fma(x_{K-1}, y_{K-1}, ... fma(x_1, y_1, fma(x_0, y_0, 0)))                      the K rows of a lane in order
// with a row past D entering as x = y = 0.  The order depends on D alone.  Products and sums are explicit fma / __dadd_rn calls, so no
// compiler flag changes them between two kernels (wave_sum_d holds additions only).
#pragma once
#include "sr_moments.hpp"

namespace evogp {

constexpr int kPairK = 4;                       // rows per lane of a tile
constexpr int kPairWaves = 4;                   // wave slots: the waves of a workgroup of the register kernel
constexpr int kPairTile = kWave * kPairK;       // rows per tile

__host__ __device__ inline int pair_tiles(int D) { return (int)(((long long)D + kPairTile - 1) / kPairTile); }
__host__ __device__ inline int pair_waves(int D) { return pair_tiles(D) < kPairWaves ? pair_tiles(D) : kPairWaves; }

// word + (the sum over this tile of x * y); called by every lane of the wave, the result is exact in the lane that holds `word`
__device__ inline double pair_add_tile(double word, const double (&x)[kPairK], const double (&y)[kPairK]) {
    double lane = 0.0;
#pragma unroll
    for (int k = 0; k < kPairK; ++k) lane = fma(x[k], y[k], lane);
    return __dadd_rn(word, wave_sum_d(lane));
}

__device__ inline double pair_add_wave(double total, double word) { return __dadd_rn(total, word); }

}  // namespace evogp
