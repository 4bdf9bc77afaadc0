// The candle-tile mapping of the entry-gate kernels (impulse_kernel and
// bb_stable_kernel, bq_impulse.hip; grid_ladder_kernel, bq_ladder.hip): one
// workgroup per (row, CT_TILE-candle tile), a thread per candle (CT_CPT
// candles, strided by the block). The kernels stay written out in their files;
// this header holds the one geometry and the host side of a launch. Internal
// to the library.
#pragma once
#include <stdint.h>

#include "bq_device.h"
#include "binquant_amd.h"

namespace bq {

// ---- geometry ----------------------------------------------------------------
constexpr int CT_TILE = BQ_IMPULSE_TILE;   // candles per workgroup tile
constexpr int CT_NT = 256;                 // threads
constexpr int CT_CPT = CT_TILE / CT_NT;    // candles per thread
static_assert(BQ_IMPULSE_TILE == BQ_GRID_LADDER_TILE, "one tile for the three kernels");
static_assert(CT_TILE % CT_NT == 0 && CT_NT % WAVE == 0, "whole waves, whole candles per thread");

// ---- host side of a launch -----------------------------------------------------
// tiles per row; false where t0 + 2 * CT_TILE could pass an int or S * tiles
// workgroups overflow a grid
inline bool candle_tiles(int64_t S, int64_t T, int64_t& tiles) {
  if (T > 0x7fffffff - 2 * CT_TILE) return false;
  tiles = (T + CT_TILE - 1) / CT_TILE;
  return tiles * S <= 0x7fffffff;
}

// val[k] = values[k] (values NULL: none): replay_values (bq_replay.h) without the mask
template <int NV>
inline void tile_values(double* (&val)[NV], double* const* values) {
  for (int k = 0; k < NV; ++k) val[k] = values ? values[k] : nullptr;
}

}  // namespace bq
