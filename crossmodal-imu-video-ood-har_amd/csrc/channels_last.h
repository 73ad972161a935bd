// What conv3d.hip (the convolutions, whose epilogues write BatchNorm tile statistics) and bn_cl.hip (the channels-last
// BatchNorm that combines them) both need.
#pragma once
#include "common.h"

template <typename T, int V> __device__ __forceinline__ void vload(const T* p, float* v) {
  if constexpr (V == 8) Vec8<T>::load(p, v);
  else for (int j = 0; j < V; ++j) v[j] = to_f<T>(p[j]);
}
template <typename T, int V> __device__ __forceinline__ void vstore(T* p, const float* v) {
  if constexpr (V == 8) Vec8<T>::store(p, v);
  else for (int j = 0; j < V; ++j) p[j] = from_f<T>(v[j]);
}

// Blocks of 256 threads for a grid-stride loop over `work` items, at most 8192 (cnn2d.hip's own grid_for caps at
// 2^19 blocks, so the two stay apart).
inline int grid_for(long work) {
  const long b = (work + 255) / 256;
  return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

constexpr int BN_TG = 16;   // tiles per level-1 group: short sequential chains, enough threads (64 measured 35 us/call)
// Layout of the tile-statistics buffer for (ntile, C), in floats: [2][ntile][C] tile (mean, M2) at 0, then
// [2][ngroup][C] group partials, [ntile] tile row counts, [ngroup] group row counts (ngroup = ⌈ntile / BN_TG⌉);
// `floats` in all.  The conv epilogues write the tile partials and counts, bn_tile_group / bn_tile_final the rest.
struct TileStats { int ngroup; long groups, cnt, gcnt, floats; };
__host__ __device__ __forceinline__ TileStats tile_stats_layout(int ntile, int C) {
  const int ng = (ntile + BN_TG - 1) / BN_TG;
  const long cnt = 2L * (ntile + ng) * C;
  return {ng, 2L * ntile * C, cnt, cnt + ntile, cnt + ntile + ng};
}
