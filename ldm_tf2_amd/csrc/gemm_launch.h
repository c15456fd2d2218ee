// Definition of launch_cfg<T, MODE> (one switch over the tile configurations); each
// gemm_inst_*.hip includes this and explicitly instantiates one (T, MODE) pair.
#pragma once
#include "gemm_kernel.h"
#include "gemm_tiles.h"

namespace ldm_gemm_detail {

// One launch case: the kernel's template arguments come from the tile's row, and so does whether the kernel exists for
// (T, MODE) at all (tile_has_kernel, which ldm_gemm has checked before it launches).
template <typename T, int MODE, int TILE>
void launch_tile(const GemmArgs& a, dim3 grid, hipStream_t s) {
  constexpr TileRow r = kTiles[TILE];
  if constexpr (tile_has_kernel(TILE, sizeof(T), MODE))
    hipLaunchKernelGGL((gemm_kernel<T, r.bm, r.bn, r.wm, r.wn, MODE, r.mf, r.st, r.ns>), grid, dim3(r.wm * r.wn * 64), 0, s, a);
}

template <typename T, int MODE>
void launch_cfg(int cfg, const GemmArgs& a, dim3 grid, hipStream_t s) {
  switch (cfg) {
    case 1: return launch_tile<T, MODE, 1>(a, grid, s);
    case 2: return launch_tile<T, MODE, 2>(a, grid, s);
    case 3: return launch_tile<T, MODE, 3>(a, grid, s);
    case 4: return launch_tile<T, MODE, 4>(a, grid, s);
    case 5: return launch_tile<T, MODE, 5>(a, grid, s);
    case 6: return launch_tile<T, MODE, 6>(a, grid, s);
    case 7: return launch_tile<T, MODE, 7>(a, grid, s);
    case 8: return launch_tile<T, MODE, 8>(a, grid, s);
    case 9: return launch_tile<T, MODE, 9>(a, grid, s);
    case 10: return launch_tile<T, MODE, 10>(a, grid, s);
    case 11: return launch_tile<T, MODE, 11>(a, grid, s);
    case 12: return launch_tile<T, MODE, 12>(a, grid, s);
    case 15: return launch_tile<T, MODE, 15>(a, grid, s);
    case 16: return launch_tile<T, MODE, 16>(a, grid, s);
    case 17: return launch_tile<T, MODE, 17>(a, grid, s);
    case 18: return launch_tile<T, MODE, 18>(a, grid, s);
    case 19: return launch_tile<T, MODE, 19>(a, grid, s);   // (13, 14: the persistent kernel's own launchers, gemm3_kernel.h)
  }
}

}  // namespace ldm_gemm_detail
