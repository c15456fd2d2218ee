// The tile table of ldm_gemm: one row per tile number, everything the HOST needs to know about a tile.  The plan
// (gemm.hip choose / final_plan), ldm_gemm's tile checks, the launch switch (gemm_launch.h) and ldm_gemm_tile_info
// (hence ops.py and the tests) read these rows.  Adding a tile: DESIGN.md section 4, "The GEMM tile table".
#pragma once
#include "ldm_hip.h"

namespace ldm_gemm_detail {

struct TileRow {
  int bm, bn, resident;             // tile rows, columns; workgroups per CU (LDS-limited)
  int wm, wn, mf, st, ns;           // gemm_kernel: WM x WN waves, MFMA path, ping-pong, ring depth (0 = the kernel's rule)
  unsigned flags;                   // LDM_TILE_* (ldm_hip.h), as ldm_gemm_tile_info reports them
  double step_us, overhead_steps;   // cost model: us per round per K-tile (bf16); launch + prologue + epilogue in K-tiles
  int halo_twin, prefer_over;       // measured policies: the halo-staged tile that replaces this one on deep stride-1
};                                  // convolutions; the tile whose under-filled launches this one beats (0 = none)
enum : unsigned {                   // the flags, short enough for a row
  tPers = LDM_TILE_PERSISTENT, tHalo = LDM_TILE_HALO, tBf16 = LDM_TILE_BF16_ONLY, tGeglu = LDM_TILE_GEGLU,
  tGegluV = LDM_TILE_GEGLU | LDM_TILE_GEGLU_VEC, tPh32 = LDM_TILE_PHASE_F32, tPh16 = LDM_TILE_PHASE_BF16,
  tForced = LDM_TILE_FORCED, tForcedBf16 = LDM_TILE_FORCED_BF16, tExper = LDM_TILE_FORCED | LDM_TILE_EXPERIMENTAL,
  tA2 = LDM_TILE_A2, tWholeN = LDM_TILE_WHOLE_N };
constexpr int kNumTiles = 20;
constexpr TileRow kTiles[kNumTiles] = {
    // bm   bn res  wm wn mf st ns  flags                                            step_us ovh twin prefer_over
    {},                                                                                               // 0 = auto
    {256, 128, 1,   4, 2, 0, 0, 0,  tGeglu | tPh32 | tForcedBf16 | tA2,                 0.82, 8},      // bf16: 11 is ~20 % faster
    {128, 128, 2,   2, 2, 0, 0, 0,  tGeglu | tPh32 | tPh16 | tA2,                       0.82, 8, 0, 1},
    {128,  64, 3,   2, 2, 0, 0, 0,  tA2,                                                0.75, 7},
    { 64,  64, 5,   2, 2, 0, 0, 0,  tA2,                                                0.87, 6},
    {256, 128, 1,   2, 2, 0, 0, 0,  tGeglu | tExper | tA2,                              0.82, 8},      // 4 waves x (128x64)
    {128, 160, 2,   4, 1, 0, 0, 0,  tForcedBf16 | tA2 | tWholeN,                        1.12, 8},      // 6-8: waves of 32x160;
    {256, 160, 1,   8, 1, 0, 0, 0,  tForcedBf16 | tA2 | tWholeN,                        1.18, 8},      // bf16: 10 / 9 are faster
    {128, 320, 1,   4, 2, 0, 0, 0,  tA2 | tWholeN,                                      1.15, 8},
    // 9-12: bf16 v_mfma_f32_16x16x32 path, wave tiles 64x80 / 64x64; the 8-wave ones (9, 11) ping-pong their halves
    {256, 160, 1,   4, 2, 1, 1, 0,  tBf16 | tPh16 | tA2 | tWholeN,                      1.03, 8, 15},
    {128, 160, 2,   2, 2, 1, 0, 0,  tBf16 | tA2 | tWholeN,                              1.09, 8},
    {256, 128, 1,   4, 2, 1, 1, 0,  tBf16 | tGegluV | tPh16 | tA2,                      0.97, 8},      // (16 twins it: plans only)
    {128, 128, 2,   2, 2, 1, 0, 0,  tBf16 | tGegluV | tForced | tA2,                    0.80, 8},      // no better than tile 2
    // 13, 14: persistent ping-pong kernel (gemm3_kernel.h, 512 threads): a workgroup walks n-tiles of its 256-row panel
    {256, 160, 1,   4, 2, 1, 1, 0,  tPers | tBf16 | tForced | tWholeN,                  1.03, 4},
    {256, 128, 1,   4, 2, 1, 1, 0,  tPers | tBf16 | tGeglu | tForced,                   0.97, 4},
    // 15, 16: tiles 9 / 11 with the halo-staged A operand: stride-1 convolutions whose M-tile is whole lines of one image
    {256, 160, 1,   4, 2, 1, 1, 0,  tHalo | tBf16 | tForced | tWholeN,                  1.0,  9},
    {256, 128, 1,   4, 2, 1, 1, 0,  tHalo | tBf16 | tForced,                            0.94, 9},
    // 17-19: tiles 4 / 3 / 2 with a 4- / 3- / 3-stage LDS ring: launches of 1-3 workgroups per CU
    { 64,  64, 2,   2, 2, 0, 0, 4,  tForced | tA2,                                      0.87, 6},
    {128,  64, 2,   2, 2, 0, 0, 3,  tForced | tA2,                                      0.75, 7},
    {128, 128, 1,   2, 2, 0, 0, 3,  tGeglu | tForced | tA2,                             0.82, 8},
};
constexpr int kFallbackTile = 2;                        // the plan when no tile qualifies (the checks then say why)
constexpr int kLnTile = 8;                              // ln_out: the tile whose bn (320) holds a whole N = 320 row
constexpr int kLnFoldTile = 14, kLnFoldWideTile = 13;   // ln_cs: persistent, 160-column n-tiles where only those divide N
constexpr bool has(int c, unsigned flag) { return (kTiles[c].flags & flag) != 0; }
constexpr bool phase_tile_ok(int c, int esize) { return has(c, esize == 2 ? LDM_TILE_PHASE_BF16 : LDM_TILE_PHASE_F32); }
// whether gemm_kernel<T, ..., MODE> of tile c exists (MODE 3 = halo-staged, 4 = phase form): asked by ldm_gemm's checks and the launch switch
constexpr bool tile_has_kernel(int c, int esize, int mode) {
  return !has(c, tPers) && (esize == 2 || !has(c, tBf16)) && (mode == 3) == has(c, tHalo) && (mode != 4 || phase_tile_ok(c, esize));
}

}  // namespace ldm_gemm_detail
