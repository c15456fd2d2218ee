"""Which launches one transformer block makes at one shape: the constructor's switches (`StFlags`), the form they
select (`StForm`) and the one function that selects it (`st_form`).  Host arithmetic on integers and flags only:
nothing here touches a tensor or a device, `UNet._st` runs what is picked here."""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import ops

# The row-panel kernels that start at the cross-attention (ldm_st_xtail, ldm_st_block) take one shape family; each
# limit restates an LDM_CHECK_ARG of csrc/ffn.hip:
PANEL_WIDTH = 384       # attention width heads * Sp: "K0 == 384" of ldm_st_tail, ldm_st_xtail and ldm_st_block
PANEL_T = 128           # query rows per sample: "T % 128 == 0" of ldm_st_xtail and ldm_st_block
PANEL_MAX_KEYS = 80     # context tokens: "Tk <= 80" of ldm_st_xtail and ldm_st_block
PANEL_MIN_LDV = 80      # row length of the context's V^T: "ldv >= 80" of ldm_st_xtail and ldm_st_block
FOLD_T = 32             # the LayerNorm fold runs on the persistent kernel: whole 32-row groups per sample
OUT2_T = 4              # ldm_gemm's transposed second output stores four rows of a sample at a time


@dataclass(frozen=True)
class StFlags:
  """The launch-form switches and thresholds of `UNet(...)`, gated by the storage type once (`StFlags.of`)."""
  # the blocks' LayerNorms come out of the producing GEMM's epilogue where its tile holds whole rows (C = 320).
  # Measured on MI355X at R=32: 11.02 vs 10.95 ms per step -- the whole-row 128x320 tile (one workgroup per CU) plus
  # the extra epilogue pass cost slightly more than the 15 LayerNorm launches they replace.  Opt-in (parity-tested).
  fuse_ln: bool
  # the self-attention q|k and v projections as one GEMM launch with a transposed second output (ldm_gemm out2)
  fuse_qkv: bool
  # bf16: q|k and v as two persistent-kernel launches (v stored transposed); False: A/B
  split_qkv: bool
  # bf16: each LayerNorm of the block (unet.py:309-313) is folded into the projection it feeds -- LN(x) W^T =
  # rstd (x (gamma (.) W)^T - mean colsum) + W beta -- and the persistent GEMM derives the row statistics from the A
  # tiles it stages anyway: 48 LayerNorm launches and their normalised copies of the residual stream disappear.  Only
  # where the launch has enough rows to fill the chip on the persistent kernel (fold_min_rows); float32 keeps the
  # separate LayerNorm (parity mode), and so does fuse_ln
  fold_ln: bool
  matrix_softmax: bool    # ldm_attention_ms on the 40-wide heads (with the fold; A/B: False)
  fused_ffn: bool         # ldm_ffn_geglu on the C = 320 blocks (needs the fold; A/B: False)
  fused_tail: bool        # ... with the o-projection before and proj_out after it (ldm_st_tail)
  fused_xattn: bool       # ... and the cross-attention in front of the tail (ldm_st_xtail)
  fused_block: bool       # ... and o1-projection + query projection in front (ldm_st_block)
  merge_qkv: bool         # LayerNorm-folded q | k | V^T as one launch (A/B: False = two)
  # (a row limit from the first form of the launch, whose workgroups lay on one side of n_split and could not be
  # balanced at M = 32768: 6 + 3 n-tiles on 2 workgroups per panel; ranges may straddle n_split now)
  merge_qkv_max_rows: int
  merge_ffproj: bool      # FF-out + proj_out as one folded product on the per-layer path (bf16; A/B: False)
  fold_min_rows: int
  ffn_min_rows: int       # the row-panel launches from 192 panels of 128 rows on (3/4 of the CUs busy)
  block_min_rows: int     # ... ldm_st_block alone from 192 panels of 64 rows on

  @classmethod
  def of(cls, dtype, *, fuse_layernorm, fuse_qkv, split_qkv, fold_layernorm, matrix_softmax, fused_ffn, fused_tail,
         fused_xattn, fused_block, merge_qkv, merge_qkv_max_rows, merge_ffproj, fold_min_rows, ffn_min_rows,
         block_min_rows):
    bf16, fuse_ln = dtype == torch.bfloat16, bool(fuse_layernorm)
    return cls(fuse_ln=fuse_ln, fuse_qkv=bool(fuse_qkv), split_qkv=bf16 and bool(split_qkv),
               fold_ln=bf16 and bool(fold_layernorm) and not fuse_ln, matrix_softmax=bool(matrix_softmax),
               fused_ffn=bool(fused_ffn), fused_tail=bool(fused_tail), fused_xattn=bool(fused_xattn),
               fused_block=bool(fused_block), merge_qkv=bool(merge_qkv), merge_qkv_max_rows=int(merge_qkv_max_rows),
               merge_ffproj=bool(merge_ffproj), fold_min_rows=int(fold_min_rows), ffn_min_rows=int(ffn_min_rows),
               block_min_rows=int(block_min_rows))


class StForm(NamedTuple):
  """What one transformer block launches at one shape."""
  norm: str             # the three LayerNorms: "fold" into their consumers | "epilogue" of their producers | "separate"
  qkv: str              # self-attention projections: "qkv_fold" | "qk_v_fold" | "qk_vt" | "qkv_out2" | "qk_bmm"
  ms: bool              # matrix-side softmax (ldm_attention_ms) in both attentions
  rest: str             # self-attention output -> block output: "block" | "xtail" | "tail" | "ffn" | "ffproj" | "layers"
  leave_prefix: bool    # a CFG pair copies its rows in front of `rest` (every form but "block", which reads half rows)


def st_form(flags, dtype, c, heads, s, sp, has_fold, has_ffn_aux, has_ffp, ms_capable, rows_in, pair, T, Tk, ldv,
            capture):
  """The form of a block of width `c` (`heads` heads of `s` padded to `sp`) whose input has `rows_in` samples of `T`
  rows -- half of the output's for a CFG `pair` -- against `Tk` context tokens in V^T rows of `ldv`.  `has_fold`,
  `has_ffn_aux`, `has_ffp`, `ms_capable`: what `_ST` built (st.fold, st.ffn_aux, st.ffp, st.ms); `capture`: the
  block's cross-attention maps are being accumulated."""
  f, hs = flags, heads * sp
  rows = rows_in * T
  rows_out = 2 * rows if pair else rows
  fold = has_fold and rows >= f.fold_min_rows and T % FOLD_T == 0
  norm = "fold" if fold else "epilogue" if f.fuse_ln and ops.linear_ln_supported(c, dtype) else "separate"
  ldt = (T + 7) // 8 * 8                # the self-attention's V^T rows, as UNet._st hands them out
  if fold and f.merge_qkv and rows <= f.merge_qkv_max_rows and hs % 128 == 0:
    qkv = "qkv_fold"
  elif fold:
    qkv = "qk_v_fold"
  elif f.split_qkv and ops.linear_t_shape_supported(dtype, c, hs, T, ldt, hs * ldt):
    qkv = "qk_vt"
  elif f.fuse_qkv and T % OUT2_T == 0:
    qkv = "qkv_out2"
  else:
    qkv = "qk_bmm"
  ms = fold and ms_capable
  # the row-panel launches: ldm_ffn_geglu's weights and enough rows; ldm_st_tail adds the width; the two that hold
  # the cross-attention add its shape family -- and ldm_st_block has a 64-row panel form for launches below 192
  # panels of 128 rows: it pays from 192 panels of 64 rows on, where the others (128-row panels only) do not
  ffn = fold and has_ffn_aux and f.fused_ffn
  panel = ffn and rows_out >= f.ffn_min_rows
  xattn = (ffn and f.fused_tail and f.fused_xattn and ms and hs == PANEL_WIDTH and T % PANEL_T == 0
           and Tk <= PANEL_MAX_KEYS and ldv >= PANEL_MIN_LDV)
  if (f.fused_block and xattn and rows_out >= min(f.ffn_min_rows, f.block_min_rows)
      and not capture):               # (ldm_st_block never materialises the queries the heat maps read)
    rest = "block"
  elif panel and xattn:
    rest = "xtail"
  elif panel and f.fused_tail and hs == PANEL_WIDTH:
    rest = "tail"
  elif panel:
    rest = "ffn"
  elif has_ffp and f.merge_ffproj:
    rest = "ffproj"
  else:
    rest = "layers"
  return StForm(norm, qkv, bool(ms), rest, bool(pair and rest != "block"))
