"""ldm_tf2_amd.st_form.st_form against the predicates `UNet._st` had inline (tests/st_form_ref.py, frozen).

Two grids, because the full cross product would run for minutes:
  A. all 2^11 flag combinations x both storage types x the threshold settings x pair x capture, on CORE: a dozen
     shapes that between them sit on both sides of every limit;
  B. every shape of SHAPES x both storage types x the threshold settings x pair x capture, on FLAG_SETS: the
     defaults, each flag flipped alone, all off, all on.
Threshold settings: the constructor's defaults, every minimum at 1, and merge_qkv_max_rows one below and exactly at the
case's rows.  The module fails if any value of StForm's fields never comes out, and prints the histogram.
"""
import collections
import itertools

import torch

import st_form_ref as REF
from ldm_tf2_amd import layout as L
from ldm_tf2_amd.st_form import StFlags, st_form

F32, BF16 = torch.float32, torch.bfloat16
FLAGS = ("fuse_layernorm", "fuse_qkv", "split_qkv", "fold_layernorm", "matrix_softmax", "fused_ffn", "fused_tail",
         "fused_xattn", "fused_block", "merge_qkv", "merge_ffproj")
# (C, heads): the three widths of the full model, the tiny test model's, and two that the models do not have: 5 heads
# of 64 (heads * Sp = 320, no multiple of 128) and 8 heads of 48 (the row-panel width 384 without the 40-wide heads)
WIDTHS = ((320, 8), (640, 8), (1280, 8), (64, 8), (320, 5), (384, 8))
# 36 and 100: T % 32 and T % 128 fail, 100 is no multiple of 8 either; 9 (a 3x3 map): T % 4 fails
TS = (4, 9, 16, 36, 64, 100, 256, 1024, 4096)
CONTEXTS = ((77, 80), (80, 80), (81, 88), (8, 8))   # (Tk, ldv) on both sides of 80 keys and of V^T rows of 80
ROW_LIMITS = (2048, 12288, 24576)                   # fold_min_rows, block_min_rows, ffn_min_rows


def _rows(T):
  """Sample counts R with R * T on both sides of every row limit (and 2 R * T, for a pair)."""
  rs = {1, 4}
  for lim in ROW_LIMITS:
    for m in (lim, lim // 2):
      r = -(-m // T)
      rs |= {r, r - 1}
  return sorted(r for r in rs if r >= 1)


SHAPES = [(c, hd, R, T, Tk, ldv) for (c, hd), T in itertools.product(WIDTHS, TS) for R in _rows(T)
          for Tk, ldv in (CONTEXTS if (c, hd, T % 128) == (320, 8, 0) else CONTEXTS[:1])]
CORE = [(320, 8, 4, 256, 77, 80), (320, 8, 8, 256, 80, 80), (320, 8, 12, 1024, 77, 80), (320, 8, 24, 1024, 81, 88),
        (320, 8, 6, 4096, 77, 8), (320, 8, 48, 256, 77, 80), (320, 8, 123, 100, 77, 80), (640, 8, 32, 64, 77, 80),
        (640, 8, 31, 64, 77, 80), (1280, 8, 4, 16, 77, 80), (1280, 8, 64, 36, 77, 80), (64, 8, 4, 36, 8, 8),
        (64, 8, 4, 9, 77, 80), (64, 8, 8, 256, 77, 80), (320, 5, 96, 256, 77, 80), (384, 8, 96, 256, 77, 80)]
FLAG_SETS = ([{}, {f: False for f in FLAGS}, {f: True for f in FLAGS}] +
             [{f: not REF.DEFAULTS[f]} for f in FLAGS])


def _thresholds(rows):
  yield {}
  yield dict(fold_min_rows=1, ffn_min_rows=1, block_min_rows=1)
  yield dict(merge_qkv_max_rows=rows - 1)
  yield dict(fold_min_rows=1, ffn_min_rows=1, block_min_rows=1, merge_qkv_max_rows=rows)


def _both(kw, dtype, shape, pair, capture):
  """(st_form's answer, the frozen predicates' answer) for one constructor setting at one shape."""
  c, heads, R, T, Tk, ldv = shape
  flags = StFlags.of(dtype, **kw)
  s = c // heads
  sp = L.padded_head(s)
  # what _ST.__init__ builds from these flags (unchanged by the picker): st.fold, st.ffn_aux, st.ffp, st.ms
  has_fold = flags.fold_ln
  got = st_form(flags, dtype, c, heads, s, sp, has_fold, has_fold and c == 320, has_fold,
                bool(has_fold and flags.matrix_softmax and s == L.MS_DIM and sp == 48), R, pair, T, Tk, ldv, capture)
  self = REF.unet_init(dtype, **kw)
  st = REF.st_init(c, heads, fold_ln=self._fold_ln, matrix_softmax=self._matrix_softmax)
  return got, REF.st_form_parent(self, st, dtype, R, T, pair, Tk, ldv, capture)


def _grid(flag_sets, shapes):
  for shape in shapes:
    for thr in _thresholds(shape[2] * shape[3]):
      for fl, dtype, pair, capture in itertools.product(flag_sets, (F32, BF16), (False, True), (False, True)):
        yield dict(REF.DEFAULTS, **fl, **thr), dtype, shape, pair, capture


def test_st_form_evaluates_the_inline_predicates():
  all_flags = [dict(zip(FLAGS, v)) for v in itertools.product((False, True), repeat=len(FLAGS))]
  assert len(all_flags) == 2 ** 11
  hist, n, bad = collections.Counter(), 0, []
  for case in itertools.chain(_grid(all_flags, CORE), _grid(FLAG_SETS, SHAPES)):
    got, want = _both(*case)
    n += 1
    hist[got] += 1
    if got != want and len(bad) < 5:
      bad.append((case, got, want))
  print(f"{n} cases, {len(hist)} distinct forms")
  for form, k in sorted(hist.items(), key=lambda kv: -kv[1]):
    print(f"  {k:8d}  {form}")
  assert not bad, bad
  for field, values in (("norm", ("fold", "epilogue", "separate")),
                        ("qkv", ("qkv_fold", "qk_v_fold", "qk_vt", "qkv_out2", "qk_bmm")), ("ms", (False, True)),
                        ("rest", ("block", "xtail", "tail", "ffn", "ffproj", "layers")), ("leave_prefix", (False, True))):
    seen = {getattr(f, field) for f in hist}
    assert seen == set(values), f"{field}: the grid produced {sorted(seen, key=str)} of {values}"


def test_each_limit_is_straddled():
  """Every limit of the picker has shapes of the grid on both sides of it."""
  T = {s[3] for s in SHAPES + CORE}
  for m in (4, 32, 128):
    assert any(t % m == 0 for t in T) and any(t % m for t in T), m
  hs = {h * L.padded_head(c // h) for c, h, *_ in SHAPES + CORE}
  assert 384 in hs and len(hs) > 1 and any(v % 128 for v in hs) and any(v % 128 == 0 for v in hs)
  for rows_of in (lambda s: s[2] * s[3], lambda s: 2 * s[2] * s[3]):
    for lim in ROW_LIMITS:
      for t in (64, 256, 1024):         # (with the limit itself, which these T divide, and the last R below it)
        r = [rows_of(s) for s in SHAPES if s[3] == t and s[:2] == (320, 8)]
        assert lim in r, (lim, t)
        if rows_of((320, 8, 1, t)) < lim:         # (a pair of single samples of T = 1024 has 2048 rows: none below)
          assert any(lim - 2 * t <= v < lim for v in r), (lim, t)
        else:
          assert t == 1024 and lim == 2048
  ctx = {s[4:] for s in SHAPES if s[:2] == (320, 8) and s[3] % 128 == 0}
  assert any(k <= 80 for k, _ in ctx) and any(k > 80 for k, _ in ctx)
  assert any(v >= 80 for _, v in ctx) and any(v < 80 for _, v in ctx)


def test_shape_form_of_linear_t_supported_agrees_with_the_tensor_form():
  from ldm_tf2_amd import ops
  for dt, K, N, R, T in itertools.product((F32, BF16), (64, 96, 320), (256, 320, 384, 200), (1, 3), (32, 36, 64, 100)):
    tp = (T + 7) // 8 * 8
    x, w, vt = (torch.empty(s, dtype=dt, device="meta") for s in ((R, T, K), (N, K), (R, N, tp)))
    want = REF.linear_t_supported(x, w, vt)
    assert ops.linear_t_supported(x, w, vt) == want
    assert ops.linear_t_shape_supported(dt, K, N, T, tp, N * tp) == want
    # a V^T whose rows are no multiple of 8 elements apart
    odd = torch.empty((R, N, tp + 4), dtype=dt, device="meta")
    assert ops.linear_t_supported(x, w, odd) == REF.linear_t_supported(x, w, odd)
