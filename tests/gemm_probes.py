"""Exact probes for ldm_gemm (GEMM / implicit-GEMM 3x3 convolution): builders, an independent integer reference, the
mutation check and the case matrix (a plain module, imported by test_gemm_probes_cpu.py and
test_gemm_accounting_gpu.py).

A tolerance test on Gaussian data cannot see ONE lost K element, ONE border tap read from the neighbouring line or a
bias shifted by one column: with w ~ K^-1/2 such an error is about K^-1/2 of one output, inside any bf16 tolerance.
Here all operands are small integers (exact in bf16), every product and partial sum stays below 2^24 (exact in float32
in ANY summation order: MFMA k order, kt = chunk * 9 + tap, split-K slabs, both reduce kernels), and every stored value
is exactly representable in the output type.  The gate is therefore torch.equal, there is no tolerance.

  probe 1, selection   wt[n, :] is one-hot at column k(n, phase) = (n * stride_n + phase) mod K, stride_n = ceil(K / N),
                       so out[m, n] is exactly ONE element of A: for a convolution the pixel (b, oy s + kh - pad,
                       ox s + kw - pad) at channel ci, or 0 where the tap is padding.  A is a position code (`code`):
                       a non-zero integer in [-127, 127] that differs between an element and its neighbours at +-1
                       pixel / line / image, +-8 channels (one 16-byte chunk), +-32 / 64 channels (one K-tile) and
                       +-1 row.  ceil(K / N) phases select every K column once; a case runs at most MAX_PHASES of
                       them, chosen so that every K-tile (hence every tap) is still selected (`phases`).
  probe 2, census      A in {+-1, +-2} with density 1/2, W in {+-1} with density min(1/4, 360 / K); bias, per-group
                       addend, residual, the second operand a2 are integers in [-8, 8]; alpha in {1, 0.5, 2}.
                       Where chance leaves a K column without a non-zero entry in some M-tile of A or N-tile of W one
                       entry is set (`_revive`), so in every (M-tile, N-tile) of the case's form every K column has a
                       non-zero product in some output: a lost column cannot hide.  (A convolution tap that is
                       padding for every row of an M-tile cannot be alive there and is exempt.)
  reference            the formula of include/ldm_hip.h written out: an explicit gather of the source pixel of every
                       (row, tap) (`conv_src`), then sum_k A[m][k] W[n][k] over integers held in float64 (every value
                       is an integer below 2^24, so float64 is exact) and the epilogue terms.  It is not a call to
                       the oracle; the CPU test compares it with oracle.ldm_oracle once per mode.
  mutation check       `MUTATIONS`: references of subtly wrong kernels.  Each must differ from the right reference in
                       every case it applies to (`mutation_applies` names the exempt cases):
                         drop_column      one K column lost in the last N-tile: applies everywhere
                         double_ktile     a K-tile from the middle of K counted twice: applies everywhere
                         drop_last_ktile  exempt: convolutions without a second operand in which tap (2, 2) is padding
                                          for EVERY output pixel (H = 1 or W = 1 without upsampling; the 2 x 2 image
                                          at stride 2 without lead pad)
                         pair_off_by_one  A K-tile kt meets W K-tile kt + 1; exempt: one K-tile
                         line_end         tap (1, 0) / (1, 2) reads the linear neighbour instead of the zero column
                         prev_image       tap row 0 / 2 reads the neighbouring image instead of the zero line
                         origin           stride-2 origin off by one (no_lead_pad confused)
                         up_odd           odd upsampled coordinates not halved
                                          these four: exempt for plain rows and wherever the wrong gather reads the
                                          very same pixels (no neighbour exists: one line or one pixel of one image
                                          for line_end, B = 1 for prev_image, stride 1 for origin, no upsampling for
                                          up_odd); `mutation_applies` compares the two gathers
                         swap_rows        the rows on both sides of the first M-tile edge (else the first and the
                                          last row); exempt: M = 1
                         bias_column      bias one column on, addend one sample on; exempt: neither is passed
                         residual_stride  exempt: no residual, or a residual whose row stride equals N
                         a2_next_pixel    exempt: no second operand, or M = 1

Non-square and odd-sided images live HERE: tests/test_bench_shapes_gpu.py derives B from OH * OH and runs square
power-of-two images only.

The wide-image limit of the upsampled form: gemm_kernel.h / gemm3_kernel.h pack the tap origin in the UPSAMPLED image
as (iy0 << 16) | (ix0 & 0xffff) and read ix0 back as a short, so 2 W (and 2 H) must stay below 32768; ldm_gemm's host
check allowed H, W < 32768 regardless of `upsample` and was tightened to 2 H, 2 W < 32768 with this module (rejection
test in test_gemm_accounting_gpu.py; nothing is launched at such a size).

First run on an MI355X: see RESULTS at the end of this docstring.

ACTIVATION EPILOGUES (`epilogue_cases`, run by test_zz_gemm_epilogue_gpu.py, proven by test_gemm_epilogue_probes_cpu.py)
  The cases above run with act = NONE.  An activation cannot keep integer outputs, so these cases make the value BEFORE
  it exact instead: the selection probe with one phase, wt one-hot of value 2^-4 (a power of two in the weights, not in
  alpha: the persistent tiles demand alpha == 1), A = `ecode` in +-31, bias / addend / residual = k 2^-4 with |k| <= 16.
  Every z = a 2^-4 + bias + addend is a multiple of 2^-4 with |z| <= 3.94; on that grid one step moves GELU or SiLU by
  at least 3.4e-5 up to |z| = 4.  LayerNorm fold: rows of +-1 in equal numbers and eps = 2^-30 give mean = 0 and
  rstd = 1 exactly in float32 (the real-number rstd differs by 2^-31, a thousandth of the smallest ceiling), the weights
  carry wv(n) 2^-4.  `reference_pre` is the exact z (`reference` without the residual), `reference_act` the float64
  activation in the header's GEGLU layout (output column c pairs logical columns (c >> 5) 64 + (c & 31) and + 32) plus the
  residual.  Gates: uniformity (exact), a derived ceiling per element (`ceiling`: float32 2e-6 for GELU / SiLU = A&S
  7.1.26 at 1.5e-7 on erf, 3e-7 at |z| = 4, + exp2 / rcp at 1 ulp each + the output's rounding; a float32 emulation of
  gelu_erf_f / silu_f with exact exp2 / rcp stays below 6e-7 on the grid; GEGLU |value| 2e-6 + 2^-23 |ref|; bf16 output
  + 2^-8 |ref|) and a measured gate (GPU module).  `EPI_MUTATIONS`: each moves some element by more than 8 ceilings in
  every case it applies to; exempt: geglu_* without GEGLU, geglu_gate_bias_missing / _addend_missing without that term,
  act_before_bias and bias_column without bias and addend, residual_inside_act without residual, stored_width unless
  GEGLU spans more than one n-tile.  The matrix: the docstring of test_zz_gemm_epilogue_gpu.py and `_epi_cases`.

RESULTS
  every form of the matrix (tiles 0-19, both storage types where the tile has them, plain rows, the three convolution
  forms, the halo-staged tiles, split-K with both reduce kernels, the persistent tiles in both deals) passed both probes
  with equality when first run; no kernel was changed.  The host check of the upsampled form was tightened (above).
"""
import math
from collections import namedtuple

import torch

F32, BF, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
MAX_PHASES = 4

# ---- the tile table: bm, bn, LDS ring depth, bf16 only (gemm_tiles.h kTiles, gemm_kernel.h NSTAGE; the tests
# cross-check bm / bn with ops._TILE_DIMS, ldm_gemm_tile_info and ldm_gemm's own rejections) -----------------------
Tile = namedtuple("Tile", "bm bn stages bf16_only")
TILES = {1: Tile(256, 128, 3, False), 2: Tile(128, 128, 2, False), 3: Tile(128, 64, 2, False), 4: Tile(64, 64, 2, False),
         5: Tile(256, 128, 2, False), 6: Tile(128, 160, 2, False), 7: Tile(256, 160, 3, False), 8: Tile(128, 320, 2, False),
         9: Tile(256, 160, 3, True), 10: Tile(128, 160, 2, True), 11: Tile(256, 128, 3, True), 12: Tile(128, 128, 2, True),
         13: Tile(256, 160, 3, True), 14: Tile(256, 128, 3, True), 15: Tile(256, 160, 3, True), 16: Tile(256, 128, 3, True),
         17: Tile(64, 64, 4, False), 18: Tile(128, 64, 3, False), 19: Tile(128, 128, 3, False)}
PERSISTENT, HALO = (13, 14), (15, 16)
AUTO_NOMINAL = Tile(128, 128, 2, False)      # tile 0: the edges the matrix aims at (the cost model picks the real tile)
AUTO_GRID = Tile(64, 64, 2, False)           # ... and the grid on which its census keeps every K column alive

# name, tile, storage type of a / w, wg (persistent tiles: split_k handed to ldm_gemm, -1 = one workgroup per panel)
Form = namedtuple("Form", "name tile dt wg")


def _forms():
  out = []
  for t in (0, 1, 2, 3, 4, 5, 6, 7, 8, 17, 18, 19):
    out += [Form(f"t{t}-bf16", t, BF, 0), Form(f"t{t}-f32", t, F32, 0)]
  out += [Form(f"t{t}-bf16", t, BF, 0) for t in (9, 10, 11, 12)]
  for t in PERSISTENT:
    out += [Form(f"t{t}-bf16-wg1", t, BF, -1), Form(f"t{t}-bf16-deal", t, BF, 0)]
  out += [Form(f"t{t}-bf16", t, BF, 0) for t in HALO]
  return out


FORMS = {f.name: f for f in _forms()}


def tile_of(form):
  return TILES[form.tile] if form.tile else AUTO_NOMINAL


def grid_of(form):
  return TILES[form.tile] if form.tile else AUTO_GRID


def bke_of(form):
  return 64 if form.dt == BF else 32


_FIELDS = dict(form="", kind="plain", M=0, N=0, K=0, K2=0, B=0, H=0, W=0, Cin=0, stride=1, up=0, nlp=0,
               bias=0, addend=0, add_rows=0, res=0, alpha=1.0, odt=None, lda_x=0, ldc_x=0, ldr_x=0, lda2_x=0, off8=0,
               split=1, defer=0, in_slice=0, out_slice=0, Bt=1, shared_w=0, trans=0, G=1, sel=0, tag="",
               act=0, boff=0, lnf=0, rej="")
Case = namedtuple("Case", list(_FIELDS), defaults=list(_FIELDS.values()))
# act: 0 | "gelu" | "silu" | "geglu" (the activation-epilogue matrix at the end of this module; all_cases() has none);
# boff: the bias is a slice that starts 4 bytes behind a 16-byte boundary; lnf: LayerNorm fold (ops.linear(ln_fold=));
# rej: the launch must be rejected with a message that matches this pattern
# kind: plain (ops.linear) | conv (ops.conv3x3) | bmm (ops.bmm_nt) | lint (ops.linear_t) | out2 (ops.linear(out2=))
#   out2: columns [0, N - K2x) row-major, the rest transposed per group of M / G rows; `G` groups (lint too)
# lda_x / ldc_x / ldr_x / lda2_x: extra elements in the row pitch of a / out / residual / a2; off8: out starts 8 bytes
# behind a 16-byte boundary; in_slice / out_slice: the conv image / output is a channel slice of a wider buffer


def conv_dims(c):
  hs, ws = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
  pads = 1 if c.nlp else 2
  return hs, ws, (hs + pads - 3) // c.stride + 1, (ws + pads - 3) // c.stride + 1


def _mk(form, kind="plain", **kw):
  f = FORMS[form]
  kw.setdefault("odt", f.dt)
  c = Case(form=form, kind=kind, **kw)
  if kind == "conv":
    _, _, oh, ow = conv_dims(c)
    assert oh > 0 and ow > 0, c
    c = c._replace(M=c.B * oh * ow, K=9 * c.Cin + c.K2, add_rows=oh * ow)
  if c.addend and not c.add_rows:
    c = c._replace(add_rows=c.M)
  return c


def case_id(c):
  s = f"{c.form}-{c.kind}-M{c.M}N{c.N}K{c.K}"
  if c.kind == "conv":
    s += f"-B{c.B}x{c.H}x{c.W}c{c.Cin}-s{c.stride}u{c.up}n{c.nlp}"
  if c.K2:
    s += f"-x2_{c.K2}"
  if c.Bt > 1:
    s += f"-bt{c.Bt}{'s' if c.shared_w else 'p'}{'T' if c.trans else ''}"
  s += "-e" + "".join(ch for ch, on in zip("bar", (c.bias, c.addend, c.res)) if on)
  if c.alpha != 1.0:
    s += f"-al{c.alpha}"
  if c.odt != FORMS[c.form].dt:
    s += "-o" + ("bf16" if c.odt == BF else "f32")
  if c.split != 1:
    s += f"-sk{c.split}"
  s += "".join(f"-{n}" for n, on in (("defer", c.defer), ("off8", c.off8), ("islice", c.in_slice), ("oslice", c.out_slice),
                                     ("lda", c.lda_x), ("ldc", c.ldc_x), ("ldr", c.ldr_x), ("lda2", c.lda2_x)) if on)
  return s + (f"-{c.tag}" if c.tag else "")


# ---- K-tiles ------------------------------------------------------------------------------------------
def ktiles_of(c):
  return c.K // bke_of(FORMS[c.form])


def ktile_cols(c, kt):
  """Columns of the [N][K] weight matrix that K-tile `kt` of the kernels' K order covers (conv: kt = chunk * 9 + tap over
  the first operand, then the K-tiles of the second)."""
  bke = bke_of(FORMS[c.form])
  if c.kind != "conv":
    return torch.arange(kt * bke, (kt + 1) * bke)
  kt9 = 9 * c.Cin // bke
  if kt >= kt9:
    return 9 * c.Cin + torch.arange((kt - kt9) * bke, (kt - kt9 + 1) * bke)
  cc, tap = divmod(kt, 9)
  return tap * c.Cin + torch.arange(cc * bke, (cc + 1) * bke)


def ktile_of_col(c):
  """[K]: the K-tile each weight column belongs to."""
  out = torch.empty(c.K, dtype=I64)
  for kt in range(ktiles_of(c)):
    out[ktile_cols(c, kt)] = kt
  return out


def expected_slabs(c):
  """The number of split-K slabs ldm_gemm writes (gemm.hip final_plan): whole K-tile ranges, the halo-staged tiles at
  whole channel chunks, empty trailing splits dropped."""
  f = FORMS[c.form]
  if f.tile in PERSISTENT or c.split <= 1:
    return 1
  kts = ktiles_of(c)
  kps = -(-kts // c.split)
  if f.tile in HALO:
    kps = -(-kps // 9) * 9
  return -(-kts // kps)


# ---- deterministic integers ---------------------------------------------------------------------------
def _gen(*key):
  return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1))


def _key(c):
  return (FORMS[c.form].tile, c.M, c.N, c.K, c.B, c.H, c.W, c.stride + 2 * c.up + 4 * c.nlp, c.Bt)


def _ints(g, shape, lo, hi):
  return torch.randint(lo, hi + 1, shape, generator=g, dtype=I64)


def code(p, ch):
  """The position code of element (pixel or row p, channel or column ch): non-zero, in [-127, 127].  |code| - 1 =
  (37 p + 11 ch) mod 127 with 127 prime: two elements whose p differ by d (0 < |d| < 127) or whose ch differ by 8, 32
  or 64 differ in |code|."""
  mag = 1 + (37 * p + 11 * ch) % 127
  return torch.where((p + ch // 8) % 3 == 0, -mag, mag)


# ---- the source pixel of every (row, tap): include/ldm_hip.h, conv = 1 --------------------------------
def conv_src(c, mut=None):
  """src [M, 9] int64: the flat pixel (b H + y) W + x that tap t = 3 kh + kw of output row m = (b, oy, ox) reads, -1 where
  it is padding.  From the header: source pixel (oy stride + kh - 1, ox stride + kw - 1) of the (nearest-2x upsampled:
  src[i][j] = img[i / 2][j / 2]) image, zero outside; no_lead_pad: no row / column before the image.
  `mut`: the gather of a subtly wrong kernel (module docstring)."""
  hs, ws, oh, ow = conv_dims(c)
  pad = 0 if c.nlp else 1
  if mut == "origin":
    pad = 1 - pad
  m = torch.arange(c.M)
  b, oy, ox = m // (oh * ow), (m % (oh * ow)) // ow, m % ow
  total = c.B * c.H * c.W
  src = torch.full((c.M, 9), -1, dtype=I64)
  for kh in range(3):
    for kw in range(3):
      iy, ix = oy * c.stride + kh - pad, ox * c.stride + kw - pad
      oky, okx = (iy >= 0) & (iy < hs), (ix >= 0) & (ix < ws)
      sy, sx = (iy // 2, ix // 2) if c.up else (iy, ix)             # floor: -1 // 2 = -1, the kernels' >> 1
      ok = oky & okx
      if mut == "up_odd" and c.up:                                    # odd coordinates not halved
        sy, sx = torch.where(iy % 2 == 1, iy, sy), torch.where(ix % 2 == 1, ix, sx)
        ok = ok & (sy < c.H) & (sx < c.W)
      p = (b * c.H + sy) * c.W + sx
      if mut == "line_end" and kh == 1:                               # the linear neighbour instead of the zero column
        ok = ok | (oky & ((ix == -1) | (ix == ws)) & (p >= 0) & (p < total))
      if mut == "prev_image" and c.B > 1:                             # the neighbouring image instead of the zero line
        ok = ok | (okx & ((iy == -1) | (iy == hs)) & (p >= 0) & (p < total))
      src[:, kh * 3 + kw] = torch.where(ok, p, torch.full_like(p, -1))
  return src


def gather_rows(c, img, src):
  """A [M, 9 Cin]: the implicit-GEMM rows, k = (kh, kw, ci); img [B, H, W, Cin]."""
  flat = img.reshape(-1, img.shape[-1])
  rows = flat[src.clamp_min(0)] * (src >= 0).unsqueeze(2).to(img.dtype)          # [M, 9, Cin]
  return rows.reshape(c.M, 9 * img.shape[-1])


# ---- probe data: a dict of int64 tensors (residual: float64, multiples of 1/2 never occur there) -----------
def _a_full(c, d, mut=None):
  """[Bt, M, K]: every row of the product's A operand, the second operand's columns behind the first's."""
  if c.kind == "conv":
    a = gather_rows(c, d["a"], conv_src(c, mut))
  else:
    a = d["a"]
  if c.K2:
    a2 = d["a2"].reshape(c.M, c.K2)
    if mut == "a2_next_pixel":
      a2 = a2.roll(-1, 0)
    a = torch.cat([a.reshape(c.M, -1), a2], 1)
  return a.reshape(c.Bt, c.M, c.K)


def _tiles(n, b):
  return [(i, min(i + b, n)) for i in range(0, n, b)]


def _revive(mat, rows, g):
  """mat [R, K]: in every row range of `rows`, a column that holds no non-zero entry gets one (+-1)."""
  for r0, r1 in rows:
    dead = ((mat[r0:r1] != 0).sum(0) == 0).nonzero().flatten()
    if dead.numel():
      sign = _ints(g, (dead.numel(),), 0, 1) * 2 - 1
      mat[r0 + dead % (r1 - r0), dead] = sign
  return mat


def probe_census(c):
  f = FORMS[c.form]
  t, g = grid_of(f), _gen(2, *_key(c))
  K1 = c.K - c.K2

  def dense(shape):
    return _ints(g, shape, 1, 2) * (_ints(g, shape, 0, 1) * 2 - 1) * _ints(g, shape, 0, 1)

  d = {}
  if c.kind == "conv":
    img = dense((c.B, c.H, c.W, c.Cin))
    src = conv_src(c)
    flat = img.reshape(-1, c.Cin)
    for r0, r1 in _tiles(c.M, t.bm):                                   # every tap that some row of the M-tile reads: alive
      for tap in range(9):
        px = src[r0:r1, tap]
        px = px[px >= 0]
        if px.numel():
          dead = ((flat[px] != 0).sum(0) == 0).nonzero().flatten()
          flat[px[dead % px.numel()], dead] = 1
    d["a"] = img
  else:
    a = dense((c.Bt, c.M, K1))
    for b in range(c.Bt):
      _revive(a[b], _tiles(c.M, t.bm), g)
    d["a"] = a
  if c.K2:
    d["a2"] = _revive(_ints(g, (c.M, c.K2), -8, 8), _tiles(c.M, t.bm), g)
  dens = min(0.25, 360.0 / c.K)
  nw = 1 if (c.shared_w or c.Bt == 1) else c.Bt
  w = (_ints(g, (nw, c.N, c.K), 0, 1) * 2 - 1) * (torch.rand((nw, c.N, c.K), generator=g) < dens).to(I64)
  for b in range(nw):
    _revive(w[b], _tiles(c.N, t.bn), g)
  d["w"] = w
  if c.bias:
    d["bias"] = _ints(g, (c.N,), -8, 8)
  if c.addend:
    d["addend"] = _ints(g, (-(-c.M // c.add_rows), c.N), -8, 8)
  if c.res:
    d["res"] = _ints(g, (c.M, c.N + c.ldr_x), -8, 8)                  # the whole buffer, pad columns included
  return d


def phases(c):
  """The phases probe 1 runs: ceil(K / N) of them select every K column; at most MAX_PHASES, picked greedily so that the
  K-tiles they select cover all (the CPU test asserts the cover)."""
  P = -(-c.K // c.N)
  kt = ktile_of_col(c)
  n = torch.arange(c.N)
  need, picked = set(range(ktiles_of(c))), []
  hits = {ph: set(kt[(n * P + ph) % c.K].tolist()) for ph in range(P)}
  while need and len(picked) < min(P, MAX_PHASES):
    ph = max((p for p in range(P) if p not in picked), key=lambda p: (len(hits[p] & need), -p))
    picked.append(ph)
    need -= hits[ph]
  return picked or [0]


def selected_column(c, phase):
  return (torch.arange(c.N) * -(-c.K // c.N) + phase) % c.K


def probe_selection(c, phase):
  """A = the position code, W one-hot at selected_column(c, phase); no epilogue term."""
  K1 = c.K - c.K2
  d = {}
  if c.kind == "conv":
    p = torch.arange(c.B * c.H * c.W).view(c.B, c.H, c.W, 1)
    d["a"] = code(p, torch.arange(c.Cin).view(1, 1, 1, c.Cin))
  else:
    r = torch.arange(c.Bt * c.M).view(c.Bt, c.M, 1)
    d["a"] = code(r, torch.arange(K1).view(1, 1, K1))
  if c.K2:
    d["a2"] = code(torch.arange(c.M).view(c.M, 1) + 50, torch.arange(c.K2).view(1, c.K2) + 3)
  nw = 1 if (c.shared_w or c.Bt == 1) else c.Bt
  w = torch.zeros(nw, c.N, c.K, dtype=I64)
  for b in range(nw):
    w[b, torch.arange(c.N), (selected_column(c, phase) + 7 * b) % c.K] = 1
  d["w"] = w
  return d


def as_selection(c):
  """The case probe 1 runs for `c`: the same launch geometry without epilogue terms and with alpha = 1."""
  return c._replace(bias=0, addend=0, res=0, alpha=1.0, ldr_x=0)


# ---- the reference -----------------------------------------------------------------------------------------
MUTATIONS = ("drop_column", "double_ktile", "drop_last_ktile", "pair_off_by_one", "line_end", "prev_image", "origin",
             "up_odd", "swap_rows", "bias_column", "residual_stride", "a2_next_pixel")


def _mid_ktile(c):
  """A K-tile in the middle of K that no geometry turns into padding (conv: the centre tap of the middle chunk)."""
  if c.kind == "conv":
    return (c.Cin // bke_of(FORMS[c.form]) // 2) * 9 + 4
  return ktiles_of(c) // 2


def mutation_applies(c, kind):
  """False where the mutation cannot change a correct result (the exempt cases of the module docstring)."""
  conv = c.kind == "conv"
  if kind == "drop_last_ktile":
    return not conv or bool(c.K2) or bool((conv_src(c)[:, 8] >= 0).any())
  if kind == "pair_off_by_one":
    return ktiles_of(c) > 1
  if kind in ("line_end", "prev_image", "origin", "up_odd"):
    return conv and not torch.equal(conv_src(c, kind), conv_src(c))
  if kind == "swap_rows":
    return c.M > 1
  if kind == "bias_column":
    return bool(c.bias or c.addend)
  if kind == "residual_stride":
    return bool(c.res and c.ldr_x)
  if kind == "a2_next_pixel":
    return bool(c.K2) and c.M > 1
  return True


def reference(c, d, mut=None):
  """[Bt, M, N] float64: alpha sum_k A[m][k] W[n][k] + bias[n] + addend[m / add_rows][n] + residual[m][n], exact (every
  term is an integer or, with alpha = 0.5, a multiple of 1/2, far below 2^53).  `mut`: one of MUTATIONS."""
  a = _a_full(c, d, mut).to(F64)
  w = d["w"].to(F64)
  t = grid_of(FORMS[c.form])
  kts = ktiles_of(c)
  if mut == "drop_column":                         # one K column lost in the last N-tile
    n0 = (c.N - 1) // t.bn * t.bn
    k = (4 * c.Cin + 5) if c.kind == "conv" else (c.K // 2 + 5) % c.K      # (conv: the centre tap, never padding)
    w = w.clone()
    w[:, n0:, k] = 0
  if mut == "pair_off_by_one":
    w2 = torch.empty_like(w)
    for kt in range(kts):
      w2[:, :, ktile_cols(c, kt)] = w[:, :, ktile_cols(c, (kt + 1) % kts)]
    w = w2
  acc = a @ w.transpose(1, 2)
  if mut in ("double_ktile", "drop_last_ktile"):
    cols = ktile_cols(c, _mid_ktile(c) if mut == "double_ktile" else kts - 1)
    part = a[:, :, cols] @ w[:, :, cols].transpose(1, 2)
    acc = acc + part if mut == "double_ktile" else acc - part
  out = c.alpha * acc
  if c.bias:
    bias = d["bias"].to(F64)
    out = out + (bias.roll(-1) if mut == "bias_column" else bias)
  if c.addend:
    ad = d["addend"].to(F64)
    if mut == "bias_column":
      ad = ad.roll(-1, 0) if ad.shape[0] > 1 else ad.roll(-1, 1)
    out = out + ad[torch.arange(c.M) // c.add_rows]
  if c.res:
    res = d["res"].to(F64)
    if mut == "residual_stride":
      res = res.flatten()[:c.M * c.N].view(c.M, c.N)
    out = out + res[:, :c.N]
  if mut == "swap_rows":
    i, j = (t.bm - 1, t.bm) if c.M > t.bm else (0, c.M - 1)
    out = out.clone()
    out[:, [i, j]] = out[:, [j, i]]
  return out


def partial_sum_bound(c, d):
  """An upper bound of every partial sum of the product and of the epilogue: sum_k max|a| max|w| + the epilogue terms."""
  amax = max(int(d["a"].abs().max()), int(d["a2"].abs().max()) if c.K2 else 0)
  return amax * int(d["w"].abs().max()) * c.K * max(1.0, c.alpha) + 8 * 3


def alive_everywhere(c, d):
  """True if in every (M-tile, N-tile) of the form every K column has a non-zero product in some output.  A conv tap
  that is padding for every row of an M-tile is exempt there."""
  t = grid_of(FORMS[c.form])
  a = _a_full(c, d)
  if c.kind == "conv":
    valid = (conv_src(c) >= 0)                                         # [M, 9]
  for b in range(c.Bt):
    w = d["w"][0 if d["w"].shape[0] == 1 else b]
    for n0, n1 in _tiles(c.N, t.bn):
      if not bool((w[n0:n1] != 0).any(0).all()):
        return False
    for r0, r1 in _tiles(c.M, t.bm):
      alive = (a[b, r0:r1] != 0).any(0)
      if c.kind == "conv":
        can = valid[r0:r1].any(0).repeat_interleave(c.Cin)
        can = torch.cat([can, torch.ones(c.K2, dtype=torch.bool)])
        alive = alive | ~can
      if not bool(alive.all()):
        return False
  return True


def representable(ref, dtype):
  return bool((ref.to(F32).to(dtype).to(F64) == ref).all())


# ---- failure report ---------------------------------------------------------------------------------------
def decode_row(c, m):
  if c.kind != "conv":
    return f"row {m}"
  _, _, oh, ow = conv_dims(c)
  return f"(b, oy, ox) = ({m // (oh * ow)}, {m % (oh * ow) // ow}, {m % ow})"


def first_difference(c, got, ref, phase=None, d=None):
  """Text for a failed case: the first differing (batch, m, n), decoded; for probe 1 the (tap, ci) that was expected and
  the coordinates near it whose code equals what came back."""
  bad = (got != ref) | torch.isnan(got)
  if not bool(bad.any()):
    return ""
  nbad = int(bad.sum())
  bt, m, n = [int(v) for v in bad.nonzero()[0]]
  s = (f"{case_id(c)}: {nbad} of {bad.numel()} elements differ; first at batch {bt}, (m, n) = ({m}, {n}), "
       f"{decode_row(c, m)}: got {float(got[bt, m, n])}, want {float(ref[bt, m, n])}")
  if phase is None:
    return s
  k = int(selected_column(c, phase)[n])
  s += f"; phase {phase} selects column k = {k}"
  v = float(got[bt, m, n])
  if c.kind == "conv" and k < 9 * c.Cin:
    tap, ci = divmod(k, c.Cin)
    s += f" = (tap ({tap // 3}, {tap % 3}), ci {ci}), source pixel {int(conv_src(c)[m, tap])} (-1: padding)"
    _, _, oh, ow = conv_dims(c)
    b, oy, ox = m // (oh * ow), m % (oh * ow) // ow, m % ow
    cy, cx = oy * c.stride // (2 if c.up else 1), ox * c.stride // (2 if c.up else 1)
    hits = []
    for bb in range(max(0, b - 1), min(c.B, b + 2)):
      for y in range(max(0, cy - 3), min(c.H, cy + 4)):
        for x in range(max(0, cx - 3), min(c.W, cx + 4)):
          for ch in sorted({ci, ci - 8, ci + 8, ci - 32, ci + 32, ci - 64, ci + 64}):
            if 0 <= ch < c.Cin and float(code(torch.tensor((bb * c.H + y) * c.W + x), torch.tensor(ch))) == v:
              hits.append((bb, y, x, ch))
    s += f"; image elements (b, y, x, ci) near it that hold {v}: {hits[:8]}"
  elif c.kind != "conv":
    hits = [(r, kk) for r in range(max(0, m - 2), min(c.M, m + 3))
            for kk in sorted({k, k - 8, k + 8, k - 32, k + 32, k - 64, k + 64})
            if 0 <= kk < c.K - c.K2 and float(code(torch.tensor(bt * c.M + r), torch.tensor(kk))) == v]
    s += f"; elements (row, k) near it that hold {v}: {hits[:8]}"
  return s


# ---- the matrix -------------------------------------------------------------------------------------------
GEOMS = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (5, 7), (7, 6), (13, 17), (12, 20), (24, 40))
# per geometry: the forms beside stride 1 (s2 = stride 2, pad 1; nlp = stride 2, no_lead_pad; up = upsampled)
_GEOM_MODES = {(1, 1): ("up", "s2"), (1, 9): ("s2",), (9, 1): ("up",), (2, 2): ("nlp", "s2"), (3, 5): ("nlp", "up"),
               (5, 7): ("s2",), (7, 6): ("nlp", "s2"), (13, 17): ("up", "s2"), (12, 20): ("s2", "nlp"),
               (24, 40): ("up",)}
# probe 1 per form: the two smallest and the two most ragged geometries that have it
_SEL_GEOMS = {"s1": ((1, 1), (2, 2), (5, 7), (13, 17)), "s2": ((1, 1), (1, 9), (5, 7), (13, 17)),
              "nlp": ((2, 2), (3, 5), (7, 6), (12, 20)), "up": ((1, 1), (9, 1), (3, 5), (13, 17))}
_EPIS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1))            # (bias, addend, residual)
_MODE_KW = {"s1": {}, "s2": dict(stride=2), "nlp": dict(stride=2, nlp=1), "up": dict(up=1)}


def m_values(t):
  return [1, 31, 33, t.bm - 1, t.bm, t.bm + 1, 2 * t.bm + 5]


def n_values(t):
  return [8, t.bn - 8, t.bn, t.bn + 8, 2 * t.bn + 24]


def kt_values(t):
  return sorted({1, t.stages - 1, t.stages, t.stages + 1, 2 * t.stages + 1, 40})


def _plain_cases(f):
  t, bke, name = tile_of(f), bke_of(f), f.name
  other = F32 if f.dt == BF else BF
  out = []
  add = lambda **kw: out.append(_mk(name, **kw))
  if f.tile in PERSISTENT:
    # N = whole n-tiles, bf16 out, alpha = 1, the epilogues the kernel is built with (none, bias, bias + residual, residual)
    epis = ((0, 0), (1, 0), (1, 1), (0, 1))
    for i, M in enumerate(m_values(t)):
      b, r = epis[i % 4]
      add(M=M, N=t.bn * (1 + i % 3), K=bke * (t.stages + 1), bias=b, res=r, split=f.wg, sel=M in (1, 31, t.bm + 1, 2 * t.bm + 5))
    for i, kt in enumerate(kt_values(t)):
      b, r = epis[(i + 1) % 4]
      add(M=33 + 256 * (i % 2), N=t.bn * (2 + i % 2), K=bke * kt, bias=b, res=r, split=f.wg, sel=1)
    add(M=t.bm + 1, N=2 * t.bn, K=bke * 5, bias=1, res=1, lda_x=8, ldc_x=16, ldr_x=8, split=f.wg, sel=1, tag="strided")
    add(kind="lint", M=3 * 96, G=3, N=2 * t.bn, K=bke * 4, sel=1)
    add(kind="lint", M=2 * 352, G=2, N=t.bn, K=bke * 7, lda_x=8)
    return out
  if f.tile in HALO:
    return out
  for i, M in enumerate(m_values(t)):
    b, a, r = _EPIS[i % 5]
    add(M=M, N=t.bn + 8, K=bke * (t.stages + 1), bias=b, addend=a, add_rows=37 if a else 0, res=r,
        sel=M in (1, 31, t.bm + 1, 2 * t.bm + 5))
  for i, N in enumerate(n_values(t)):
    b, a, r = _EPIS[(i + 2) % 5]
    add(M=t.bm + 1, N=N, K=bke * t.stages, bias=b, addend=a, add_rows=50 if a else 0, res=r, sel=N in (8, 2 * t.bn + 24))
  for i, kt in enumerate(kt_values(t)):
    b, a, r = _EPIS[(i + 1) % 5]
    add(M=33, N=t.bn + 8, K=bke * kt, bias=b, addend=a, res=r, sel=1, tag="kt")
  # the scalar epilogue: N % 8 != 0, and an output 8 bytes behind a 16-byte boundary
  add(M=t.bm + 1, N=77, K=bke * (t.stages + 1), bias=1, addend=1, add_rows=37, res=1, sel=1)
  add(M=33, N=100, K=bke * 3, bias=1, res=1)
  add(M=t.bm + 1, N=t.bn + 8, K=bke * 3, bias=1, addend=1, add_rows=37, res=1, off8=1, sel=1)
  # pitches: strided A, output and residual; an addend group that does not divide bm
  add(M=t.bm + 5, N=t.bn + 8, K=bke * 5, bias=1, addend=1, add_rows=37, res=1, lda_x=8, ldc_x=16, ldr_x=8, sel=1, tag="strided")
  add(M=70, N=72, K=bke * 4, res=1, ldr_x=8, ldc_x=8)
  add(M=33, N=t.bn, K=bke * 3, bias=1, alpha=0.5)
  add(M=t.bm + 1, N=24, K=bke * 4, bias=1, res=1, alpha=2.0)
  add(M=33, N=t.bn + 8, K=bke * 4, bias=1, odt=other, tag="odt")
  # second A operand with its own pitch
  add(M=t.bm + 1, N=t.bn + 8, K=bke * 5, K2=bke * 2, bias=1, res=1, lda2_x=8, sel=1)
  add(M=33, N=40, K=bke * 2, K2=bke, lda_x=8, lda2_x=16)
  # batched: 3 batches, shared and per-batch W, row-major and transposed with a padded pitch
  add(kind="bmm", Bt=3, M=t.bm + 1, N=t.bn + 8, K=bke * 3, shared_w=1, bias=1, sel=1)
  add(kind="bmm", Bt=3, M=33, N=t.bn + 8, K=bke * 4, alpha=0.5)
  add(kind="bmm", Bt=3, M=t.bm + 5, N=40, K=bke * 3, trans=1, sel=1)
  add(kind="bmm", Bt=3, M=31, N=t.bn + 8, K=bke * 2, shared_w=1, trans=1, bias=1)
  if f.tile:
    # second, transposed output for the columns behind n_split = bn (K2 columns; G groups of M / G rows)
    add(kind="out2", M=3 * 44, G=3, N=t.bn + 40, K=bke * 3, bias=1, sel=1)
    # split-K: even division, a short last slab, dropped empty trailing splits; both reduce kernels; deferred reduce
    add(M=t.bm + 1, N=t.bn + 8, K=bke * 8, split=2, bias=1, addend=1, add_rows=37, res=1, sel=1)
    add(M=33, N=t.bn + 8, K=bke * 10, split=4, bias=1, res=1, sel=1)
    add(M=t.bm + 1, N=72, K=bke * 9, split=4, bias=1, addend=1, add_rows=37, sel=1)
    add(M=33, N=77, K=bke * 10, split=4, bias=1, addend=1, add_rows=20, res=1, sel=1)
    add(M=t.bm + 1, N=t.bn + 8, K=bke * 9, split=4, bias=1, addend=1, add_rows=37, res=1, off8=1)
    add(M=70, N=t.bn, K=bke * 9, split=4, bias=1, res=1, defer=1)
    add(M=33, N=100, K=bke * 7, split=3, bias=1, defer=1)
    add(M=t.bm + 1, N=40, K=bke * 6, K2=bke * 2, split=3, bias=1, res=1, lda2_x=8)
  return out


def _conv_cases(f):
  t, bke, name = tile_of(f), bke_of(f), f.name
  pers = f.tile in PERSISTENT
  out = []
  if f.tile in HALO or f.tile == 5:
    return out
  couts = (t.bn, 2 * t.bn, t.bn) if pers else (8, t.bn, t.bn + 8)
  # persistent tiles: the conv kernels are built with none, bias, bias + addend, bias + residual
  epis = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1)) if pers else _EPIS
  split = f.wg if pers else 1
  i = 0
  for gi, (H, W) in enumerate(GEOMS):
    for mode in ("s1",) + _GEOM_MODES[(H, W)]:
      B = (1, 3, 5)[(gi + i) % 3]
      if H * W >= 240 and mode == "up":
        B = 1
      cout = couts[i % 3]
      chunks = (1, 2, 3, 5)[i % 4]
      if cout == 8 or H * W >= 240:
        chunks = 1 + i % 2                                           # (probe 1 covers 9 / 18 K-tiles with 8 columns)
      b, a, r = epis[i % len(epis)]
      out.append(_mk(name, "conv", B=B, H=H, W=W, Cin=chunks * bke, N=cout, bias=b, addend=a, res=r, split=split,
                     sel=int((H, W) in _SEL_GEOMS[mode]), **_MODE_KW[mode]))
      i += 1
  add = lambda **kw: out.append(_mk(name, "conv", split=kw.pop("split", split), **kw))
  # channel slices of wider buffers in and out
  add(B=3, H=5, W=7, Cin=2 * bke, N=t.bn, bias=1, res=1, in_slice=1, out_slice=1, sel=1)
  add(B=2, H=7, W=6, Cin=bke, N=t.bn, bias=1, in_slice=1, out_slice=1, up=1)
  add(B=3, H=7, W=6, Cin=3 * bke, N=t.bn, bias=1, addend=1, in_slice=1, stride=2, nlp=1)
  if not pers:
    # second operand: a channel-sliced second image
    add(B=3, H=5, W=7, Cin=2 * bke, K2=bke, N=t.bn + 8, bias=1, res=1, lda2_x=8, sel=1)
    add(B=1, H=13, W=17, Cin=bke, K2=2 * bke, N=t.bn, bias=1, addend=1, lda2_x=16, in_slice=1)
    if f.tile:
      add(B=3, H=3, W=5, Cin=2 * bke, N=t.bn + 8, bias=1, addend=1, res=1, split=2, sel=1)         # 18 K-tiles: 9 + 9
      add(B=5, H=2, W=2, Cin=3 * bke, N=72, bias=1, res=1, split=4)                                # 27: 7, 7, 7, 6
      add(B=1, H=13, W=17, Cin=bke, N=t.bn, bias=1, split=4, sel=1)                                # 9 at 4: 3 slabs
      add(B=3, H=7, W=6, Cin=bke, N=t.bn, bias=1, addend=1, split=4, defer=1, stride=2)
      add(B=2, H=5, W=7, Cin=2 * bke, K2=bke, N=40, bias=1, split=3, up=0, lda2_x=8)
      add(B=1, H=9, W=1, Cin=bke, N=t.bn + 8, bias=1, res=1, split=2, up=1, out_slice=1)
  return out


def _halo_cases(f):
  t, name = tile_of(f), f.name
  out = []
  geoms = [(16, 16), (32, 16), (48, 16), (8, 32), (16, 32), (24, 32), (40, 32)]
  for i, (H, W) in enumerate(geoms):
    b, a, r = _EPIS[i % 5]
    chunks = (1, 2, 3, 5)[i % 4]
    out.append(_mk(name, "conv", B=(1, 3)[i % 2], H=H, W=W, Cin=64 * chunks, N=t.bn * (1 + i % 2), bias=b, addend=a, res=r,
                   split=(1, 2, 3)[i % 3] if chunks >= 3 else 1 + (chunks == 2) * (i % 2), sel=int(i < 4)))
  add = lambda **kw: out.append(_mk(name, "conv", **kw))
  add(B=3, H=16, W=16, Cin=320, N=t.bn, bias=1, addend=1, res=1, split=2, sel=1)            # 45 K-tiles: 27 + 18
  add(B=1, H=8, W=32, Cin=320, N=2 * t.bn, bias=1, split=3, defer=1)                        # 18 + 18 + 9
  add(B=3, H=16, W=32, Cin=192, N=t.bn, bias=1, res=1, split=1)
  add(B=1, H=48, W=16, Cin=128, N=t.bn, bias=1, in_slice=1, split=2, sel=1)
  add(B=3, H=24, W=32, Cin=64, N=t.bn, in_slice=1, out_slice=1, res=1)
  add(B=1, H=16, W=16, Cin=192, N=t.bn, bias=1, addend=1, split=4)                          # 27 at 4: 9 + 9 + 9
  return out


def cases(f):
  return _plain_cases(f) + _conv_cases(f) + _halo_cases(f) if f.tile in HALO else _plain_cases(f) + _conv_cases(f)


_ALL = None


def all_cases():
  global _ALL
  if _ALL is None:
    _ALL = [c for f in FORMS.values() for c in cases(f)]
    ids = [case_id(c) for c in _ALL]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:4]
  return _ALL


# ===========================================================================================================
# Activation epilogues: act(alpha sum + bias + addend) + residual on every store path (module docstring, "ACTIVATION
# EPILOGUES"; run by test_zz_gemm_epilogue_gpu.py, proven on the CPU by test_gemm_epilogue_probes_cpu.py)
# ===========================================================================================================
EPI_SCALE = 2.0 ** -4
ACT_CODES = {0: 0, "gelu": 1, "geglu": 2, "silu": 3}                 # include/ldm_hip.h LDM_ACT_*
ALIGN_REJ, ADDEND_REJ = "needs the 16-byte alignment", "GEGLU takes no addend"
EPI_MUTATIONS = ("geglu_pair_shift", "geglu_blocks_swapped", "geglu_gate_bias_missing", "geglu_gate_addend_missing",
                 "act_before_bias", "residual_inside_act", "bias_column", "stored_width", "nothing_stored")
CEIL_F32 = 2e-6                                                      # module docstring: how it is made up
MUTATION_FACTOR = 8.0


def nout_of(c):
  return c.N // 2 if c.act == "geglu" else c.N


def ecode(p, ch):
  """The position code of the epilogue probe: non-zero, in [-31, 31] (31 prime), so that code * 2^-4 + bias + addend
  stays within [-4, 4]."""
  mag = 1 + (37 * p + 11 * ch) % 31
  return torch.where((p + ch // 8) % 3 == 0, -mag, mag)


def probe_epilogue(c):
  """float64 operands, all multiples of 2^-4 that the storage types hold exactly.  wt[n, :] is one-hot at
  selected_column(c, 0) with the value 2^-4 (LayerNorm fold: wv(n) 2^-4), A is `ecode` (LayerNorm fold: rows of +-1 in
  equal numbers, so that mean = 0, E[x^2] = 1 and, with eps = 2^-30, rstd = 1 in float32), bias / addend / residual are
  k 2^-4 with |k| <= 16: z = a[m, k(n)] w + bias[n] + addend[m / add_rows, n] is a multiple of 2^-4 with |z| <= 3.94."""
  s, n = EPI_SCALE, torch.arange(c.N)
  d = {}
  if c.kind == "conv":
    p = torch.arange(c.B * c.H * c.W).view(c.B, c.H, c.W, 1)
    d["a"] = ecode(p, torch.arange(c.Cin).view(1, 1, 1, c.Cin)).to(F64)
  elif c.lnf:
    d["a"] = (1 - 2 * ((torch.arange(c.M).view(1, c.M, 1) + torch.arange(c.K).view(1, 1, c.K)) % 2)).to(F64)
  else:
    d["a"] = ecode(torch.arange(c.M).view(1, c.M, 1), torch.arange(c.K).view(1, 1, c.K)).to(F64)
  wv = (1 + (7 * n) % 31) if c.lnf else torch.ones_like(n)
  w = torch.zeros(1, c.N, c.K, dtype=F64)
  w[0, n, selected_column(c, 0)] = wv.to(F64) * s
  d["w"] = w
  if c.bias:
    d["bias"] = ((5 * n + 3) % 33 - 16).to(F64) * s
  if c.addend:
    g = torch.arange(-(-c.M // c.add_rows)).view(-1, 1)
    d["addend"] = ((7 * n.view(1, -1) + 11 * g + 5) % 33 - 16).to(F64) * s
  if c.res:
    m, q = torch.arange(c.M).view(-1, 1), torch.arange(nout_of(c) + c.ldr_x).view(1, -1)
    d["res"] = ((3 * m + 13 * q + 1) % 33 - 16).to(F64) * s          # the whole buffer, pad columns included
  if c.lnf:
    d["cs"] = w[0].sum(1)
    d["eps"] = 2.0 ** -30
  return d


def gelu64(x):
  return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def silu64(x):
  return x / (1.0 + torch.exp(-x))


def geglu_cols(c):
  """(value, gate) logical columns of every output column: include/ldm_hip.h, blocks of 64 = 32 value rows, 32 gate rows."""
  cc = torch.arange(c.N // 2)
  nv = (cc >> 5) * 64 + (cc & 31)
  return nv, nv + 32


def reference_pre(c, d, mut=None):
  """[Bt, M, N] float64: the exact pre-activation value z of every logical column (`reference` without the residual)."""
  return reference(c._replace(res=0), d, mut)


def _epi_terms(c, d):
  """[M, N]: bias + addend alone."""
  e = torch.zeros(c.M, c.N, dtype=F64)
  if c.bias:
    e = e + d["bias"]
  if c.addend:
    e = e + d["addend"][torch.arange(c.M) // c.add_rows]
  return e


def reference_act(c, d, mut=None):
  """[Bt, M, nout] float64: act(z) + residual in float64 (GELU by erf, SiLU, value * gelu(gate) in the header's layout).
  `mut`: one of EPI_MUTATIONS, the result of a subtly wrong epilogue."""
  z = reference_pre(c, d, "bias_column" if mut == "bias_column" else None)
  epi = _epi_terms(c, d)
  res = d["res"][:, :nout_of(c)] if c.res else None
  inside = mut == "residual_inside_act"
  if c.act == "geglu":
    nv, ng = geglu_cols(c)
    if mut == "geglu_pair_shift":
      ng = (ng + 1) % c.N
    if mut == "geglu_blocks_swapped":
      nv, ng = ng, nv
    v, g = z[..., nv], z[..., ng]
    if mut == "geglu_gate_bias_missing":
      g = g - d["bias"][ng]
    if mut == "geglu_gate_addend_missing":
      g = g - d["addend"][torch.arange(c.M) // c.add_rows][:, ng]
    if mut == "act_before_bias":
      out = (v - epi[:, nv]) * gelu64(g - epi[:, ng]) + epi[:, nv]
    else:
      out = ((v + res) if inside else v) * gelu64(g)
  else:
    f = gelu64 if c.act == "gelu" else silu64
    out = f(z - epi) + epi if mut == "act_before_bias" else f(z + res) if inside else f(z)
  if res is not None and not inside:
    out = out + res
  if mut == "stored_width":                       # output column of n-tile ti computed from ti bn instead of ti bn / 2
    bo = tile_of(FORMS[c.form]).bn // 2
    cc = torch.arange(c.N // 2)
    dest = (cc // bo) * 2 * bo + cc % bo
    moved = torch.full_like(out, float("nan"))
    moved[..., dest[dest < c.N // 2]] = out[..., cc[dest < c.N // 2]]
    out = moved
  if mut == "nothing_stored":
    out = torch.full_like(out, float("nan"))
  return out


def epi_mutation_applies(c, kind):
  if kind.startswith("geglu") and c.act != "geglu":
    return False
  if kind == "geglu_gate_bias_missing":
    return bool(c.bias)
  if kind == "geglu_gate_addend_missing":
    return bool(c.addend)
  if kind in ("act_before_bias", "bias_column"):
    return bool(c.bias or c.addend)
  if kind == "residual_inside_act":
    return bool(c.res)
  if kind == "stored_width":
    return c.act == "geglu" and c.N > tile_of(FORMS[c.form]).bn
  return True


def ceiling(c, d, ref=None):
  """[Bt, M, nout]: the derived bound of |out - reference_act| per element (module docstring).  `ref`: a mutated
  reference to build the bound around instead (the failure report)."""
  ref = reference_act(c, d) if ref is None else torch.nan_to_num(ref, nan=0.0)
  if c.act == "geglu":
    ce = reference_pre(c, d)[..., geglu_cols(c)[0]].abs() * CEIL_F32 + 2.0 ** -23 * ref.abs()
  else:
    ce = torch.full_like(ref, CEIL_F32)
  return ce + 2.0 ** -8 * ref.abs() if c.odt == BF else ce


def oracle_act(c, d, O):
  """The same epilogue by oracle.ldm_oracle's gelu / silu in float32 on the exact z, rounded to the output type."""
  z = reference_pre(c, d).to(F32)
  if c.act == "geglu":
    nv, ng = geglu_cols(c)
    out = z[..., nv] * O.gelu(z[..., ng])
  else:
    out = O.gelu(z) if c.act == "gelu" else O.silu(z)
  if c.res:
    out = out + d["res"][:, :nout_of(c)].to(F32)
  return out.to(c.odt).to(F64)


def uniformity_groups(c, d):
  """[Bt * M * nout] int64: outputs with the same number share (z, residual), for GEGLU (value, gate, residual)."""
  z = reference_pre(c, d)
  if c.act == "geglu":
    nv, ng = geglu_cols(c)
    keys = [z[..., nv], z[..., ng]]
  else:
    keys = [z]
  keys.append(d["res"][:, :nout_of(c)].expand_as(keys[0]) if c.res else torch.zeros_like(keys[0]))
  flat = torch.stack([k.reshape(-1) for k in keys], 1)
  return torch.unique(flat, dim=0, return_inverse=True)[1]


def not_uniform(got, groups):
  """The number of groups whose members do not all hold the same value (NaN counts as a value of its own)."""
  v = torch.nan_to_num(got.reshape(-1), nan=1e300)
  n = int(groups.max()) + 1
  lo = torch.full((n,), float("inf"), dtype=F64).scatter_reduce(0, groups, v, "amin")
  hi = torch.full((n,), -float("inf"), dtype=F64).scatter_reduce(0, groups, v, "amax")
  return int((lo != hi).sum())


def exceeds(got, ref, ce, factor=1.0):
  """[...] bool: |got - ref| > factor * ceiling, a NaN on one side only counting as an infinite difference."""
  diff = (got - ref).abs()
  diff = torch.where(torch.isnan(got) != torch.isnan(ref), torch.full_like(diff, float("inf")), diff)
  return torch.nan_to_num(diff, nan=0.0) > factor * ce


def matching_mutations(c, d, got):
  """The mutations whose reference `got` meets within the ceiling (the failure report names them)."""
  refs = {k: reference_act(c, d, k) for k in EPI_MUTATIONS if epi_mutation_applies(c, k)}
  return [k for k, r in refs.items() if not bool(exceeds(got, r, ceiling(c, d, r)).any())]


def epi_id(c):
  base = case_id(c._replace(tag="", off8=0, ldc_x=0, defer=0, split=1) if c.tag else c)       # the tag names the store path
  return base + f"-{c.act}" + (f"-{c.tag}" if c.tag else "") + ("-ln" if c.lnf else "") + ("-rej" if c.rej else "")


def epi_group(c):
  """The case without its store path: the float32 outputs of one group's paths are compared with each other."""
  return c._replace(off8=0, ldc_x=0, boff=0, split=1, defer=0, rej="", tag="")


_EPI_TILES = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 17, 18, 19)
_GEGLU_TILES = (0, 1, 2, 5, 11, 12, 19)
_EPI_TERMS = ((1, 0, 0), (1, 1, 0), (1, 0, 1))                                # (bias, addend, residual)
_EPI_COMBOS = [(mi, ni, term, oi) for mi in (0, 1) for ni in (0, 1) for term in (0, 1, 2) for oi in (0, 1)]
# store paths, in two groups that each share one (M, N, terms, output type): vector epilogue / generic / vector reduce
# and generic (pitch) / generic (bias) / scalar reduce
_EPI_PATHS = ((("vec", {}), ("off8", dict(off8=1)), ("sk2", dict(split=2))),
              (("ldc4", dict(ldc_x=4)), ("boff", dict(boff=1)), ("sk2off8", dict(split=2, off8=1))))


def _forms_of(tiles):
  return [n for t in tiles for n in ((f"t{t}-bf16",) if TILES.get(t, AUTO_NOMINAL).bf16_only else (f"t{t}-bf16", f"t{t}-f32"))]


def _epi_cases():
  out, gi = [], 0
  for act, tiles in (("gelu", _EPI_TILES), ("silu", _EPI_TILES), ("geglu", _GEGLU_TILES)):
    wide = 64 if act == "geglu" else 8
    for name in _forms_of(tiles):
      f = FORMS[name]
      t, bke = tile_of(f), bke_of(f)
      for paths in _EPI_PATHS:
        mi, ni, term, oi = _EPI_COMBOS[(7 * gi) % len(_EPI_COMBOS)]
        gi += 1
        b, a, r = _EPI_TERMS[term if act != "geglu" else (0, 2)[term % 2]]     # GEGLU takes no addend
        M = (1, t.bm + 1)[mi]
        kw = dict(M=M, N=(wide, t.bn + wide)[ni], K=2 * bke, bias=b, addend=a, add_rows=37 if a and M > 37 else 0, res=r,
                  ldr_x=8 * r, odt=F32 if f.dt == F32 or oi else BF, act=act)
        for tag, pkw in paths:
          if pkw.get("split") and not f.tile:
            continue                                                          # the cost model's pick: no forced split
          rej = ALIGN_REJ if act == "geglu" and f.tile in (11, 12) and not pkw.get("split") and tag != "vec" else ""
          out.append(_mk(name, tag=tag, rej=rej, **kw, **pkw))
      if act == "geglu":                                                      # finding 2: rejected on every path
        kw = dict(M=t.bm + 1, N=t.bn + 64, K=2 * bke, bias=1, addend=1, add_rows=37, act=act, rej=ADDEND_REJ)
        out.append(_mk(name, tag="vec", **kw))
        if f.tile == 2:
          out += [_mk(name, tag="off8", off8=1, **kw), _mk(name, tag="sk2", split=2, **kw),
                  _mk(name, tag="defer", split=2, defer=1, **kw)]
  # the deferred reduce, then ops.finish
  for act in ("gelu", "silu", "geglu"):
    for name in ("t2-bf16", "t2-f32", "t11-bf16"):
      t, bke = tile_of(FORMS[name]), bke_of(FORMS[name])
      out.append(_mk(name, tag="defer", M=t.bm + 1, N=t.bn + (64 if act == "geglu" else 8), K=2 * bke, bias=1, res=1, ldr_x=8,
                     split=2, defer=1, act=act))
  # the transposed store (GemmParams built by the test): one 32x32 tile, one 16x16x32 tile
  for name, act, M in (("t2-bf16", "gelu", 129), ("t2-f32", "silu", 129), ("t11-bf16", "gelu", 257), ("t11-bf16", "silu", 131)):
    t, bke = tile_of(FORMS[name]), bke_of(FORMS[name])
    out.append(_mk(name, "tstore", M=M, N=t.bn + 8, K=2 * bke, bias=1, act=act))
  # one 3x3 convolution with SiLU
  for name in ("t2-bf16", "t11-bf16"):
    out.append(_mk(name, "conv", B=1, H=3, W=5, Cin=64, N=136, bias=1, res=1, act="silu"))
  # the persistent tiles: bias + activation only (the kernels that are built), both deals
  i = 0
  for tile, acts in ((13, ("gelu", "silu")), (14, ("gelu", "silu", "geglu"))):
    for deal in ("wg1", "deal"):
      name = f"t{tile}-bf16-{deal}"
      f = FORMS[name]
      for act in acts:
        out.append(_mk(name, M=(1, 257)[i % 2], N=TILES[tile].bn * (1 + (i // 2) % 2), K=128, bias=1, split=f.wg, act=act))
        i += 1
      if tile == 14:
        out.append(_mk(name, M=(257, 1)[i % 2], N=256, K=128, bias=1, split=f.wg, act="geglu", lnf=1))
  # rejections that launch nothing
  out.append(_mk("t13-bf16-deal", M=33, N=160, K=128, act="gelu", rej="no kernel for this epilogue"))
  out.append(_mk("t14-bf16-wg1", M=33, N=128, K=128, split=-1, act="silu", rej="no kernel for this epilogue"))
  out.append(_mk("t14-bf16-deal", "conv", B=1, H=3, W=5, Cin=64, N=128, bias=1, act="silu", rej="no kernel for this epilogue"))
  out.append(_mk("t3-bf16", M=33, N=64, K=128, bias=1, act="geglu", rej="GEGLU needs a tile"))
  out.append(_mk("t9-bf16", M=33, N=320, K=128, bias=1, act="geglu", rej="GEGLU needs a tile"))
  return out


_EPI = None


def epilogue_cases():
  global _EPI
  if _EPI is None:
    _EPI = _epi_cases()
    ids = [epi_id(c) for c in _EPI]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:4]
  return _EPI
