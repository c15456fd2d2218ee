"""Exact probes for the attention kernels: builders, the float64 reference, the gates (a plain module, imported by
test_attention_probes_cpu.py and test_attention_accounting_gpu.py).

A tolerance test on random data cannot see ONE lost key or ONE misplaced query row in a bf16 attention: the output
is a softmax average, so a single key moves it by |v| / Tk, far inside any bf16 tolerance, and one wrong row is
diluted by sqrt(rows) in a whole-tensor norm.  The probes below have outputs that are known exactly, so such an error
is O(1):

  probe 1, key census      q = 0: every valid key weighs exactly 1 / Tk and P = exp2(0) = 1 is exact.
                           V[b, k, h, d] = 1 if (k + h + b) % S == d else 0, so out[d] = count_d / Tk.  K is random
                           (it must not matter).  Gate: 1 bf16 ulp (norm_check.bf16_ulp) or 4 * 2^-24 relative
                           (float32: the reciprocal and the product) of count_d / Tk; an exact 0 must be 0.
  probe 2, key selection   k_j = c_j in {+-1}^S, q_i = beta * c_pi(i): the softmax is one-hot (>= 1 - 1e-9 on key
                           pi(i), shown by the CPU test), so out[i] = V[pi(i)].  pi is affine per (batch, head) with
                           rows 0, 31, 32, Tq - 1 pinned to keys 0, KT - 1, KT, Tk - 1.  Gate: 1 bf16 ulp, or
                           8 * 2^-24 * max(|ref|, 2^-6) in float32.
  probe 3, powers of two   (matrix-side-softmax layout only) integer logits in the exp2 domain on two levels
                           L0 + {0..3} and L0 + 9 + {0..2}, L0 in {-20, 0, +20} per row, V integer in [-4, 4]:
                           numerator and denominator are exact in float32 in any order.  Gate: 1 bf16 ulp.
  probe 4, random data     |got - ref| <= u (c absref + |ref|) + tiny per element, u = 2^-9 (bf16) / 2^-24 (float32),
                           absref = P |V|; variants: plain, a late dominating key, the +-40 logit offset.

Measured on the CPU over every shape of the matrix below (test_attention_probes_cpu.py measures them again and asserts
that the recorded figures still cover what it finds):
  probe 2, float32: the oracle's float32 attention (oracle/ldm_oracle.py multihead_attention, unit projections) is
    within ORACLE_SELECT_F32 = 0.002 x 2^-24 max(|ref|, 2^-6) of float64 on the probe's inputs (a one-hot row is
    reproduced exactly, what is left is the leak), far below half of the factor 8, which therefore stays.
  probe 4, bf16: float64 attention with P and the output rounded to bf16 (P in the numerator only, as the lane-side
    softmax does, or in the denominator too, as the matrix-side softmax does) needs c = 2.18 in every variant (u = 2^-9
    is half of bf16's largest relative rounding error, so the rounding of P alone takes c = 2): c = 4 x 2.18 = 8.72.
  probe 4, float32: the oracle's float32 attention needs c = 19.5 (plain), 50.4 (late dominating key) and 282 (the
    +-40 offset: logits of several hundred, each carrying |logit| 2^-24 of rounding into the exponent), so
    c = 78, 201.6 and 1128.
Largest figures the kernels reach on an MI355X, in units of each gate (<= 1 passes; also DESIGN.md section 2):
  form                 census  selection  pow2   bound (probe 4, worst variant)
  attn_kernel float32  0.24    0.24       -      0.27   (Sp = 32 .. 160)
  attn_kernel bf16     0.49    0          -      0.32
  8-wave, PF = 2       0.49    0          -      0.31
  matrix softmax 4 / 8 0.49    0          0.50   0.33 / 0.33
  wide float32 / bf16  0.19 / 0.44  0     -      0.19 / 0.30
  ldm_st_xtail         0.22    0          0.50   0.30
  ldm_st_block         0.22 (plain and CFG pair)
Every form passed when first run; no kernel was changed.
"""
import math
from collections import namedtuple

import torch

from norm_check import bf16_ulp

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
LN2 = math.log(2.0)
MS_DIM = 40                    # layout.MS_DIM (asserted equal by the GPU test)

# probe 4: the largest c a reference computation needs (docstring), per storage type and variant; the gate uses 4 x
MODEL_C = {(BF, "plain"): 2.18, (BF, "spike"): 2.18, (BF, "offset+40"): 2.18, (BF, "offset-40"): 2.18,
           (F32, "plain"): 19.5, (F32, "spike"): 50.4, (F32, "offset+40"): 282.0, (F32, "offset-40"): 282.0}
ORACLE_SELECT_F32 = 0.002


def c_of(dtype, variant):
  return max(2.0, 4.0 * MODEL_C[(dtype, variant)])


SELECT_F32_FACTOR = 8.0
TINY = 2.0 ** -126

# name, kind (plain | ms | wide | xtail), dtype, S (head size), Sp (padded), Q (queries per workgroup), KT (keys per
# tile), pf2 (two tiles in flight)
Form = namedtuple("Form", "name kind dtype S Sp Q KT pf2")

_HEADS = ((32, 32), (48, 40), (64, 64), (80, 80), (96, 88), (160, 160))


def _forms():
  out = []
  for sp, s in _HEADS:
    out.append(Form(f"attn{sp}-f32", "plain", F32, s, sp, 128, 64 if sp == 32 else 32, False))
    out.append(Form(f"attn{sp}-bf16", "plain", BF, s, sp, 128, 128 if sp == 32 else 64, False))
  out.append(Form("attn48x8-bf16", "plain", BF, 40, 48, 256, 64, True))
  out.append(Form("ms4-bf16", "ms", BF, 40, 48, 128, 64, False))
  out.append(Form("ms8-bf16", "ms", BF, 40, 48, 256, 64, True))
  out.append(Form("wide-f32", "wide", F32, 512, 512, 32, 32, False))
  out.append(Form("wide-bf16", "wide", BF, 512, 512, 32, 32, False))
  out.append(Form("xtail-bf16", "xtail", BF, 40, 48, 128, 80, False))
  return out


FORMS = {f.name: f for f in _forms()}

# one case of the matrix: sizes, batch, heads and the operand layout
Case = namedtuple("Case", "form Tq Tk R H ldvt_extra shared_qk out_wide")


def roundup8(n):
  return (n + 7) // 8 * 8


def beta_of(S):
  return 16.0 if S <= 48 else 8.0 if S <= 160 else 4.0


def _switches(form):
  """bf16 Sp = 48: the dispatch sends Tq >= 256 to the 8-wave kernels."""
  return form.dtype == BF and form.Sp == 48 and form.kind in ("plain", "ms")


def tq_values(form):
  Q = form.Q
  if form.kind == "xtail":
    return [128, 384]
  if _switches(form) and Q == 128:
    return [1, 31, 33, Q - 1, Q, Q + 1, 255]          # 2Q + 5 = 261 belongs to the 8-wave row
  if _switches(form):
    return [Q, Q + 1, Q + 31, Q + 33, 2 * Q - 1, 2 * Q + 5]   # 1, 31, 33, Q - 1 belong to the 4-wave row
  return [1, 31, 33, Q - 1, Q, Q + 1, 2 * Q + 5]


def tk_values(form):
  KT = form.KT
  if form.kind == "xtail":
    return [1, 5, 16, 17, 64, 77, 80]
  v = {1, 7, 8, 9, KT - 1, KT, KT + 1, 2 * KT, 2 * KT + 1, 3 * KT - 7, 77}
  if form.pf2:
    v |= {3 * KT, 4 * KT}                              # 1, 2, 3, 4 key tiles end the two-buffer loop differently
  return sorted(v)


def _rh(form, Tq, Tk):
  if form.kind == "wide":
    return 2 + (Tq + Tk) % 2, 1
  if form.kind == "xtail":
    return 2 + (Tq // 128 + Tk) % 2, 8
  heads = (2, 3) if form.S >= 160 else (2, 3, 4, 8)
  return 2 + (Tq + Tk) % 2, heads[(7 * Tq + Tk) % len(heads)]


def cases(form):
  """Every Tq value with two Tk values, every Tk value with two Tq values, the largest of both together, and the
  layout forms: (a) q | k as the column halves of one buffer, (b) out a column slice of a wider buffer, (c) ldvt =
  roundup8(Tk) exactly and + 8 (alternating over the matrix; both in the layout cases)."""
  tqs, tks = tq_values(form), tk_values(form)
  n, m = len(tks), len(tqs)
  pairs = []
  for i, tq in enumerate(tqs):
    pairs += [(tq, tks[(2 * i) % n]), (tq, tks[(2 * i + 1 + n // 2) % n])]
  for j, tk in enumerate(tks):
    pairs += [(tqs[j % m], tk), (tqs[(j + 1 + m // 2) % m], tk)]
  pairs += [(tqs[-1], tks[-1]), (tqs[-1], 77), (tqs[0], tks[-1])]
  for tk in tks:                                         # (the two rules above may have produced the same pair)
    pairs += [(tq, tk) for tq in tqs if len({p[0] for p in pairs if p[1] == tk}) < 2 and (tq, tk) not in pairs][:1]
  for tq in tqs:
    pairs += [(tq, tk) for tk in tks if len({p[1] for p in pairs if p[0] == tq}) < 2 and (tq, tk) not in pairs][:1]
  out, seen = [], set()
  for tq, tk in pairs:
    if (tq, tk) in seen:
      continue
    seen.add((tq, tk))
    r, h = _rh(form, tq, tk)
    out.append(Case(form.name, tq, tk, r, h, 8 * (len(out) % 2), False, False))
  if form.kind == "xtail":
    return out                                           # ldv 80 / 88 alternate; q / ctx / out are contiguous there
  t = form.Q + 33 if form.pf2 else form.Q + 1          # (a) needs Tq = Tk; ragged in both
  if _switches(form) and form.Q == 128:
    t = form.Q - 1 + 64                                  # 191: stays on the 4-wave side
  r, h = _rh(form, t, t)
  out.append(Case(form.name, t, t, r, h, 0, True, True))
  out.append(Case(form.name, t, t, r, h, 8, True, False))
  out.append(Case(form.name, tqs[1], 77, 3, h, 0, False, True))
  return out


def case_id(c):
  lay = ("-qk1" if c.shared_qk else "") + ("-oslice" if c.out_wide else "")
  return f"{c.form}-Tq{c.Tq}-Tk{c.Tk}-R{c.R}H{c.H}-ldvt+{c.ldvt_extra}{lay}"


def all_cases():
  return [c for f in FORMS.values() for c in cases(f)]


# ---- rounding helpers ---------------------------------------------------------------------------------
def rounded(x, dtype):
  """float64 values of x after rounding to the storage type."""
  return x.to(F32).to(dtype).to(F64)


def _gen(*key):
  return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1))


# ---- the float64 reference ----------------------------------------------------------------------------
def attn_ref64(q, k, v, scale, base):
  """q [R, Tq, H, S], k / v [R, Tk, H, S]: the exact values handed to the kernel, as float64.  base = math.e:
  P = softmax(q k^T scale); base = 2: base-2 softmax of q k^T scale (the matrix-side-softmax layout, whose q is already
  in the exp2 domain: scale = 1).  Returns ref = P V and absref = P |V|, both [R, Tq, H, S]."""
  assert q.dtype == k.dtype == v.dtype == F64
  logits = torch.einsum("nqhs,nchs->nhqc", q, k) * scale
  if base == 2:
    logits = logits * LN2
  else:
    assert base == math.e
  p = torch.softmax(logits, dim=3)
  return torch.einsum("nhqc,nchs->nqhs", p, v), torch.einsum("nhqc,nchs->nqhs", p, v.abs())


def selected_weight(q, k, scale, base, pi):
  """The softmax weight each row puts on its selected key pi [R, H, Tq] (probe 2)."""
  logits = torch.einsum("nqhs,nchs->nhqc", q, k) * scale * (LN2 if base == 2 else 1.0)
  return torch.softmax(logits, dim=3).gather(3, pi.unsqueeze(3)).squeeze(3)


def mutated_ref64(q, k, v, scale, base, kind):
  """The reference of a subtly wrong kernel: key Tk - 1 dropped, key 0 counted twice, or two query rows swapped
  (row 0 of the first batch element with row Tq - 1 of the last)."""
  if kind == "drop_last_key":
    if k.shape[1] == 1:
      return torch.full_like(q[..., :v.shape[-1]], float("nan"))       # no key left: 0 / 0
    return attn_ref64(q, k[:, :-1], v[:, :-1], scale, base)[0]
  if kind == "double_key0":
    return attn_ref64(q, torch.cat([k[:, :1], k], 1), torch.cat([v[:, :1], v], 1), scale, base)[0]
  assert kind == "swap_rows"
  ref = attn_ref64(q, k, v, scale, base)[0].clone()
  a, b = ref[0, 0].clone(), ref[-1, -1].clone()
  ref[0, 0], ref[-1, -1] = b, a
  return ref


# ---- gates: each returns the worst element in units of its gate (<= 1 passes; non-finite output -> inf) ----------
def _err(got, ref):
  got = got.detach().cpu().to(F64)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  err = (got - ref).abs()
  return torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))


def _ratio(err, tol):
  r = err / tol
  r = torch.where((err == 0), torch.zeros_like(r), r)
  r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
  return float(r.max()) if r.numel() else 0.0


def census_excess(got, ref, dtype):
  """probe 1: distance from count_d / Tk in bf16 ulp, or in units of 4 * 2^-24 |ref| (float32; 0 must be 0)."""
  err = _err(got, ref)
  tol = bf16_ulp(ref) if dtype == BF else 4 * 2.0 ** -24 * ref.abs()
  return _ratio(err, tol)


def selection_excess(got, ref, dtype):
  """probe 2 (and 3): distance in bf16 ulp, or in units of 8 * 2^-24 max(|ref|, 2^-6) (float32)."""
  err = _err(got, ref)
  tol = bf16_ulp(ref) if dtype == BF else SELECT_F32_FACTOR * 2.0 ** -24 * ref.abs().clamp_min(2.0 ** -6)
  return _ratio(err, tol)


def bound_excess(got, ref, absref, dtype, variant):
  """probe 4: |got - ref| over u (c absref + |ref|) + tiny, c = c_of(dtype, variant)."""
  u = 2.0 ** -9 if dtype == BF else 2.0 ** -24
  c = c_of(dtype, variant)
  return _ratio(_err(got, ref), u * (c * absref + ref.abs()) + TINY)


def c_needed(got, ref, absref, dtype):
  """The smallest c with which `got` meets probe 4's bound (calibration of c from a reference computation)."""
  u = 2.0 ** -9 if dtype == BF else 2.0 ** -24
  need = ((got - ref).abs() - u * ref.abs() - TINY) / (u * absref.clamp_min(1e-300))
  return max(0.0, float(need.max()))


# ---- probe builders: q [R, Tq, H, S], k, v [R, Tk, H, S] float64, exactly representable in the storage type --------
def probe_census(form, c):
  S, g = form.S, _gen(1, form.S, c.Tq, c.Tk, c.R, c.H)
  q = torch.zeros(c.R, c.Tq, c.H, S, dtype=F64)
  k = rounded(torch.randn(c.R, c.Tk, c.H, S, generator=g), form.dtype)
  kk = torch.arange(c.Tk).view(1, c.Tk, 1, 1)
  hh = torch.arange(c.H).view(1, 1, c.H, 1)
  bb = torch.arange(c.R).view(c.R, 1, 1, 1)
  dd = torch.arange(S).view(1, 1, 1, S)
  v = ((kk + hh + bb) % S == dd).to(F64)
  return q, k, v


def census_counts(c, S):
  """count_d [R, H, S] of probe 1, by counting (not through the softmax)."""
  cnt = torch.zeros(c.R, c.H, S, dtype=F64)
  for b in range(c.R):
    for h in range(c.H):
      for key in range(c.Tk):
        cnt[b, h, (key + h + b) % S] += 1
  return cnt


_CODES = {}


def codes(S, Tk):
  """Tk codes in {+-1}^S, drawn with a fixed seed per (S, Tk); a code whose product with an earlier one exceeds
  `max_product(S)` is drawn again (same generator), which keeps the softmax of probe 2 one-hot to 1e-9."""
  key = (S, Tk)
  if key not in _CODES:
    g = _gen(2, S, Tk)
    cds = torch.randint(0, 2, (Tk, S), generator=g).to(F64) * 2 - 1
    lim = max_product(S)
    for _ in range(1000):
      gram = torch.tril(cds @ cds.t(), diagonal=-1)
      bad = (gram > lim).any(dim=1).nonzero().flatten()
      if bad.numel() == 0:
        break
      cds[bad] = torch.randint(0, 2, (bad.numel(), S), generator=g).to(F64) * 2 - 1
    else:
      raise AssertionError(f"no code set for S={S} Tk={Tk}")
    _CODES[key] = cds
  return _CODES[key]


def max_product(S):
  """Largest product of two different codes: the natural-log logit gap beta S^-0.5 (S - product) must be >= 28
  (Tk e^-28 < 1e-9 for Tk <= 1024); in the exp2-domain layout the gap is larger still."""
  return S - math.ceil(28.0 / (beta_of(S) * S ** -0.5))


def selection_map(form, c):
  """pi [R, H, Tq]: (a i + b) mod Tk with a odd and coprime to Tk, different per (batch, head); rows 0, 31, 32, Tq - 1
  hit keys 0, KT - 1, KT, Tk - 1 (clamped to the keys that exist)."""
  i = torch.arange(c.Tq)
  pi = torch.zeros(c.R, c.H, c.Tq, dtype=torch.int64)
  for b in range(c.R):
    for h in range(c.H):
      a = 2 * (3 * b + h) + 3
      while math.gcd(a, c.Tk) != 1:
        a += 2
      pi[b, h] = (a * i + 5 * b + 11 * h + 1) % c.Tk
  for row, key in ((0, 0), (31, form.KT - 1), (32, form.KT), (c.Tq - 1, c.Tk - 1)):
    if row < c.Tq:
      pi[:, :, row] = min(key, c.Tk - 1)
  return pi


def probe_selection(form, c):
  S, g = form.S, _gen(3, form.S, c.Tq, c.Tk, c.R, c.H)
  cds = codes(S, c.Tk)
  pi = selection_map(form, c)
  k = cds.view(1, c.Tk, 1, S).expand(c.R, c.Tk, c.H, S).clone()
  q = (beta_of(S) * cds[pi]).permute(0, 2, 1, 3).contiguous()          # [R, H, Tq, S] -> [R, Tq, H, S]
  v = rounded(torch.randn(c.R, c.Tk, c.H, S, generator=g), form.dtype)
  return q, k, v, pi


P3_COLS, P3_ONE = 16, 16        # level columns 0..15 of k, dim 16 of k holds 1 (q holds L0 there)
P3_L0 = (-20.0, 0.0, 20.0, 0.0)


def probe_pow2(form, c):
  """probe 3.  Column j of k (16 of them) carries a level per key; a row reads ONE column (q = unit vector) plus its
  L0.  Column classes (col % 4): 0: L0 = -20, high keys only in the last key tile; 1: L0 = 0, only in the last tile;
  2: L0 = +20, high keys anywhere; 3: L0 = 0, anywhere.  Returns q, k, v and the integer logits [R, H, Tq, Tk]."""
  assert form.S == 40
  S, g = form.S, _gen(4, c.Tq, c.Tk, c.R, c.H, form.KT)
  last0 = (c.Tk - 1) // form.KT * form.KT
  low = torch.randint(0, 4, (c.R, c.Tk, c.H, P3_COLS), generator=g).to(F64)
  high = 9 + torch.randint(0, 3, (c.R, c.Tk, c.H, P3_COLS), generator=g).to(F64)
  pick = torch.rand(c.R, c.Tk, c.H, P3_COLS, generator=g)
  col = torch.arange(P3_COLS).view(1, 1, 1, P3_COLS)
  key = torch.arange(c.Tk).view(1, c.Tk, 1, 1)
  late = (col % 4) < 2
  is_high = torch.where(late, (key >= last0) & (pick < 0.25), pick < 0.125)
  is_high = is_high | (key == c.Tk - 1 - (col % 3).clamp_max(c.Tk - 1 - last0))      # at least one high key
  k = torch.zeros(c.R, c.Tk, c.H, S, dtype=F64)
  k[..., :P3_COLS] = torch.where(is_high, high, low)
  k[..., P3_ONE] = 1.0
  q = torch.zeros(c.R, c.Tq, c.H, S, dtype=F64)
  i = torch.arange(c.Tq).view(1, c.Tq, 1)
  rc = (i + 3 * torch.arange(c.H).view(1, 1, c.H) + 5 * torch.arange(c.R).view(c.R, 1, 1)) % P3_COLS
  q.scatter_(3, rc.unsqueeze(3), 1.0)
  q[..., P3_ONE] = torch.tensor(P3_L0, dtype=F64)[rc % 4]
  v = torch.randint(-4, 5, (c.R, c.Tk, c.H, S), generator=g).to(F64)
  logits = torch.einsum("nqhs,nchs->nhqc", q, k)
  return q, k, v, logits, rc


P4_VARIANTS = ("plain", "spike", "offset+40", "offset-40")


def probe_random(form, c, variant):
  """probe 4: N(0, 1) data rounded to the storage type; `spike`: key Tk - 3 (last tile) = 6 q[5] for batch 0, head 0;
  `offset+-40`: k + (+-40) mean_rows(q) / 8.  For the matrix-side-softmax layout q is moved to the exp2 domain
  (x S^-0.5 log2 e) and rounded again: the reference sees those values, with base 2 and scale 1."""
  S, g = form.S, _gen(5, form.S, c.Tq, c.Tk, c.R, c.H)
  q = torch.randn(c.R, c.Tq, c.H, S, generator=g)
  k = torch.randn(c.R, c.Tk, c.H, S, generator=g)
  v = torch.randn(c.R, c.Tk, c.H, S, generator=g)
  if variant == "spike":
    k[0, max(c.Tk - 3, 0), 0] = q[0, min(5, c.Tq - 1), 0] * 6.0
  elif variant.startswith("offset"):
    k = k + float(variant[6:]) * q.mean(dim=1, keepdim=True) / 8.0
  else:
    assert variant == "plain"
  q, k, v = rounded(q, form.dtype), rounded(k, form.dtype), rounded(v, form.dtype)
  if form.kind in ("ms", "xtail"):
    q = rounded(q * (S ** -0.5 / LN2), form.dtype)
  return q, k, v


def scale_base(form, probe):
  """(scale, base) the reference uses.  Matrix-side-softmax layout: the logits are q k^T, base 2."""
  if form.kind in ("ms", "xtail"):
    return 1.0, 2
  return form.S ** -0.5, math.e


# ---- reference computations that fix c (probe 4) ----------------------------------------------------------
def bf16_model(q, k, v, scale, base, round_denominator):
  """float64 attention with P (relative to the row maximum) and the output rounded to bf16."""
  logits = torch.einsum("nqhs,nchs->nhqc", q, k) * scale * (LN2 if base == 2 else 1.0)
  p = torch.exp(logits - logits.max(dim=3, keepdim=True).values)
  pb = rounded(p, BF)
  den = (pb if round_denominator else p).sum(dim=3)
  out = torch.einsum("nhqc,nchs->nqhs", pb, v) / den.permute(0, 2, 1).unsqueeze(3)
  return rounded(out, BF)


def oracle_f32(q, k, v):
  """The oracle's float32 attention (oracle/ldm_oracle.py multihead_attention) on float32 operands.  Its key and value
  projections read one context tensor, so the context is (k | v) and the two kernels are the unit matrices that pick
  the halves (exact in float32); the query and output projections are unit matrices."""
  from oracle import ldm_oracle as O
  R, Tq, H, S = q.shape
  D = H * S
  eye, zero = torch.eye(D, dtype=F32), torch.zeros(D, D, dtype=F32)
  w = {"query/kernel": eye.view(D, H, S), "key/kernel": torch.cat([eye, zero], 0).view(2 * D, H, S),
       "value/kernel": torch.cat([zero, eye], 0).view(2 * D, H, S), "output/kernel": eye.view(H, S, D),
       "output/bias": torch.zeros(D)}
  ctx = torch.cat([k.to(F32).reshape(R, -1, D), v.to(F32).reshape(R, -1, D)], 2)
  out = O.multihead_attention(q.to(F32).reshape(R, Tq, D), ctx, w.__getitem__, S)
  return out.reshape(R, Tq, H, S).to(F64)


# ---- device layouts -------------------------------------------------------------------------------------
def pack(form, c, q, k, v, device):
  """The operands as ops.attention takes them: q [R, Tq, H Sp], k [R, Tk, H Sp], vt [R, H Sp, ldvt], out like q, all
  views of NaN-filled buffers with distinct batch strides (a NaN pad row per batch element), V^T columns [Tk, ldvt)
  NaN, out NaN.  shared_qk: q and k are the column halves of one [R, T, 2 H Sp] buffer; out_wide: out is columns
  [8, 8 + H Sp) of a [R, Tq, H Sp + 16] buffer.  Matrix-side-softmax layout: k[..., 40] = 1 and V^T row 40 = 1 per
  head.  Returns (q, k, vt, out, out_base)."""
  dt, S, Sp, W = form.dtype, form.S, form.Sp, c.H * form.Sp
  nan = float("nan")
  ms = form.kind in ("ms", "xtail")

  def padded(x, T):
    y = torch.zeros(c.R, T, c.H, Sp, dtype=F64)
    y[..., :S] = x
    return y

  qd, kd, vd = padded(q, c.Tq), padded(k, c.Tk), padded(v, c.Tk)
  if ms:
    kd[..., MS_DIM] = 1.0
    vd[..., MS_DIM] = 1.0
  if c.shared_qk:
    assert c.Tq == c.Tk
    base = torch.full((c.R, c.Tq + 1, 2 * W), nan, dtype=F64)
    base[:, :c.Tq, :W] = qd.reshape(c.R, c.Tq, W)
    base[:, :c.Tq, W:] = kd.reshape(c.R, c.Tk, W)
    base = base.to(dt).to(device)
    qv, kv = base[:, :c.Tq, :W], base[:, :c.Tk, W:]
  else:
    qb = torch.full((c.R, c.Tq + 1, W), nan, dtype=F64)
    qb[:, :c.Tq] = qd.reshape(c.R, c.Tq, W)
    kb = torch.full((c.R, c.Tk + 2, W), nan, dtype=F64)
    kb[:, :c.Tk] = kd.reshape(c.R, c.Tk, W)
    qv, kv = qb.to(dt).to(device)[:, :c.Tq], kb.to(dt).to(device)[:, :c.Tk]
  ldvt = (80 if form.kind == "xtail" else roundup8(c.Tk)) + c.ldvt_extra     # ldm_st_xtail: rows of >= 80
  vt = torch.full((c.R, W, ldvt), nan, dtype=F64)
  vt[:, :, :c.Tk] = vd.reshape(c.R, c.Tk, W).permute(0, 2, 1)
  vt = vt.to(dt).to(device)
  if c.out_wide:
    ob = torch.full((c.R, c.Tq, W + 16), nan, dtype=dt, device=device)
    out = ob[:, :, 8:8 + W]
  else:
    ob = torch.full((c.R, c.Tq, W), nan, dtype=dt, device=device)
    out = ob
  return qv, kv, vt, out, ob


def unpack(form, c, out, out_base):
  """(values [R, Tq, H, S] float64, padded dims [R, Tq, H, Sp - S], the untouched columns of a wider out buffer)."""
  o = out.detach().cpu().to(F64).reshape(c.R, c.Tq, c.H, form.Sp)
  W = c.H * form.Sp
  rest = torch.cat([out_base[:, :, :8], out_base[:, :, 8 + W:]], 2).detach().cpu().to(F64) if c.out_wide else None
  return o[..., :form.S], o[..., form.S:], rest
