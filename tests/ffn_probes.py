"""Exact probes for the row-panel kernels of csrc/ffn.hip (ldm_ffn_geglu, ldm_st_tail, ldm_st_xtail, ldm_st_block):
builders, an independent float64 reference, the gates, the mutation list and the case matrix (a plain module, imported
by test_ffn_probes_cpu.py and test_ffn_accounting_gpu.py).

A whole-tensor norm cannot see one wrong row among M, one lost hidden unit of 1280 or a bias shifted by four columns.
Each probe below isolates ONE phase of the chain

  [FRONT] h1 = r0 + bo1 + Wo1 att            q = Wq' LayerNorm(h1) + qb
  [XATT ] att2 = softmax2(q K^T) V           (exp2 domain, <= 80 keys of the panel's sample)
  [PRE ]  h = res + bo + Wo att2             (res = h1 or r0)
          y = h + b2 + W2 (a gelu(g)),  (a | g) = W1 LayerNorm(h) + b1
  [POST]  out = r1 + bp + Wp y

by making every other phase an exact identity or an exact zero (w1 = 0 closes the feed-forward: the GEGLU is then the
constant b'_val gelu(b'_gate); V = 0 closes an attention; Wp = I and Wo = the head selector pass rows through):

  probe 1  o-projection (Wo of tail / xtail, Wo1 of st_block): one-hot selection in 2 phases over the 384 K columns and
           a census (att in {+-1, +-2}, wo in {0, +-1}); bo, b2, bp, r0, r1 integers in [-8, 8].  Exact.  In ldm_st_xtail
           the rows of att are the attention's output: q = 0 and V constant over the keys of a sample, so att is that
           constant (Tk v rcp(Tk) rounds back to the integer v in bf16) -- per sample, not per row.
           ldm_st_block's second o-projection gets the same census (`census2`).
  probe 2  proj_out over y = h + b2: Wp a permutation, then a census.  Exact.
  probe 3  every hidden unit: w1 = 0, val_j an integer, gate_j in {0, 8} (gelu_erf_f(8) == 8 in float32, shown by the
           CPU test on a float32 transcription), w2 one-hot in 4 phases + a census with val_j = +-1/8.  Exact.
  probe 4  first product through the LayerNorm fold: every row of h is a signed rotation of one multiset (160 x 1,
           96 x 2, 64 x 3, half of each negative: sum 0, sum of squares 1120, variance 3.5) and eps = 12.5, so
           var + eps = 16 and rstd = 1/4; value rows of w1 hold ten non-zero integers per row, each K column exactly
           once per 32 hidden units, with column sums (p4_cs) distinct inside a 64-unit chunk and against the chunk
           before; the gate is held open at 8 by the bias, so hidden = 2 acc + 8 b, an integer that the hidden tile's
           bf16 rounding lands on.  Second variant: + (1 or 2) on every element of a row (rows r and r ^ 16 differ), so
           nm * cs matters.  Observed through probe 3's one-hot w2.  Gate: 1 bf16 ulp (the reference itself is exact).
  probe 6  GEGLU transfer curve: w1 = 0, val_j = 1, gate_j a grid of 1280 points over [-20, 20] (dense in [-6, 0], +-0,
           the bf16 neighbours of 0, beyond the exp2 underflow).  Gate: |got - gelu(g)| <= 1 bf16 ulp (true ulp, not
           clamped) + A |g|; finite everywhere; g >= 15 must return bf16(g) exactly.
  probe 7  the full chain on small random integers with real LayerNorms and attentions:
           |got - ref| <= 2^-9 (c absref + |ref|), absref = |r1| + |bp| + |Wp| |y|.

  probe 5  ldm_st_block's query projection through unit-vector keys (probe5's docstring); h1 >= 0 and V >= 0, so
           h1 + att2 never cancels.  Gate: 1 bf16 ulp of the reference.

Views: ops.st_xtail / ops.st_block require contiguous q / att, so the padded row pitch of the input rows is exercised
on ldm_ffn_geglu (x) and ldm_st_tail (att) only; r0, r1 and out are padded on every entry point.

Measured on the CPU (test_ffn_probes_cpu.py measures again and asserts the recorded figures still cover them):
  GELU_A     = 4 x 7.0e-8: the float64 evaluation of gelu_erf_f's Abramowitz-Stegun formula is within 6.97e-8 |g| of
               the exact-erf GELU on the probe's grid (the documented 1.5e-7 on erf, halved by the 0.5
               of the GELU); x 4 for the hardware rcp / exp2.
  MODEL_C    = per entry point the largest c that the float64 chain with the kernel's documented bf16 rounding points
               (h1, q, P, att2, h, hidden, y, out) needs against the unrounded chain on probe 7's data; the gate uses 4 x.
RESULTS (MI355X, largest figure per form in units of each gate, <= 1 passes; probes 1 - 3 pass only at 0):
  form                          p1  p2  p3  p4  p5    p6    p7
  ldm_ffn_geglu                 -   -   0   0   -     0.50  0.48
  ldm_st_tail                   0   0   0   0   -     0.50  0.33
  ldm_st_xtail                  0   0   0   0   -     0.50  0.38
  ldm_st_block, 64-row, plain   0   0   0   0   1.00  0.50  0.25
  ldm_st_block, 64-row, pair    0   0   0   0   1.00  0.50  0.41
  ldm_st_block, 128-row, plain  0   .   0   .   1.00  .     0.44     (. = not run at M = 24576)
  ldm_st_block, 128-row, pair   0
  Probe 4 is met with equality, not only within its ulp.  Probe 5 sits on its gate: a few elements per thousand are
  exactly one bf16 ulp of att2 from the reference (the reciprocal of the row sum where att2 lies next to a rounding tie),
  none more.  Every form passed unchanged: no kernel was changed.
"""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
C, K0, H, S, SP, HID, MS_DIM = 320, 384, 8, 40, 48, 1280, 40
SWITCH_PANELS = 192            # ldm_st_block: 128-row panels from this many on (cross-checked against ffn.hip's text)
GELU_G = 8.0                   # an open gate: gelu_erf_f(8) == 8
GELU_A_MODEL = 7.0e-8          # docstring
GELU_A = 4.0 * GELU_A_MODEL
MODEL_C = {"ffn": 0.66, "tail": 0.55, "xtail": 0.83, "block": 1.03}
TINY = 2.0 ** -126

Case = namedtuple("Case", "entry M R T Tk ldv in_rows")


def cases():
  out = [Case(e, M, 0, 0, 0, 0, M) for e in ("ffn", "tail") for M in (1, 200, 256)]
  out += [Case("xtail", R * T, R, T, Tk, ldv, R * T) for R, T, Tk, ldv in ((2, 128, 77, 80), (1, 256, 80, 80), (3, 128, 5, 88))]
  out += [Case("block", R * T, R, T, 77, 80, R * T) for R, T in ((2, 128), (1, 256), (3, 128))]
  out += [Case("block", R * T, R, T, 77, 80, R * T // 2) for R, T in ((2, 128), (4, 128))]
  return out


def big_cases():
  """The 128-row form of ldm_st_block: the smallest M the dispatch sends there, plain and as a pair."""
  M = SWITCH_PANELS * 128
  return [Case("block", M, M // 128, 128, 77, 80, M), Case("block", M, M // 128, 128, 77, 80, M // 2)]


BIG_PROBES = {False: ("p1", "p3", "p5", "p7"), True: ("p1",)}      # by pair: five launches' worth of probes, first tag each


def case_id(c):
  s = f"{c.entry}-M{c.M}"
  if c.R:
    s += f"-R{c.R}T{c.T}Tk{c.Tk}ldv{c.ldv}"
  return s + ("-pair" if c.in_rows != c.M else "")


def probes_of(c):
  if c.entry == "ffn":
    return ("p3", "p4", "p6", "p7")
  return ("p1", "p2", "p3", "p4") + (("p5",) if c.entry == "block" else ()) + ("p6", "p7")


def _gen(*key):
  return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1))


def rb(x):
  """float64 values after rounding to bf16 (through float32, as the kernels do)."""
  return x.to(F32).to(BF).to(F64)


def _ulp(ref, floor):
  """2^(floor(log2 a) - 7), a = max(|ref|, floor), from the exponent bits: exact on any device (torch.ldexp goes through
  pow(2, e), which a GPU may round; a gate of exactly one ulp must not depend on that)."""
  a = ref.abs().clamp_min(floor).contiguous()
  return (a.view(torch.int64) & 0x7FF0000000000000).view(F64) * 2.0 ** -7


def bf16_ulp(ref):
  """norm_check.bf16_ulp (one bf16 ulp at max(|ref|, 2^-6)), bit-exact on the device too; the CPU test asserts that the
  two agree."""
  return _ulp(ref, 2.0 ** -6)


def true_ulp(ref):
  """One bf16 ulp at |ref| itself (no floor but the smallest normal number)."""
  return _ulp(ref, TINY)


# ---- operands -------------------------------------------------------------------------------------------------
def selector():
  wo = torch.zeros(C, K0, dtype=F64)
  for h in range(H):
    for s in range(S):
      wo[S * h + s, SP * h + s] = 1.0
  return wo


def neutral(c):
  """Operands (float64, reference layouts: weights [out, in], w1 rows = value | gate) with which every phase is an
  identity or a zero: out = r1 + bp + r0 + ... = 0."""
  z = lambda *sh: torch.zeros(*sh, dtype=F64)
  P = SimpleNamespace(case=c, eps=1e-5)
  P.x = z(c.in_rows, C if c.entry == "ffn" else K0)
  P.r0, P.r1 = z(c.in_rows, C), z(c.in_rows, C)
  P.wo1, P.bo1, P.wq, P.qb = z(C, K0), z(C), z(K0, C), z(K0)
  P.k, P.v = z(max(c.R, 1), max(c.Tk, 1), H, S), z(max(c.R, 1), max(c.Tk, 1), H, S)
  P.wo, P.bo = selector(), z(C)
  P.w1, P.b1, P.w2, P.b2 = z(2 * HID, C), z(2 * HID), z(C, HID), z(C)
  P.wp, P.bp = torch.eye(C, dtype=F64), z(C)
  P.gsel = None
  return P


TENSORS = ("x", "r0", "r1", "wo1", "bo1", "wq", "qb", "k", "v", "wo", "bo", "w1", "b1", "w2", "b2", "wp", "bp", "gsel")


def to_device(P, device):
  Q = SimpleNamespace(**vars(P))
  for n in TENSORS:
    t = getattr(P, n)
    if t is not None:
      setattr(Q, n, t.to(device))
  return Q


def rowcol(rows, cols, seed):
  """Integers in [-8, 8] that differ between neighbours at +-1 row, +-8 and +-64 columns (steps 5 / 7, 14, 4 mod 17)."""
  m, n = torch.arange(rows).view(-1, 1), torch.arange(cols).view(1, -1)
  return (((5 * m + 3 * n + 7 * (n // 8) + 11 * (n // 64) + 2 * (m // 16) + seed) % 17) - 8).to(F64)


def vec(n, seed):
  """Integers in [-8, 8]; v[i] != v[i + 4] everywhere (28 mod 17 != 0)."""
  return (((7 * torch.arange(n) + seed) % 17) - 8).to(F64)


def _ri(g, lo, hi, *shape):
  return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _pm(g, *shape):
  """random in {+-1, +-2}"""
  return (_ri(g, 1, 2, *shape)) * (2 * _ri(g, 0, 1, *shape) - 1)


def _revive(W):
  """Census weights [N, K]: where chance left a K column without a non-zero weight in one of the 64-column wave-tile
  regions, give it one."""
  for n0 in range(0, W.shape[0], 64):
    dead = torch.nonzero((W[n0:n0 + 64] != 0).sum(0) == 0).view(-1)
    W[n0 + dead % min(64, W.shape[0] - n0), dead] = 1.0
  return W


def _set_h(P, h, c):
  """Make the feed-forward's input rows h: directly (ffn) or through r0 with everything in front of it closed."""
  if c.entry == "ffn":
    P.x = h
  else:
    P.r0 = h


def _w2_onehot(ph):
  w2 = torch.zeros(C, HID, dtype=F64)
  j = (3 * torch.arange(C) + 7) % C + C * ph
  w2[torch.arange(C), j] = 1.0
  return w2, j


def probe1(c):
  out = []
  for tag in ("sel0", "sel1", "census"):
    P, g = neutral(c), _gen(11, c.M, c.Tk, len(tag) + ord(tag[-1]))
    n = torch.arange(C)
    if tag == "census":
      W = _revive(_ri(g, -1, 1, C, K0))
    else:
      W = torch.zeros(C, K0, dtype=F64)
      W[n, (7 * (n + C * int(tag[-1])) + 3) % K0] = 1.0
    code = _pm(g, c.in_rows, K0) if tag == "census" else rowcol(c.in_rows, K0, 3)
    if c.entry == "tail":
      P.x, P.wo, P.bo = code, W, vec(C, 1)
    elif c.entry == "xtail":
      cv = _pm(g, c.R, 1, H, S) if tag == "census" else _ri(g, -4, 4, c.R, 1, H, S)
      P.v = cv.expand(c.R, c.Tk, H, S).clone()
      P.k = _ri(g, -2, 2, c.R, c.Tk, H, S)          # q = 0: the keys must not matter
      P.wo, P.bo = W, vec(C, 1)
    else:
      P.x, P.wo1, P.bo1, P.bo = code, W, vec(C, 1), vec(C, 9)
      P.k = _ri(g, -2, 2, c.R, c.Tk, H, S)
    P.r0, P.r1 = rowcol(c.in_rows, C, 0), rowcol(c.in_rows, C, 6)
    P.b2, P.bp = vec(C, 4), vec(C, 12)
    out.append((tag, P, "exact"))
  if c.entry == "block":        # the second o-projection, fed as in ldm_st_xtail: q = 0, V constant over a sample's keys
    P, g = neutral(c), _gen(11, c.M, c.Tk, 2)
    P.v = _pm(g, c.R, 1, H, S).expand(c.R, c.Tk, H, S).clone()
    P.k = _ri(g, -2, 2, c.R, c.Tk, H, S)
    P.wo, P.bo, P.bo1 = _revive(_ri(g, -1, 1, C, K0)), vec(C, 1), vec(C, 9)
    P.r0, P.r1 = rowcol(c.in_rows, C, 0), rowcol(c.in_rows, C, 6)
    P.b2, P.bp = vec(C, 4), vec(C, 12)
    out.append(("census2", P, "exact"))
  return out


def probe2(c):
  out = []
  for tag in ("sel", "census"):
    P, g = neutral(c), _gen(12, c.M, len(tag))
    n = torch.arange(C)
    if tag == "sel":
      P.wp = torch.zeros(C, C, dtype=F64)
      P.wp[n, (7 * n + 3) % C] = 1.0
      P.r0, P.bo, P.b2 = rowcol(c.in_rows, C, 0), vec(C, 1), vec(C, 4)
      if c.entry == "block":
        P.bo1 = vec(C, 9)
    else:
      P.wp = _revive(_ri(g, -1, 1, C, C))
      P.r0 = (rowcol(c.in_rows, C, 0) + 8) % 5 - 2
      P.b2 = (vec(C, 4) + 8) % 3 - 1
    P.r1, P.bp = rowcol(c.in_rows, C, 6), vec(C, 12)
    out.append((tag, P, "exact"))
  return out


def _base_rows(P, c):
  _set_h(P, rowcol(c.in_rows, C, 0), c)
  if c.entry != "ffn":
    P.bo, P.r1, P.bp = vec(C, 1), rowcol(c.in_rows, C, 6), vec(C, 12)
  if c.entry == "block":
    P.bo1 = vec(C, 9)
  P.b2 = vec(C, 4)


def probe3(c):
  out = []
  j = torch.arange(HID)
  for tag in ("sel0", "sel1", "sel2", "sel3", "census"):
    P, g = neutral(c), _gen(13, c.M, len(tag) + ord(tag[-1]))
    _base_rows(P, c)
    gate = torch.where((7 * j + j // 64) % 5 == 0, 0.0, GELU_G).to(F64)
    if tag == "census":
      val = (1.0 - 2.0 * ((3 * j + j // 7) % 2)).to(F64) / 8.0
      P.w2 = _revive(_ri(g, -1, 1, C, HID) * (_ri(g, 0, 1, C, HID)))          # density 1/3
    else:
      val = ((5 * j) % 17 - 8).to(F64)
      val = torch.where(val == 0, torch.full_like(val, 4.0), val)
      P.w2, _ = _w2_onehot(int(tag[-1]))
    P.b1 = torch.cat([val, gate])
    out.append((tag, P, "exact"))
  return out


P4_EPS = 12.5


def p4_rows(rows, mean):
  """Rows of equal statistics (probe 4's multiset); mean > 0 lifts row r by mean + bit 4 of r."""
  mag = torch.cat([torch.full((160,), 1.0), torch.full((96,), 2.0), torch.full((64,), 3.0)]).to(F64)
  u = mag * (1.0 - 2.0 * (torch.arange(C) % 2))
  u = u[(37 * torch.arange(C)) % C]
  m, k = torch.arange(rows).view(-1, 1), torch.arange(C).view(1, -1)
  h = u[(k + 7 * m) % C] * (1.0 - 2.0 * ((m // 3) % 2))
  if mean:
    h = h + float(mean) + ((m >> 4) & 1)
  return h


def p4_cs():
  """The column sums of probe 4's value rows: the 64 non-zero integers of [-32, 32] in every 64-unit chunk, rotated by one
  from chunk to chunk, so a unit's sum differs from every other one of its chunk and from the unit at its place in the
  chunks before and after."""
  base = torch.cat([torch.arange(1, 33), -torch.arange(1, 33)])[(27 * torch.arange(64)) % 64]
  j = torch.arange(HID)
  return base[(j % 64 + j // 64) % 64].to(F64)


def p4_w1():
  """Ten non-zero integers per value row that add up to p4_cs: of one sign and as equal as possible from |cs| = 10 on
  (sum |w| = |cs| <= 32, so |sum w h0| <= 96 on rows of magnitude <= 3), +-1 (one 2 where needed) below."""
  w = torch.zeros(HID, C, dtype=F64)
  j = torch.arange(HID)
  cs = p4_cs()
  a, s = cs.abs().to(torch.int64), cs.sign()
  d = 10 - a
  for i in range(10):
    big = (a // 10 + (i < a % 10)).to(F64)
    small = torch.where(i < (d + 1) // 2, -1.0, 1.0) * torch.where((i == 9) & (d % 2 == 1), 2.0, 1.0)
    e = s * torch.where(a >= 10, big, small.to(F64))
    w[j, (j % 32 + 32 * ((i + j // 32) % 10) + 3 * (j // 32)) % C] = e
  return w


def probe4(c):
  out = []
  wv = p4_w1()
  j = torch.arange(HID)
  for mean in (False, True):
    for ph in range(4):
      P = neutral(c)
      _set_h(P, p4_rows(c.in_rows, mean), c)
      P.eps = P4_EPS
      P.w1[:HID] = wv
      P.b1 = torch.cat([((5 * j + j // 64) % 7 - 3).to(F64), torch.full((HID,), GELU_G, dtype=F64)])
      P.w2, _ = _w2_onehot(ph)
      P.b2 = (torch.arange(C) % 7).to(F64) - 3.0
      out.append((f"{'mean' if mean else 'zero'}{ph}", P, "ulp"))
  return out


def gelu_grid():
  """1280 gate values (float32-representable): 128 in [-12, -6), 768 in [-6, 0), 352 in (0, 12], +-0, the bf16
  neighbours of 0, and +-15 .. +-20 (1.4427 z^2 > 149 from |g| = 14.4 on: exp2 underflows to zero)."""
  a = torch.linspace(-12.0, -6.0, 129, dtype=F64)[:-1]
  b = torch.linspace(-6.0, 0.0, 769, dtype=F64)[:-1]
  d = torch.linspace(0.0, 12.0, 353, dtype=F64)[1:]
  sp = torch.tensor([0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 2.0 ** -120, -2.0 ** -120, 15.0, -15.0, 16.0, -16.0, 17.5, -17.5,
                     20.0, -20.0, 14.5, -14.5, 4.0, -4.0, 4.5, -4.5, 5.0, -5.0, 1.0, -1.0, 8.0, -8.0, 0.5, -0.5, 2.0, -2.0,
                     3.0, -3.0], dtype=F64)
  grid = torch.cat([a, b, d, sp]).to(F32).to(F64)
  assert grid.numel() == HID
  return grid[(77 * torch.arange(HID)) % HID]          # neighbours on the curve are not neighbours in the tile


def probe6(c):
  out = []
  grid = gelu_grid()
  for ph in range(4):
    P = neutral(c)
    P.b1 = torch.cat([torch.ones(HID, dtype=F64), grid])
    P.w2, j = _w2_onehot(ph)
    P.gsel = grid[j]
    out.append((f"ph{ph}", P, "gelu"))
  return out


def probe7(c):
  P, g = neutral(c), _gen(17, c.M, c.Tk)
  sp = lambda n, k, den, sc: _ri(g, -1, 1, n, k) * (torch.rand(n, k, generator=g) < den).to(F64) * sc
  P.x = _ri(g, -2, 2, c.in_rows, P.x.shape[1])
  if c.entry == "xtail":
    P.x.view(c.in_rows, H, SP)[:, :, S:] = 0.0
  P.r0, P.r1 = _ri(g, -3, 3, c.in_rows, C), _ri(g, -3, 3, c.in_rows, C)
  P.wo1, P.wo, P.wp = sp(C, K0, 0.4, 2.0 ** -3), sp(C, K0, 0.4, 2.0 ** -2), sp(C, C, 0.4, 2.0 ** -3)
  P.wq = sp(K0, C, 0.4, 2.0 ** -3)
  P.wq.view(H, SP, C)[:, S:] = 0.0
  P.qb = _ri(g, -1, 1, K0) * 0.5
  P.qb.view(H, SP)[:, S:] = 0.0
  P.k, P.v = _ri(g, -1, 1, *P.k.shape), _ri(g, -3, 3, *P.v.shape)
  P.w1, P.w2 = sp(2 * HID, C, 0.4, 2.0 ** -3), sp(C, HID, 0.2, 2.0 ** -3)
  P.b1 = _ri(g, -2, 2, 2 * HID) * 0.5
  P.bo1, P.bo, P.b2, P.bp = vec(C, 9), vec(C, 1), vec(C, 4), vec(C, 12)
  return [("chain", P, "bound")]


def probe5(c):
  """ldm_st_block's query projection: h1 = r0 = probe 4's rows lifted by 3 or 4 (integers in [0, 7]; eps = 12.5,
  rstd = 1/4), wq = 4 at one K column per live row (a permutation of the 320 channels; the 64 padded rows stay zero, as
  layout.split_kernel leaves them -- the kernel's layout contract), so q = h1[k(n)] - mean + qb, an integer.  Key j of
  sample s is the unit vector of dim (j + s) mod 40 in every head, so its logit is one element of q and every
  probability an exact power of two; V integer in [0, 4].  h1 >= 0 and att2 >= 0, so nothing cancels in
  out = h1 + att2: the one rcp enters at att2's magnitude, which is never above the output's.  Gate: 1 bf16 ulp of the
  reference."""
  assert c.entry == "block" and c.Tk >= S
  P, g = neutral(c), _gen(15, c.M)
  P.r0, P.eps = p4_rows(c.in_rows, 3), P4_EPS
  live = (SP * torch.arange(H).view(-1, 1) + torch.arange(S).view(1, -1)).reshape(-1)
  P.wq[live, (7 * torch.arange(C) + 3) % C] = 4.0
  P.qb[live] = (vec(C, 2) + 8) % 3 - 1
  j, s = torch.arange(c.Tk).view(1, -1), torch.arange(c.R).view(-1, 1)
  P.k.view(c.R, c.Tk, H, S)[s, j, :, (j + s) % S] = 1.0
  P.v = _ri(g, 0, 4, c.R, c.Tk, H, S)
  return [("unit-keys", P, "ulp")]


PROBES = {"p5": probe5, "p1": probe1, "p2": probe2, "p3": probe3, "p4": probe4, "p6": probe6, "p7": probe7}


# ---- the float64 reference (and the references of subtly wrong kernels) ------------------------------------------
LOSE_K = {"wo1": 263, "wq": 77, "wo": 263, "w1": 300, "w2": 701, "wp": 130}
PRODUCTS = {"ffn": ("w1", "w2"), "tail": ("wo", "w1", "w2", "wp"), "xtail": ("wo", "w1", "w2", "wp"),
            "block": ("wo1", "wq", "wo", "w1", "w2", "wp")}
# the product whose raw accumulator a wn = 0 wave's acc2[2] holds before each N = 320 product (None: zero-initialised; the
# query projection leaves its columns 256 .. 319 there, the o-projection W att2, the feed-forward W2 hidden)
STALE_FROM = {"wo1": None, "wo": "wq", "w2": "wo", "wp": "w2"}
PIECE3 = ("piece3_zero", "piece3_wn1_rows", "piece3_rows_192", "piece3_stale")
PAD = {"x": 8, "r0": 4, "r1": 12, "out": 4}
GUARD_ROWS = 2


def gelu64(x):
  return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_as64(x):
  """gelu_erf_f's formula (Abramowitz & Stegun 7.1.26) in float64."""
  ax = x.abs()
  z = ax * 0.70710678118654752440
  t = 1.0 / (1.0 + 0.3275911 * z)
  poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592)
  return x.clamp_min(0.0) - 0.5 * ax * poly * t * torch.exp2(-1.4426950408889634 * z * z)


def gelu_f32(x):
  """The same, every operation rounded to float32 (a transcription of gelu_erf_f; fma as two roundings)."""
  f = lambda v: v.to(F32)
  x = f(x)
  ax = x.abs()
  z = f(ax * f(torch.tensor(0.70710678118654752440)))
  t = f(1.0 / f(f(torch.tensor(0.3275911)) * z + 1.0))
  poly = f(torch.tensor(1.061405429))
  for cst in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
    poly = f(poly * t + f(torch.tensor(cst)))
  e = f(torch.exp2(f(f(f(torch.tensor(-1.4426950408889634)) * z) * z)))
  q = f(f(poly * t) * e)
  return f(f(-0.5 * ax) * q + x.clamp_min(0.0))


def ref64(P, mut=None, rnd=True, view="contig", rows=None):
  """The chain of include/ldm_hip.h in float64 on the operands of P; rnd: with the kernel's bf16 rounding points.
  `mut`: the reference of a subtly wrong kernel (MUTATIONS).  `rows`: evaluate only these rows (whole, aligned 128-row
  panels, ascending).  Returns (out [rows, C], info) with info.exact (no rounding point changed a value), info.absref,
  info.maxint (largest magnitude that passed a rounding point)."""
  c = P.case
  e, M = c.entry, c.M
  dev = P.x.device
  m = torch.arange(M, device=dev) if rows is None else rows.to(dev)
  src = m % c.in_rows
  mut = mut or ("none",)
  kind, target = mut[0], (mut[1] if len(mut) > 1 else None)
  info = SimpleNamespace(exact=True, maxint=0.0, absref=None, pow2=None)
  nan = float("nan")

  def R_(t):
    q = rb(t)
    if not bool(((q - t).abs() <= 1e-12 * t.abs()).all()):      # (gelu(8) = 8 (1 - 6e-16) in float64)
      info.exact = False
    info.maxint = max(info.maxint, float(t.abs().max()))
    return q if rnd else t

  rowmask = ((m >= 32) & (m < 48) if M > 32 else torch.ones_like(m, dtype=torch.bool)).to(F64).view(-1, 1)

  accs = {}

  def prod(name, A, W):
    out = A @ W.t()
    accs[name] = out.clone()
    if target != name:
      return out
    K = A.shape[1]
    if kind == "lose_k":
      k = LOSE_K[name]
      out[:, 64:128] -= A[:, k:k + 1] * W[64:128, k].view(1, -1) * rowmask
    elif kind == "drop_last_ktile":
      out = out - A[:, K - 64:] @ W[:, K - 64:].t()
    elif kind == "double_mid_ktile":
      t = (K // 64) // 2
      out = out + A[:, 64 * t:64 * t + 64] @ W[:, 64 * t:64 * t + 64].t()
    elif kind == "shift_b_ktile":
      out = A[:, :K - 64] @ W[:, 64:].t()
    elif kind == "piece3_zero":
      out[:, 256:320] = 0.0
    elif kind == "piece3_wn1_rows":       # rows 64 .. 127 of the third piece's ring slot: weight rows 320 .. 383, which
      slot = torch.cat([W, torch.zeros(K0 - C, K, dtype=F64, device=dev)])      # issue_rows leaves to the out-of-range zero
      out[:, 256:320] = A @ slot[320:384].t()
    elif kind == "piece3_rows_192":       # ... or the rows the wn = 1 wave read last: those of the second piece
      out[:, 256:320] = A @ W[192:256].t()
    elif kind == "piece3_stale":          # neither zeroed nor computed: what the product before it left in acc2[2]
      prev = accs.get(STALE_FROM[name])
      out[:, 256:320] = 0.0 if prev is None else prev[:, 256:320]
    return out

  def bias(name):
    b = getattr(P, name)
    if kind == "swap_bias" and name in ("bo", "b2", "bp"):
      b = getattr(P, {"bo": "b2", "b2": "bp", "bp": "bo"}[name])
    if kind == "shift4" and target == name:
      b = torch.roll(b, -4)
    return b.view(1, -1)

  def residual(name):
    if kind == "swap_res":
      name = {"r0": "r1", "r1": "r0"}[name]
    r = getattr(P, name)
    if kind == "r1_unmapped" and name == "r1":          # rows m >= in_rows meet the NaN guard behind r1
      out = r[src].clone()
      out[m >= c.in_rows] = nan
      return out
    if kind == "stride_ignored" and target == name and view == "padded":
      buf = torch.full((c.in_rows + GUARD_ROWS, C + PAD[name]), nan, dtype=F64, device=dev)
      buf[:c.in_rows, :C] = r
      idx = src.view(-1, 1) * C + torch.arange(C, device=dev).view(1, -1)
      return buf.view(-1)[idx]
    return r[src]

  def stats(h):
    mu = h.mean(1, keepdim=True)
    var = ((h - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + P.eps)
    if kind == "stats_xor16":
      i = torch.arange(h.shape[0], device=dev)
      j = torch.where((i ^ 16) < h.shape[0], i ^ 16, i)
      mu, rstd = mu[j], rstd[j]
    return mu, rstd

  def attention(q):
    npan = m.numel() // 128
    smp = m[::128] // c.T
    if kind == "ctx_next_sample":
      smp = (smp + 1) % c.R
    qh = q.view(npan, 128, H, SP)[..., :S]
    logits = torch.einsum("pqhs,pchs->phqc", qh, P.k[smp])
    p = R_(torch.exp2(logits - logits.max(dim=3, keepdim=True).values))
    info.pow2 = bool(torch.equal(p, torch.exp2(torch.log2(p).round())))
    o = torch.einsum("phqc,pchs->pqhs", p, P.v[smp]) / p.sum(dim=3).permute(0, 2, 1).unsqueeze(3)
    out = torch.zeros(npan, 128, H, SP, dtype=F64, device=dev)
    out[..., :S] = R_(o)
    return out.view(-1, K0)

  a = P.x[src]
  if e == "block":
    h1 = R_(residual("r0") + bias("bo1") + prod("wo1", a, P.wo1))
    mu, rstd = stats(h1)
    q = R_(rstd * (prod("wq", h1, P.wq) - mu * P.wq.sum(1).view(1, -1)) + bias("qb"))
    res = h1
  elif e == "xtail":
    q, res = a, residual("r0")
  if e in ("xtail", "block"):
    att = attention(q)
  elif e == "tail":
    att, res = a, residual("r0")
  h = a if e == "ffn" else R_(res + bias("bo") + prod("wo", att, P.wo))

  mu, rstd = stats(h)
  acc = prod("w1", h, P.w1)
  cs, b1 = P.w1.sum(1), P.b1
  if kind == "aux_prev_chunk":
    roll = lambda t: torch.cat([torch.roll(t[:HID], 64), torch.roll(t[HID:], 64)])
    cs, b1 = roll(cs), roll(b1)
  if kind == "cs_bias_swapped":
    cs, b1 = b1, cs
  pre = rstd * acc - rstd * mu * cs.view(1, -1) + b1.view(1, -1)
  val, gate = pre[:, :HID].clone(), pre[:, HID:].clone()
  if kind == "val_gate_swapped":
    val[:, 96:128], gate[:, 96:128] = pre[:, HID + 96:HID + 128], pre[:, 96:128]
  if kind == "gelu_tanh":
    gl = 0.5 * gate * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (gate + 0.044715 * gate ** 3)))
  elif kind == "gelu_relu4":
    gl = torch.where(gate.abs() > 4.0, gate.clamp_min(0.0), gelu64(gate))
  else:
    gl = gelu64(gate)
  hid = R_(val * gl)
  if kind == "hidden_cell_shift":
    hid[:, 192:256] = hid[:, 192:256][:, torch.arange(64, device=dev) ^ 4]
  y = h + bias("b2") + prod("w2", hid, P.w2)
  if e == "ffn":
    out = R_(y)
    info.absref = h.abs() + P.b2.abs().view(1, -1) + hid.abs() @ P.w2.abs().t()
  else:
    y = R_(y)
    r1 = residual("r1")
    out = R_(r1 + bias("bp") + prod("wp", y, P.wp))
    info.absref = torch.nan_to_num(r1.abs()) + P.bp.abs().view(1, -1) + y.abs() @ P.wp.abs().t()
  if kind == "swap_rows":
    i, j = target - 1, target
    out[[i, j]] = out[[j, i]]
  return out, info


# ---- gates: (figure in units of the gate, passed) ---------------------------------------------------------------
def _ratio(err, tol):
  r = err / tol
  r = torch.where(err == 0, torch.zeros_like(r), r)
  r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
  return float(r.max()) if r.numel() else 0.0


def _err(got, ref):
  got = got.to(F64)
  err = (got - ref).abs()
  return torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))


def judge(gate, got, ref, info, P, c):
  """got, ref [rows, C] (same device).  exact: figure in bf16 ulp, passes only at 0; ulp: <= 1 bf16 ulp; gelu: 1 true bf16
  ulp + GELU_A |gate|, and bf16(g) exactly from g = 15 on; bound: 2^-9 (4 MODEL_C absref + |ref|)."""
  err = _err(got, ref)
  if gate == "exact":
    f = _ratio(err, bf16_ulp(ref))
    return f, f == 0.0
  if gate == "ulp":
    f = _ratio(err, bf16_ulp(ref))
    return f, f <= 1.0
  if gate == "gelu":
    g = P.gsel.to(ref.device).view(1, -1).expand_as(ref)
    f = _ratio(err, true_ulp(ref) + GELU_A * g.abs())
    far = g >= 15.0
    ok = bool(torch.equal(got.to(F64)[far], rb(g)[far]))
    return (f if ok else float("inf")), f <= 1.0 and ok
  assert gate == "bound"
  f = _ratio(err, 2.0 ** -9 * (4.0 * MODEL_C[c.entry] * info.absref + ref.abs()) + TINY)
  return f, f <= 1.0


def c_needed(got, ref, absref):
  need = ((got - ref).abs() - 2.0 ** -9 * ref.abs() - TINY) / (2.0 ** -9 * absref.clamp_min(1e-300))
  return max(0.0, float(need.max()))


# ---- mutations -------------------------------------------------------------------------------------------------
def mutations():
  out = [(k, p) for p in ("wo1", "wq", "wo", "w1", "w2", "wp")
         for k in ("lose_k", "drop_last_ktile", "double_mid_ktile", "shift_b_ktile")]
  out += [(k, p) for p in ("wo1", "wo", "w2", "wp") for k in PIECE3]
  out += [("aux_prev_chunk",), ("cs_bias_swapped",), ("val_gate_swapped",), ("hidden_cell_shift",)]
  out += [("shift4", b) for b in ("bo1", "qb", "bo", "b2", "bp")] + [("swap_bias",), ("swap_res",)]
  out += [("stride_ignored", "r0"), ("stride_ignored", "r1")]
  out += [("swap_rows", b) for b in (16, 32, 64, 128)] + [("stats_xor16",), ("r1_unmapped",), ("ctx_next_sample",)]
  out += [("store_row_M",), ("store_pad",), ("gelu_tanh",), ("gelu_relu4",)]
  return out


MUTATIONS = mutations()


def mutation_applies(mut, c):
  """(applies, reason if not)."""
  kind, target = mut[0], (mut[1] if len(mut) > 1 else None)
  if kind in ("lose_k", "drop_last_ktile", "double_mid_ktile", "shift_b_ktile") + PIECE3 and target not in PRODUCTS[c.entry]:
    return False, "the entry point has no such product"
  if kind == "shift4" and target not in {"ffn": ("b2",), "tail": ("bo", "b2", "bp"), "xtail": ("bo", "b2", "bp"),
                                         "block": ("bo1", "qb", "bo", "b2", "bp")}[c.entry]:
    return False, "the entry point has no such vector"
  if kind in ("swap_bias", "swap_res", "stride_ignored") and c.entry == "ffn":
    return False, "ldm_ffn_geglu has one bias and no global residual"
  if kind == "stride_ignored" and c.M == 1:
    return False, "one row: its stride is never used"
  if kind == "swap_rows" and c.M <= target:
    return False, "no such row"
  if kind == "stats_xor16" and c.M <= 16:
    return False, "no row 16"
  if kind == "r1_unmapped" and c.in_rows == c.M:
    return False, "not a pair"
  if kind == "ctx_next_sample" and c.R < 2:
    return False, "no context, or one sample"
  return True, ""


def store(buf, out, M, mut=None):
  """What a launch leaves in `out`'s buffer [(M + GUARD_ROWS), C + pad] (sentinel-filled): rows < M, columns < C; the two
  out-of-bounds mutations write one cell more."""
  buf = buf.clone()
  buf[:M, :C] = out
  if mut == ("store_row_M",):
    buf[M, :4] = out[M - 1, :4]
  if mut == ("store_pad",) and buf.shape[1] > C:
    buf[0, C:C + 4] = out[0, :4]
  return buf


def untouched(before, after, M):
  """Pad columns and guard rows bit-identical."""
  b, a = before.view(torch.int16), after.view(torch.int16)
  return bool(torch.equal(b[M:], a[M:]) and torch.equal(b[:M, C:], a[:M, C:]))


# ---- device operands ---------------------------------------------------------------------------------------------
SENTINEL = 24576.0


def device_operands(P, dev, padded):
  """The launch's arguments through the project's own layout functions (layout.dense_kernel, geglu_kernel, ln_fold with
  gamma = 1 / beta = 0, ffn_aux), as views of NaN-filled buffers: input rows with padded pitches where `padded` (and
  where the host wrapper takes a pitch), in_rows rows followed by as many NaN rows in the pair form, out with a sentinel
  in its pad columns and its two guard rows.  Returns a namespace; D.out_buf is out's whole buffer."""
  import numpy as np
  from ldm_tf2_amd import layout as L
  c = P.case
  D = SimpleNamespace()
  nan = float("nan")
  one, zero = np.ones(C, np.float32), np.zeros(C, np.float32)
  dk = lambda w: L.dense_kernel(w.t().contiguous().to(F32).numpy(), BF, dev)

  def rows(t, pad, can_pad=True):
    n, w = t.shape
    guard = n if c.in_rows != c.M else GUARD_ROWS
    buf = torch.full((n + guard, w + (pad if padded and can_pad else 0)), nan, dtype=F64)
    buf[:n, :w] = t
    return buf.to(BF).to(dev)[:n, :w]

  D.x = rows(P.x, PAD["x"], c.entry in ("ffn", "tail"))
  if c.entry in ("xtail", "block"):
    D.x = D.x.view(c.in_rows // c.T, c.T, K0)
    kd = torch.zeros(c.R, c.Tk, H, SP, dtype=F64)
    kd[..., :S] = P.k
    kd[..., MS_DIM] = 1.0
    vv = torch.zeros(c.R, c.Tk, H, SP, dtype=F64)
    vv[..., :S] = P.v
    vv[..., MS_DIM] = 1.0
    vt = torch.full((c.R, K0, c.ldv), nan, dtype=F64)
    vt[:, :, :c.Tk] = vv.reshape(c.R, c.Tk, K0).permute(0, 2, 1)
    D.k, D.vt = kd.reshape(c.R, c.Tk, K0).to(BF).to(dev), vt.to(BF).to(dev)
  D.r0, D.r1 = rows(P.r0, PAD["r0"]), rows(P.r1, PAD["r1"])
  gw, gb = L.geglu_kernel(P.w1.t().contiguous().to(F32).numpy(), P.b1.to(F32).numpy(), F32, "cpu")
  D.w1, cs, bb = L.ln_fold(gw, one, zero, gb.numpy(), BF, dev)
  D.aux = L.ffn_aux(cs, bb)
  D.w2, D.b2 = dk(P.w2), L.vec(P.b2, dev)
  if c.entry != "ffn":
    D.wo, D.bo, D.wp, D.bp = dk(P.wo), L.vec(P.bo, dev), dk(P.wp), L.vec(P.bp, dev)
  if c.entry == "block":
    D.wo1, D.bo1 = dk(P.wo1), L.vec(P.bo1, dev)
    D.wq, D.qcs, D.qb = L.ln_fold(P.wq.to(F32), one, zero, P.qb.to(F32).numpy(), BF, dev)
  D.out_buf = torch.full((c.M + GUARD_ROWS, C + (PAD["out"] if padded else 0)), SENTINEL, dtype=BF, device=dev)
  D.out = D.out_buf[:c.M, :C]
  return D


def launch(ops, P, D):
  c = P.case
  if c.entry == "ffn":
    ops.ffn_geglu(D.x, D.w1, D.aux, D.w2, D.b2, D.out, P.eps)
  elif c.entry == "tail":
    ops.st_tail(D.x, D.wo, D.bo, D.r0, D.w1, D.aux, D.w2, D.b2, D.wp, D.bp, D.r1, D.out, P.eps)
  elif c.entry == "xtail":
    ops.st_xtail(D.x, D.k, D.vt, D.wo, D.bo, D.r0, D.w1, D.aux, D.w2, D.b2, D.wp, D.bp, D.r1, D.out, P.eps)
  else:
    ops.st_block(D.x, D.wo1, D.bo1, D.r0, D.wq, D.qcs, D.qb, D.k, D.vt, D.wo, D.bo, D.w1, D.aux, D.w2, D.b2, D.wp, D.bp,
                 D.r1, D.out, P.eps)

