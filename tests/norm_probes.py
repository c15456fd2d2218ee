"""Exact probes of the GroupNorm and LayerNorm kernels (a plain module: builders, float64 reference, float32
emulations, mutations and the case matrix; tests/test_norm_probes_cpu.py and tests/test_zz_norm_accounting_gpu.py use it).

Probe "census".  A unit is a (sample, group) of a GroupNorm or a row of a LayerNorm, with n elements.  Every element of
unit u is the integer M_u, |M_u| in 4 .. 7, sign and value differing between neighbouring groups, samples and rows,
except p pairs of deviants at M_u + d and M_u - d (d in {1, 2}, 1 <= p <= 4).  All values are integers below 256 (exact
in bf16) and every partial sum is an integer below 2^24 (exact in float32 in any order): the mean is exactly M_u,
x - mean is exactly 0 or +-d and the sum of squares is the integer 2 p d^2.

Gates.  Non-deviant elements are bit-exact: the output is beta[c] as stored in the output dtype.  beta is 0 on every
second channel of a group (any error of the mean shows as a non-zero value where an exact zero is due) and takes
non-zero bf16 values elsewhere; gamma is a non-zero bf16 value per channel (both distinct within any 1536 consecutive
channels: 6 binades x 128 mantissas x 2 signs).  With SiLU: exact zero at the beta = 0 channels, the rest by
norm_check.check.  Deviants are compared with the float64 reference +-d gamma / sqrt(2 p d^2 / n + eps) + beta: bf16
within 1 bf16 ulp (norm_check.bf16_ulp); float32 within 8 * 2^-24 * (|ref - beta| + |beta|) -- the roundings of S2 / n,
of + eps, of rsqrtf (1 ulp), of * gamma, of d * sc and of + beta come to about 4 ulp, doubled for margin.  A lost
deviant changes the value by at least 1 / (2 p) >= 12 %.

Sweep.  Only deviants probe the second pass and the gamma index.  A case runs L launches; unit k of its class takes
the 2 p consecutive positions from t = (launch * U + k) * 2 p of its own n = HW * cpg elements, taken mod n and moved on
by one for every completed pass t / n (position q = pixel q / cpg, channel q % cpg of the group).  The classes of the fused GroupNorm are the group's slot g % GB in its
workgroup, so the union over units and launches covers the whole slab [HW][GB * cpg] of a workgroup; L is the smallest
count that does, and L <= 24 is a condition on B (sweep_launches).  LayerNorm: every column.  The two-launch pair
never makes the pilot element (pixel 0, the group's first channel, K of gn_pilot) a deviant in its exact cases (its
sweep covers every other position; x - K is then 0 or +-d and dm exactly 0); one extra case per dtype makes the pilot a
deviant of every unit and is gated by norm_check.check.  The one-row case of the GEMM's LayerNorm output (N = 320)
cannot cover 320 columns with 8 deviants in 24 launches: it sweeps the first 192 columns, the cases with M >= 127
sweep all (the column a lane owns does not depend on the row).

Buffers.  Input and output are channel slices of wider buffers at a 16-byte channel offset whose row pitch is a
multiple of EPC and not C.  The foreign input channels and the rows after the last sample hold NaN; the foreign output
channels hold a bit pattern that must survive; the output is pre-filled with NaN; two runs must give identical bits.

Reference.  The formulas of include/ldm_hip.h in float64 (reference()); the CPU test compares it with the oracle's
group_norm and layer_norm.  Mutations (MUTATIONS) are references of subtly wrong kernels; every one must fail the
gates on every case mutation_applies() names.

RESULTS (MI355X; per family and dtype the largest deviant error in units of its gate, <= 1 passes; every non-deviant
was bit-exact, every output outside the slice kept its pattern and every second run gave the same bits):
  family                         cases  launches  bf16   float32
  ldm_groupnorm_fused            29+23  398+233   0.50   0.33   (fused-f32-B3-HW200-C2560, form 1.20.512.8)
  ldm_groupnorm_partial + apply  14+12  120+94    0.50   0.30   (pair-f32-B3-HW215-C640-G64)
  ldm_layernorm                  14+15   80+71    0.50   0.24   (ln-f32-B77-C772, LPR 32)
  ldm_gemm ln_out                 4+4    27+27    0.50   0.16
  ldm_gemm ln_cs (fold)           4       4       0.53 bf16 ulp over all elements (tile 14, one workgroup per panel)
  The bf16 figure is the rounding of the store itself.  The pilot cases gave rel-L2 6.3e-6 and max |err| 1.8e-3 in
  float32 against norm_check's 3.5e-5 and 3.2e-3 (the pilot there is an outlier at 16 sigma of its group).  Every case
  passed on the first run: no kernel was changed.
"""
import math
from collections import namedtuple

import torch

from norm_check import bf16_ulp, check

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
DTN = {F32: "f32", BF: "bf16"}
EPS = 1e-5
MAX_LAUNCHES = 24
F32_GATE = 8.0 * 2.0 ** -24
FOREIGN = -7.5                    # the bit pattern of the foreign output channels

# kind: fused | pair | ln | ln_out | ln_fold.  B samples (rows for the LayerNorms) x HW pixels (1) x C channels in G
# groups (1); p pairs of deviants; nchunks: the pair's (0 = the library's choice); pilot: the pair's pilot is a deviant;
# form: fused (GB, S, NT, MAXCH), ln (LPR,), ln_fold (tile, deal), else ()
Case = namedtuple("Case", "kind dt B HW C G p nchunks silu pilot form")


def epc(dt):
  return 8 if dt == BF else 4


def cpg(c):
  return c.C // c.G


# ---- host mirrors ------------------------------------------------------------------------------------------------
def fused_plan(B, HW, C, G, dt):
  """gn_fused_plan of csrc/gn_fused.h: (GB, S, NT, MAXCH) or None."""
  if G <= 0 or C % G:
    return None
  e, cg = epc(dt), C // G
  if cg < e:
    return None
  GB = next((g for g in (1, 2, 4, 8) if G % g == 0 and (g * cg) % e == 0), 0)
  if not GB:
    return None
  S = GB * cg // e
  if S > 64:
    return None
  need = -(-HW // (64 // S))
  waves = B * (G // GB)
  if need <= 8 and waves >= 512:
    return (GB, S, 64, 8)
  if need <= 16 and waves >= 512:
    return (GB, S, 64, 16)
  if need <= 24 and waves >= 1024:
    return (GB, S, 64, 24)
  for NT in (256, 512, 1024):
    need = -(-HW // (NT // S))
    if need <= 8:
      return (GB, S, NT, 8)
    if need <= 16:
      return (GB, S, NT, 16)
  return None


def old_last_loop(S, HW):
  """The plan loop this module's enumeration proved dead: the (NT, 24) it would return once every form above it
  has refused the slab, or None."""
  if any(-(-HW // (NT // S)) <= 16 for NT in (256, 512, 1024)):
    return None
  for NT in (256, 512):
    if -(-HW // (NT // S)) <= 24:
      return (NT, 24)
  return None


def nchunks_default(B, HW):
  """ldm_groupnorm_nchunks."""
  return max(1, min((1024 + B - 1) // B, max(1, HW // 32), 128))


def pair_geom(c):
  """(nchunks, ppc, VT, P) of gn_partial_kernel."""
  nch = c.nchunks or nchunks_default(c.B, c.HW)
  nvec = c.C // epc(c.dt)
  VT = min(nvec, 256)
  return nch, -(-c.HW // nch), VT, 256 // VT


def ln_lpr(C, dt):
  nvec, lpr = C // epc(dt), 4
  while lpr < 64 and lpr * 8 < nvec:
    lpr *= 2
  return lpr


# ---- census ----------------------------------------------------------------------------------------------------
def _bf16_family(j, lo_exp):
  """Distinct non-zero bf16 values for j = 0 .. 1535: sign, 6 binades from 2^lo_exp, 128 mantissas."""
  j = j % 1536
  sign = 1.0 - 2.0 * (j % 2)
  i = j // 2
  return sign * 2.0 ** (lo_exp + (i // 128) % 6) * (1.0 + (i % 128) / 128.0)


def params(c):
  """(gamma, beta) float32 [C], bf16-representable; beta = 0 on every second channel of a group."""
  cg = cpg(c)
  ch = torch.arange(c.C)
  g, k = ch // cg, ch % cg
  gamma = _bf16_family(ch * 7 + 3, -2).to(F32)
  beta = _bf16_family(ch * 5 + 1, -3).to(F32)
  beta[(k + g) % 2 == 0] = 0.0
  assert torch.equal(gamma.to(BF).to(F32), gamma) and torch.equal(beta.to(BF).to(F32), beta)
  return gamma, beta


def unit_values(c):
  """M_u [B, G] float64."""
  b = torch.arange(c.B).view(-1, 1)
  g = torch.arange(c.G).view(1, -1)
  return ((1 - 2 * ((b + g) % 2)) * (4 + (b + g // 2 + b // 2) % 4)).to(F64)


def base(c):
  """The input without deviants: [B * HW, C] float64."""
  m = unit_values(c).repeat_interleave(cpg(c), dim=1)            # [B, C]
  return m.repeat_interleave(c.HW, dim=0).contiguous()


def sweep_class(c):
  """(gb, U): groups g and g' of a sample share deviant classes when g % gb == g' % gb; U units per class."""
  gb = c.form[0] if c.kind == "fused" else 1
  return gb, c.B * (c.G // gb)


def sweep_launches(c):
  if c.pilot:
    return 1
  gb, U = sweep_class(c)
  span = c.HW * cpg(c) - (1 if c.kind == "pair" else 0)
  L = -(-span // (U * 2 * c.p))
  if c.kind == "ln_out" and c.B == 1:
    L = min(L, MAX_LAUNCHES)
  return L


def deviants(c, launch):
  """(row [N], channel [N], delta [N] float64, unit [N]) of the launch's deviants; row = b * HW + pixel."""
  cg = cpg(c)
  n = c.HW * cg
  gb, U = sweep_class(c)
  skip = 1 if c.kind == "pair" else 0
  span = n - skip
  assert 2 * c.p <= span
  b = torch.arange(c.B).view(-1, 1, 1)
  g = torch.arange(c.G).view(1, -1, 1)
  i = torch.arange(2 * c.p).view(1, 1, -1)
  k = b * (c.G // gb) + g // gb
  t = (launch * U + k) * 2 * c.p + i
  q = skip + (t + t // span) % span                   # (a second pass over the unit is shifted by one position)
  if c.pilot:
    q = torch.where(i == 0, torch.zeros_like(q), 1 + ((k * 2 * c.p + i) % (n - 1)))
  d = 1 + (k + launch) % 2
  delta = (d * (1 - 2 * (i % 2))).to(F64)
  row = b * c.HW + q // cg
  ch = g * cg + q % cg
  unit = (b * c.G + g).expand_as(q)
  return row.reshape(-1), ch.reshape(-1), delta.reshape(-1), unit.reshape(-1)


def census(c, launch):
  """x [B * HW, C] float64 of the launch."""
  x = base(c)
  r, ch, delta, _ = deviants(c, launch)
  x[r, ch] += delta
  return x


def slab_positions(c, launch):
  """The launch's deviant positions reduced to (pixel, channel offset in the workgroup's GB * cpg segment)."""
  cg = cpg(c)
  gb, _ = sweep_class(c)
  r, ch, _, _ = deviants(c, launch)
  return (r % c.HW) * (gb * cg) + ch % (gb * cg)


# ---- float64 reference and its mutations --------------------------------------------------------------------------
MUTATIONS = ["drop_mean", "drop_square", "straddle_low", "pad_slot", "idle_row", "padded_n", "next_sample",
             "slice_left", "gamma_shift", "chunk_tail", "last_vector", "row0"]


def _fused_geom(c):
  GB, S, NT, MC = c.form
  return GB, S, NT, MC, NT // S


def mutation_applies(c, name):
  """Whether mutation `name` changes what a kernel of case c's kind computes (else it is exempt)."""
  gn = c.kind in ("fused", "pair")
  ln = c.kind in ("ln", "ln_out")
  if c.kind == "ln_fold":
    return False                                      # (its own lost-deviant check: test_norm_probes_cpu.py)
  if name in ("drop_mean", "drop_square", "gamma_shift"):
    return True
  if name == "slice_left":
    return c.kind != "ln_out"                         # the product has no foreign channels
  if name == "next_sample":
    return gn and c.B > 1
  if c.kind == "fused":
    GB, S, NT, MC, P = _fused_geom(c)
    if name == "straddle_low":
      return cpg(c) % epc(c.dt) != 0
    if name in ("pad_slot", "padded_n"):
      return MC * P != c.HW
    if name == "idle_row":
      return c.HW % P != 0
  if c.kind == "pair" and name == "chunk_tail":
    return c.HW % pair_geom(c)[1] != 0
  if c.kind == "ln" and name == "last_vector":
    return (c.C // epc(c.dt)) % c.form[0] != 0
  if ln and name == "row0":
    return c.B > 1
  return False


def reference(c, x, gamma, beta, mut=None, launch=0, left=None):
  """GroupNorm (LayerNorm: HW = G = 1) of x [B * HW, C] float64 by the formulas of include/ldm_hip.h, in float64.
  mut: the statistics of a subtly wrong kernel (MUTATIONS); left: x's slice moved one chunk left (slice_left)."""
  B, HW, C, G = c.B, c.HW, c.C, c.G
  cg = C // G
  e = epc(c.dt)
  xg = x.view(B, HW, G, cg)
  src = xg                                            # what the statistics read
  n = float(HW * cg)
  gam, bet = gamma.to(F64).to(x.device), beta.to(F64).to(x.device)
  if mut == "slice_left":
    src = left.view(B, HW, G, cg)
  if mut == "row0":
    xg = xg.clone()
    xg[B - 1] = xg[0]
    src = xg
  if mut == "idle_row":
    P = _fused_geom(c)[4]
    src = src[:, :HW - HW % P]
  if mut == "chunk_tail":
    ppc = pair_geom(c)[1]
    src = src[:, :HW - HW % ppc]
  if mut == "last_vector":
    src = src[..., :cg - e]
  s1 = src.sum(dim=(1, 3))                            # [B, G]
  if mut == "drop_mean":
    s1 = s1 - xg[:, HW - 1, :, cg - 1]
  if mut == "straddle_low":
    # the elements of group g + 1 that share a chunk with group g are counted to g
    for g in range(G - 1):
      head = (-((g + 1) * cg)) % e                    # elements of g + 1 in the chunk that straddles the boundary
      if head and (g + 1) % c.form[0]:                # (the boundary lies inside a workgroup's segment)
        t = xg[:, :, g + 1, :head].sum(dim=(1, 2))
        s1[:, g] += t
        s1[:, g + 1] -= t
  if mut == "padded_n":
    GB, S, NT, MC, P = _fused_geom(c)
    n = float(MC * P * cg)
  mean = s1 / n
  if mut == "next_sample":
    mean = mean.roll(-1, 0)
  dv = src - mean.view(B, 1, G, 1)
  s2 = (dv * dv).sum(dim=(1, 3))
  if mut == "drop_square":
    r, ch, delta, unit = deviants(c, launch)
    first = torch.arange(0, len(r), 2 * c.p)          # the first deviant of every unit
    s2 = s2 - (delta[first] ** 2).view(B, G).to(x.device)
  if mut == "pad_slot":
    GB, S, NT, MC, P = _fused_geom(c)
    s2 = s2 + (MC * P - HW) * cg * mean * mean
  rstd = 1.0 / torch.sqrt(s2 / n + EPS)
  if mut == "gamma_shift":
    gam, bet = gam.roll(-1), bet.roll(-1)
  y = (xg - mean.view(B, 1, G, 1)) * rstd.view(B, 1, G, 1)
  y = y.reshape(B * HW, C) * gam + bet
  return y * torch.sigmoid(y) if c.silu else y


def fold_reference(c, x, w_sel, bias):
  """The GEMM's LayerNorm fold with one-hot weight rows: out[m][n] = rstd_m (x[m][k(n)] - mean_m) + bias[n]."""
  mean = x.mean(dim=1, keepdim=True)
  var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
  return (x[:, w_sel] - mean) / torch.sqrt(var + EPS) + bias.to(F64)


# ---- gates -----------------------------------------------------------------------------------------------------------
def rounded(y, dt):
  return y.to(dt)


def thread_slot(c, pixel, ch):
  """Where the kernel holds element (pixel, channel)."""
  e = epc(c.dt)
  if c.kind == "fused":
    GB, S, NT, MC, P = _fused_geom(c)
    seg = GB * cpg(c)
    return f"workgroup segment {ch // seg}, thread {(pixel % P) * S + (ch % seg) // e}, chunk {pixel // P}, element {ch % seg % e}"
  if c.kind == "pair":
    nch, ppc, VT, P = pair_geom(c)
    v = ch // e
    return f"chunk {pixel // ppc}, thread {((pixel % ppc) % P) * VT + v % VT}, vector {v}, element {ch % e}"
  if c.kind == "ln":
    v = ch // e
    return f"lane {v % c.form[0]} of the row, piece {v // c.form[0]}, element {ch % e}"
  return f"lane {ch // 8}, element {ch % 8}"


def first_difference(c, bad, got, want):
  """The first element of the [B * HW, C] mask `bad`, decoded to (sample, pixel, channel, group, thread slot)."""
  idx = torch.nonzero(bad.reshape(-1))
  if idx.numel() == 0:
    return None
  i = int(idx[0])
  r, ch = divmod(i, c.C)
  b, pix = divmod(r, c.HW)
  return (f"{int(bad.sum())} elements differ, first at sample/row {b} pixel {pix} channel {ch} group {ch // cpg(c)} "
          f"({thread_slot(c, pix, ch)}): got {float(got.reshape(-1)[i])!r}, expected {float(want.reshape(-1)[i])!r}")


def _checked(label, got, ref, dt, k):
  """norm_check.check (max |gamma| = 16) as a message."""
  try:
    check(label, got, ref.cpu(), dt, k, 16.0)
  except AssertionError as err:
    return str(err)
  return None


def gates(c, got, ref, beta, launch, label=""):
  """got [B * HW, C] in the output dtype, ref float64 (same device).  Returns (message or None, worst deviant error in
  units of its gate)."""
  dev = got.device
  g64 = got.to(F64)
  if c.pilot:
    # norm_check's k is the input's offset / sigma: here at least |M_u| / (d sqrt(2 p / n)) >= 4 / (2 sqrt(2 p / n))
    return _checked(label, got, ref, c.dt, 2.0 * math.sqrt(c.HW * cpg(c) / (2.0 * c.p))), 0.0
  b_dt = beta.to(c.dt).to(F64).to(dev).expand_as(g64)
  r, ch, _, _ = deviants(c, launch)
  r, ch = r.to(dev), ch.to(dev)
  isdev = torch.zeros(g64.shape, dtype=torch.bool, device=dev)
  isdev[r, ch] = True
  if c.silu:
    bad = (~isdev) & (b_dt == 0) & ~(g64 == 0)
    msg = first_difference(c, bad, g64, b_dt)
    if msg:
      return "a non-deviant at a beta = 0 channel is not exactly zero: " + msg, 0.0
    return _checked(label, got, ref, c.dt, 0), 0.0
  bad = (~isdev) & ~(g64 == b_dt)
  msg = first_difference(c, bad, g64, b_dt)
  if msg:
    return "non-deviants are not exactly beta: " + msg, 0.0
  gd, rd, bd = g64[r, ch], ref[r, ch], b_dt[r, ch]
  tol = bf16_ulp(rd) if c.dt == BF else F32_GATE * ((rd - bd).abs() + bd.abs())
  err = (gd - rd).abs() / tol
  err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
  worst = float(err.max())
  if worst > 1.0:
    full = torch.zeros(g64.shape, dtype=torch.bool, device=dev)
    j = err > 1.0
    full[r[j], ch[j]] = True
    return f"a deviant is {worst:.2f} x its gate from the float64 reference: " + first_difference(c, full, g64, ref), worst
  return None, worst


def fold_operands(c):
  """(N, k(n) [N], bias [N] float32) of an ln_fold case: weight row n is one-hot at column k(n), so ln_cs[n] = 1."""
  N = 320 if c.form[0] == 13 else 384
  n = torch.arange(N)
  bias = _bf16_family(n * 5 + 1, -3).to(F32)
  bias[n % 2 == 0] = 0.0
  return N, (n * 7 + 3) % c.C, bias


def fold_gates(c, got, ref):
  """Every element within 1 bf16 ulp (norm_check.bf16_ulp) of the float64 reference: this kernel takes E[x^2] - mean^2
  and adds rstd * x and -rstd * mean separately, so its non-deviants are not bit-exact.  (message or None, worst)."""
  g64 = got.to(F64)
  err = (g64 - ref).abs() / bf16_ulp(ref)
  err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
  worst = float(err.max())
  if worst > 1.0:
    i = int(torch.nonzero((err > 1.0).reshape(-1))[0])
    m, n = divmod(i, ref.shape[1])
    return (f"row {m} column {n} is {worst:.2f} bf16 ulp from the float64 reference: got {float(g64[m, n])!r}, "
            f"expected {float(ref[m, n])!r}"), worst
  return None, worst


# ---- float32 emulations of the kernels' arithmetic ------------------------------------------------------------------------
def _rsqrt32(v):
  return (1.0 / torch.sqrt(v.to(F32))).to(F32)


def _act(c, y):
  return y * torch.sigmoid(y) if c.silu else y


def emulate_fused(c, x, gamma, beta):
  """gn_fused_kernel: per thread a (lo, hi) pair over its MAXCH chunks, per chunk column over the pixel lanes, per group
  over the columns; mean; centred squares of the live slots the same way; normalise.  x [B * HW, C] float32."""
  GB, S, NT, MC, P = _fused_geom(c)
  B, HW, C, G = c.B, c.HW, c.C, c.G
  cg, e = C // G, epc(c.dt)
  nblk = G // GB
  assert MC * P >= HW and S * e == GB * cg
  slab = torch.zeros(B, MC * P, C, dtype=F32)
  slab[:, :HW] = x.view(B, HW, C)
  live = (torch.arange(MC * P) < HW).view(1, MC, P, 1, 1, 1)
  v = slab.view(B, MC, P, nblk, S, e)                 # thread (pl, cs) of workgroup (b, blk), chunk k
  el = torch.arange(S * e).view(S, e)
  grp = el // cg                                      # group (in the segment) of every element of a chunk column
  is_lo = grp == grp[:, :1]
  n = torch.tensor(float(HW) * float(cg), dtype=F32)

  def reduce_groups(t):                               # t [B, MC, P, nblk, S, e] -> [B, nblk, GB]
    lo = (t * is_lo).sum(dim=5).sum(dim=1)            # [B, P, nblk, S]: the thread's running sums
    hi = (t * ~is_lo).sum(dim=5).sum(dim=1)
    lo, hi = lo.sum(dim=1), hi.sum(dim=1)             # over the pixel lanes: s_tot[c]
    red = torch.zeros(B, nblk, GB, dtype=F32)
    for col in range(S):
      red[:, :, int(grp[col, 0])] += lo[:, :, col]
      if not bool(is_lo[col].all()):
        red[:, :, int(grp[col, 0]) + 1] += hi[:, :, col]
    return red

  mean = reduce_groups(v) / n                         # [B, nblk, GB]
  mu = mean[:, :, grp].view(B, 1, 1, nblk, S, e)      # per element
  d = torch.where(live, v - mu, torch.zeros((), dtype=F32))
  rstd = _rsqrt32(reduce_groups(d * d) / n + torch.tensor(EPS, dtype=F32))
  sc = rstd[:, :, grp].view(B, 1, 1, nblk, S, e) * gamma.view(1, 1, 1, nblk, S, e)
  y = (v - mu) * sc + beta.view(1, 1, 1, nblk, S, e)
  return _act(c, y).reshape(B, MC * P, C)[:, :HW].reshape(B * HW, C).to(c.dt)


def emulate_pair(c, x, gamma, beta):
  """gn_partial_kernel + gn_apply_kernel: sums of x - K and (x - K)^2 per chunk, added over the chunks; dm, var = E - dm^2,
  (x - K) * sc + (beta - dm * sc)."""
  B, HW, C, G = c.B, c.HW, c.C, c.G
  cg = C // G
  nch, ppc, _, _ = pair_geom(c)
  xg = x.view(B, HW, G, cg)
  K = xg[:, :1, :, :1]
  d = xg - K
  t1 = torch.zeros(B, G, dtype=F32)
  t2 = torch.zeros(B, G, dtype=F32)
  for k in range(nch):
    lo, hi = k * ppc, min(HW, (k + 1) * ppc)
    if lo < hi:
      t1 += d[:, lo:hi].sum(dim=(1, 3))
      t2 += (d[:, lo:hi] * d[:, lo:hi]).sum(dim=(1, 3))
  n = torch.tensor(float(HW) * float(cg), dtype=F32)
  dm = t1 / n
  var = torch.clamp(t2 / n - dm * dm, min=0.0)
  rstd = _rsqrt32(var + torch.tensor(EPS, dtype=F32))
  sc = rstd.view(B, 1, G, 1) * gamma.view(1, 1, G, cg)
  sh = beta.view(1, 1, G, cg) - dm.view(B, 1, G, 1) * sc
  return _act(c, d * sc + sh).reshape(B * HW, C).to(c.dt)


def emulate_ln(c, x, gamma, beta):
  """layernorm_kernel: per lane over its pieces, LPR-wide butterfly; mean = s / C; centred squares; rsqrtf."""
  lpr, e = c.form[0], epc(c.dt)
  rows, C = x.shape
  nvec = C // e
  pad = torch.zeros(rows, 8 * lpr * e, dtype=F32)
  pad[:, :C] = x
  pv = pad.view(rows, 8, lpr, e)
  live = (torch.arange(8 * lpr) < nvec).view(1, 8, lpr, 1)
  s = pv.sum(dim=3).sum(dim=1).sum(dim=1, keepdim=True)
  mean = s / torch.tensor(float(C), dtype=F32)
  d = torch.where(live, pv - mean.view(rows, 1, 1, 1), torch.zeros((), dtype=F32))
  q = (d * d).sum(dim=3).sum(dim=1).sum(dim=1, keepdim=True)
  rstd = _rsqrt32(q / torch.tensor(float(C), dtype=F32) + torch.tensor(EPS, dtype=F32))
  return ((x - mean) * rstd * gamma + beta).to(c.dt)


def emulate_ln_out(c, x, gamma, beta):
  """The GEMM's LayerNorm output: mean = sum * (1 / BN), rstd = rsqrtf(sum d^2 * (1 / BN) + eps)."""
  inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(c.C), dtype=F32)
  mean = x.sum(dim=1, keepdim=True) * inv
  d = x - mean
  rstd = _rsqrt32((d * d).sum(dim=1, keepdim=True) * inv + torch.tensor(EPS, dtype=F32))
  return (d * rstd * gamma + beta).to(c.dt)


def emulate_ln_fold(c, x, w_sel, bias):
  """gemm3_kernel.h: mu = s / K, rstd = rsqrtf(max(fma(-mu, mu, q / K), 0) + eps), out = fma(rstd, acc, fma(-rstd mu, cs, b))
  with cs = 1 (one-hot weight rows) and acc = x[m][k(n)]."""
  ik = torch.tensor(1.0, dtype=F32) / torch.tensor(float(c.C), dtype=F32)
  mu = x.sum(dim=1, keepdim=True) * ik
  ex2 = (x * x).sum(dim=1, keepdim=True) * ik
  var = (ex2.to(F64) - mu.to(F64) * mu.to(F64)).to(F32)          # one fma: a single rounding
  r = _rsqrt32(torch.clamp(var, min=0.0) + torch.tensor(EPS, dtype=F32))
  inner = ((-r * mu).to(F64) + bias.to(F64)).to(F32)
  return ((r.to(F64) * x[:, w_sel].to(F64)) + inner.to(F64)).to(F32).to(c.dt)


EMULATE = {"fused": emulate_fused, "pair": emulate_pair, "ln": emulate_ln, "ln_out": emulate_ln_out}


# ---- case matrix ---------------------------------------------------------------------------------------------------
def _fused(dt, C, B, HW, form, G=32, p=4, silu=False):
  return Case("fused", dt, B, HW, C, G, p, 0, silu, False, form)


def fused_cases():
  bf, f = BF, F32
  return [
      # (64, 8): idle lanes (64 % 5), S | 64 (C = 512), straddling (C = 1920, 960) and not, HW < P, HW = 8 P, B % 8 != 0
      _fused(bf, 1280, 16, 16, (1, 5, 64, 8)), _fused(bf, 1280, 16, 96, (1, 5, 64, 8), p=1),
      _fused(bf, 1920, 32, 30, (2, 15, 64, 8)), _fused(bf, 512, 17, 35, (1, 2, 64, 8), silu=True),
      _fused(bf, 512, 16, 7, (1, 2, 64, 8), p=2),
      _fused(f, 320, 33, 35, (2, 5, 64, 8)), _fused(f, 2560, 17, 24, (1, 20, 64, 8), p=3),
      # (64, 16)
      _fused(bf, 2560, 17, 63, (1, 10, 64, 16)), _fused(bf, 1920, 33, 49, (2, 15, 64, 16)),
      _fused(f, 320, 33, 97, (2, 5, 64, 16)), _fused(f, 1920, 17, 49, (1, 15, 64, 16), silu=True),
      _fused(f, 512, 16, 256, (1, 4, 64, 16)),
      # (64, 24)
      _fused(bf, 2560, 33, 110, (1, 10, 64, 24)), _fused(bf, 1280, 32, 210, (1, 5, 64, 24)),
      _fused(f, 2560, 33, 72, (1, 20, 64, 24)), _fused(f, 1920, 33, 82, (1, 15, 64, 24)),
      # (256, 8): GB = 8 (odd cpg = 9), GB = 4, G in {1, 4, 64}
      _fused(bf, 320, 3, 35, (4, 5, 256, 8)), _fused(bf, 960, 3, 64, (4, 15, 256, 8)),
      _fused(bf, 960, 4, 132, (4, 15, 256, 8), p=3, silu=True), _fused(bf, 288, 2, 20, (8, 9, 256, 8)),
      _fused(bf, 960, 3, 136, (4, 15, 256, 8)),
      _fused(bf, 64, 13, 37, (1, 8, 256, 8), G=1), _fused(bf, 64, 3, 129, (1, 2, 256, 8), G=4),
      _fused(bf, 640, 3, 70, (4, 5, 256, 8), G=64),
      _fused(f, 320, 3, 35, (2, 5, 256, 8)), _fused(f, 960, 3, 64, (2, 15, 256, 8)), _fused(f, 128, 3, 19, (1, 1, 256, 8)),
      _fused(f, 32, 7, 37, (1, 8, 256, 8), G=1), _fused(f, 640, 3, 70, (2, 5, 256, 8), G=64),
      # (256, 16)
      _fused(bf, 960, 3, 143, (4, 15, 256, 16)), _fused(bf, 960, 5, 256, (4, 15, 256, 16)),
      _fused(bf, 960, 6, 272, (4, 15, 256, 16)),
      _fused(f, 960, 3, 143, (2, 15, 256, 16)), _fused(f, 2560, 2, 100, (1, 20, 256, 16), silu=True),
      # (512, 8)
      _fused(bf, 2560, 6, 401, (1, 10, 512, 8)), _fused(bf, 2560, 6, 408, (1, 10, 512, 8)),
      _fused(f, 2560, 3, 193, (1, 20, 512, 8)), _fused(f, 2560, 3, 200, (1, 20, 512, 8)),
      # (512, 16)
      _fused(bf, 320, 6, 899, (4, 5, 512, 16)), _fused(bf, 320, 7, 1024, (4, 5, 512, 16)), _fused(bf, 320, 11, 1632, (4, 5, 512, 16)),
      _fused(f, 320, 6, 899, (2, 5, 512, 16)), _fused(f, 960, 5, 273, (2, 15, 512, 16)),
      _fused(f, 960, 6, 544, (2, 15, 512, 16)),
      # (1024, 8): floor(1024 / S) must exceed 2 floor(512 / S) -- S = 9 (bf16, odd cpg, GB = 8) and S = 20
      _fused(bf, 288, 11, 897, (8, 9, 1024, 8)), _fused(bf, 288, 11, 904, (8, 9, 1024, 8)),
      _fused(f, 2560, 6, 401, (1, 20, 1024, 8)), _fused(f, 2560, 6, 408, (1, 20, 1024, 8)),
      # (1024, 16)
      _fused(bf, 960, 11, 552, (4, 15, 1024, 16)), _fused(bf, 960, 11, 560, (4, 15, 1024, 16)),
      _fused(f, 960, 11, 552, (2, 15, 1024, 16)), _fused(f, 960, 11, 1088, (2, 15, 1024, 16)),
  ]


def _pair(dt, C, B, HW, nchunks, G=32, p=4, silu=False, pilot=False):
  c = Case("pair", dt, B, HW, C, G, p, nchunks, silu, pilot, ())
  return c._replace(form=(pair_geom(c)[0],))


def pair_cases():
  out = []
  for dt in (BF, F32):
    big = 2560 if dt == BF else 1280                  # nvec >= 256
    out += [
        _pair(dt, 320, 3, 45, 1), _pair(dt, 320, 3, 215, 3), _pair(dt, 320, 3, 215, 7, p=2),
        _pair(dt, 320, 7, 419, 128),                  # more chunks than ceil(HW / ppc): ppc = 4, 105 live chunks
        _pair(dt, 320, 3, 1099, 0), _pair(dt, 320, 1, 77, 3, p=1), _pair(dt, 320, 3, 215, 7, silu=True),
        _pair(dt, big, 3, 215, 7), _pair(dt, big, 6, 419, 0),
        _pair(dt, 640, 3, 215, 3, G=64), _pair(dt, 320, 3, 113, 7, G=8),
        _pair(dt, 320, 3, 215, 3, pilot=True),
    ]
  out += [_pair(BF, 128, 3, 215, 7), _pair(BF, 128, 1, 77, 1)]    # cpg = 4 < 8: the fused kernel refuses
  return out


LN_WIDTHS = {BF: {4: 64, 8: 328, 16: 768, 32: 1288, 64: 2568}, F32: {4: 64, 8: 160, 16: 320, 32: 772, 64: 1284}}


def ln_cases():
  out = []
  for dt in (BF, F32):
    for lpr, C in LN_WIDTHS[dt].items():
      blk = 4 * (64 // lpr)
      need = -(-C // (8 * MAX_LAUNCHES))              # rows below this cannot sweep C columns in 24 launches
      for rows in sorted({1, blk - 1, blk + 1, 77}):
        if rows >= need:
          out.append(Case("ln", dt, rows, 1, C, 1, 4 if rows % 2 else 3, 0, False, False, (lpr,)))
  return out


def ln_out_cases():
  return [Case("ln_out", dt, M, 1, 320, 1, 4, 0, False, False, ()) for dt in (BF, F32) for M in (1, 127, 129, 300)]


def ln_fold_cases():
  return [Case("ln_fold", BF, M, 1, 320, 1, 4, 0, False, False, (tile, deal))
          for tile in (13, 14) for deal, M in ((0, 300), (1, 129))]


def all_cases():
  return fused_cases() + pair_cases() + ln_cases() + ln_out_cases() + ln_fold_cases()


def case_id(c):
  s = f"{c.kind}-{DTN[c.dt]}-B{c.B}-HW{c.HW}-C{c.C}-G{c.G}-p{c.p}"
  if c.kind == "fused":
    s += "-form" + ".".join(str(v) for v in c.form)
  elif c.kind == "pair":
    s += f"-nchunks{c.form[0]}" + ("-default" if not c.nchunks else "")
  elif c.kind == "ln":
    s += f"-lpr{c.form[0]}"
  elif c.kind == "ln_fold":
    s += f"-tile{c.form[0]}-deal{c.form[1]}"
  return s + ("-silu" if c.silu else "") + ("-pilot" if c.pilot else "")
