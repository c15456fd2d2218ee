"""Probes for the sampler kernels (csrc/sampler.hip): the update of a sampling step in its 14 instantiations, the forward
diffusion and the Philox kernels.  Case lists placed on the kernels' own edges, input builders, a reference written out
from include/ldm_hip.h, and an index-arithmetic model of the two work decompositions (one element per thread, four
elements per thread) with switchable faults (a plain module, imported by test_sampler_probes_cpu.py and
test_zz_sampler_accounting_gpu.py; torch on the CPU only).

Every probe is exact (gate: torch.equal, no tolerance)
  Data are integer position codes mult * ((i + 37 a) % P) of element i of array a (eps_u, eps_c, xt, the four ring
  slots, z0, every Q row, every eta-noise row).  P is a prime no neighbour distance of a case is a multiple of (one
  element, one quad, one pixel, one sample, one grid pass: the CPU test asserts it), so an element never carries the
  code of such a neighbour, nor that of the same element of another array.
    selection probes   P = 8191, mult = 1.  The table rows make an output ONE input element:
                       (c1, c2, a_prev, sigma) = (1, 0, 1, 0) -> xt;  (0, -1, 0, 0) -> e' (sa = 0, sb = 1);
                       (0, 0, 0, 1) -> the eta noise (sb = sqrtf(0) = 0);  gs or gtab[idx] in {0, 1} -> eps_u / eps_c;
                       a one-hot weight row -> ring slot (idx + m) & 3;  mask in {0, 1} with q_coef (1, 0) / (0, 1)
                       -> xt', z0 or Q[idx - 1].  ldm_q_sample: sqrt_ac[t] = 2^-(t % 8) and sqrt_1m_ac = 0 (or the
                       other way round), t distinct per sample with -1 and num_steps + 5 among them.
    census probes      P = 251, mult = 24: c1 = 2, c2 = 4, a_prev in {0, 1}, gs = 3, mask in {0, 0.5, 1}, q_coef (2, 1),
                       weights (1, 2, -4, 8); every eps and ring value a multiple of 24, so the /2, /12 and /24 of the
                       Adams-Bashforth rows are exact.  The inversion has a_prev = 1 (sa = 1, sb = 0) and c1 = 2.
  Every intermediate of the header's formulas is then an integer or a multiple of 1/2 (2^-7 in q_sample) of magnitude
  below 2^24 units, the same in float32 in any evaluation order, with or without fma contraction: `reference` hands
  every intermediate (and the sum of the magnitudes of the terms of every sum) to a tracker, and the CPU test asserts
  this for every case instead of assuming it.
  Drawn noise: a launch takes the drawn value with weight exactly 1 and everything else with weight exactly 0
  (sigma = 1, a_prev = c1 = c2 = 0 for eta; mask = 1, q_coef (0, 1) for Q), so the output must equal, bit for bit, what
  ldm_normal_fill gives for stream ETA + idx / Q + idx - 1 (first_sample_index = 5).  ldm_normal_fill is tied to
  ldm_philox_u32 and that, exactly, to tests/philox_ref.py at the same shapes.  On the CPU the draws are stood in for
  by the integers (Philox word >> 12), so the model and its faults run on the same counters.
  x_unet_out (float32 and bf16): both halves must equal the round-to-nearest-even conversion of xt_out.

Guards
  Every operand is a view into a NaN-filled buffer and every output has NaN canaries before and after it.  What the
  header says is not read holds NaN: every row of coef, gtab, q_coef and weights other than the launch's, the weight
  entries beyond j, the ring slots beyond j and the slot written, the unconditional half and gtab in the
  conditional-only form, z0 / Q / q_coef at idx = 0, the sigma column of the non-DDIM entries.  Ring slots not written
  keep their bits; pred_x0_out and the slot written hold the unblended step's values; *index moves only with dec_index.

Faults (FAULTS): references of subtly wrong kernels, each a switch of `model`.  `mutation_applies` names the cases a
fault cannot show in; in every other case it must change an output (test_sampler_probes_cpu.py).

RESULTS (MI355X, first run)
  test_zz_sampler_accounting_gpu.py: 515 tests in 3.8 s of wall time (pytest's total).  381 probe cases, one launch
  each (346 updates over the 14 instantiations, 35 of ldm_q_sample / ldm_q_sample_rng / ldm_normal_fill /
  ldm_philox_u32; the largest four take 0.12 - 0.14 s each, building their 1 M-element operands on the host included):
  every probe equal, no canary touched, no input written, no ring slot outside idx & 3 changed.  ldm_normal_fill
  against the float64 Box-Muller of the device's own words: at most 1.4e-5, bound 5.6e-5.  All 124 rejected calls
  raised their entry's message and wrote nothing; in place gave the bits of out of place for all 9 update entries.
  No kernel and no host check needed a change.
"""
from types import SimpleNamespace as NS

import numpy as np
import torch

import philox_ref as R

F32, BF, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
NAN = float("nan")
DTN = {None: "noxu", F32: "f32", BF: "bf16"}

# ---- the numbers of csrc/sampler.hip (the CPU test reads them back from the source text) ------------------------------
BLOCK, CAP, WIDE = 256, 1024, 4
SEED, FIRST = (1 << 32) + 7, 5                       # both key words in use; first_sample_index != 0
N_ROWS = 12                                          # rows of coef / gtab / q_coef / weights
Q_STEPS = 13                                         # num_steps of the q_sample probes
LIMIT = 2.0 ** 24

UPDATE_ENTRIES = ("ddim", "ddim_masked", "ddim_rng", "plms", "plms_rng", "ms", "ms_rng", "sched", "invert")
FILL_ENTRIES = ("q_sample", "q_sample_rng", "normal_fill", "philox_u32")
# the template arguments behind update_launch's switch: (body, Hist, Scale, Rng, Blend)
INSTANTIATIONS = {
    ("scalar", "ddim", "arg", False, True), ("scalar", "ddim", "arg", False, False),
    ("wide", "ddim", "arg", True, True),
    ("wide", "ab", "arg", False, True), ("wide", "ab", "arg", False, False), ("wide", "ab", "arg", True, True),
    ("wide", "table", "arg", False, True), ("wide", "table", "arg", True, True),
    ("wide", "table", "table", False, True), ("wide", "table", "table", True, True),
    ("wide", "table", "cond", False, True), ("wide", "table", "cond", True, True),
    ("wide", "invert", "arg", False, False), ("wide", "invert", "cond", False, False),
}


def form(c):
  """(body, Hist, Scale, Rng, Blend) of the kernel update_launch picks for case `c`."""
  e = c.entry
  if e in ("ddim", "ddim_masked"):
    return ("scalar", "ddim", "arg", False, c.blend)
  if e == "ddim_rng":
    return ("wide", "ddim", "arg", True, True)
  if e == "plms":
    return ("wide", "ab", "arg", False, c.blend)
  if e == "plms_rng":
    return ("wide", "ab", "arg", True, True)
  if e in ("ms", "ms_rng"):
    return ("wide", "table", "arg", e == "ms_rng", True)
  if e == "sched":
    return ("wide", "table", "table" if c.guided else "cond", c.rng, True)
  assert e == "invert"
  return ("wide", "invert", "arg" if c.guided else "cond", False, False)


def width(c):
  if c.entry in UPDATE_ENTRIES:
    return 1 if form(c)[0] == "scalar" else WIDE
  return 1 if c.entry == "q_sample" else WIDE


def passes(c):
  """(grid-stride passes, workgroups) of case `c` (common.h grid_for, cap 1024)."""
  items = c.B * c.n // width(c)
  grid = max(1, min(CAP, -(-items // BLOCK)))
  return -(-items // (grid * BLOCK)), grid


def has_hist(c):
  return c.entry in ("plms", "plms_rng", "ms", "ms_rng") or (c.entry == "sched" and c.weights)


def has_weights(c):
  return c.entry in ("ms", "ms_rng") or (c.entry == "sched" and c.weights)


def is_ddim(c):
  return c.entry in ("ddim", "ddim_masked", "ddim_rng")


def order(c):
  d = c.start - c.idx
  return max(0, min(3, d)) if has_hist(c) else 0


def blend_on(c):
  return c.blend and c.idx >= 1


# ============================================================================================================
# cases
# ============================================================================================================
def _u(entry, probe, n=12, ch=4, idx=1, B=3, xd=F32, blend=False, mask="sel", qc=(1, 0), gs=1, a_prev=1, clip=0,
       d=0, hot=0, pitch=16, qs=1, ns=1, guided=True, rng=False, weights=True, pred=True, dec=True, alias=False, tag=""):
  """One update launch.  qs / ns: q_index_stride / noise_index_stride as 0, 1 (= B n) or 2 (= B n + 4); d = start - idx;
  hot: the one-hot weight (selection probes of the table entries)."""
  c = NS(entry=entry, probe=probe, n=n, ch=ch, idx=idx, B=B, xd=xd, blend=bool(blend), mask=mask, qc=qc, gs=gs,
         a_prev=a_prev, clip=clip, start=idx + d, hot=hot, pitch=pitch, guided=bool(guided), rng=bool(rng),
         weights=bool(weights), pred=bool(pred), dec=bool(dec), alias=bool(alias))
  total = B * n
  c.q_stride = (0, total, total + 4)[qs]
  c.noise_stride = (0, total, total + 4)[ns]
  c.P, c.mult = (251, 24) if probe.startswith("census") else (8191, 1)
  if entry == "ddim_masked":
    c.blend = True
  if entry == "invert" or entry == "ddim":
    c.blend = False
  if entry == "sched" and not c.guided:
    c.gs = 1
  c.hot = min(hot, order(c))
  parts = [entry, probe, f"B{B}n{n}c{ch}", f"i{idx}", DTN[xd]]
  if entry == "sched":
    parts.append(("g" if c.guided else "c") + ("r" if c.rng else "t") + ("w" if c.weights else "n"))
  if entry == "invert":
    parts.append("g" if c.guided else "c")
  if has_hist(c):
    parts.append(f"d{d}")
  if has_weights(c):
    parts.append(f"h{c.hot}p{pitch}")
  if c.blend:
    parts.append(f"m{mask}q{qc[0]}{qc[1]}s{qs}")
  if is_ddim(c) and entry != "ddim_rng":
    parts.append(f"ns{ns}")
  parts.append(f"gs{c.gs}a{a_prev}" + ("clip" if clip else "") + ("" if pred else "-nopred") + ("" if dec else "-nodec") +
               ("-inplace" if alias else ""))
  if tag:
    parts.append(tag)
  c.id = "-".join(parts)
  return c


# (entry, the keywords that pick the instantiation, whether it can blend)
VARIANTS = [
    ("ddim", {}, False), ("ddim_masked", {}, True), ("ddim_rng", {}, True), ("plms", {}, True), ("plms_rng", {}, True),
    ("ms", {}, True), ("ms_rng", {}, True),
    ("sched", dict(guided=1, rng=0), True), ("sched", dict(guided=1, rng=1), True),
    ("sched", dict(guided=0, rng=0), True), ("sched", dict(guided=0, rng=1), True),
    ("sched", dict(guided=1, rng=0, weights=0), True), ("sched", dict(guided=0, rng=1, weights=0), True),
    ("invert", dict(guided=1), False), ("invert", dict(guided=0), False),
]
BLEND_SHAPES = ((12, 1), (12, 2), (12, 3), (12, 4), (12, 6), (24, 8), (1020, 3), (1020, 6), (1028, 2))
ORDERS = (-1, 0, 1, 2, 3, 7)
ONE_PASS = {1: BLOCK * CAP, WIDE: BLOCK * CAP * WIDE}


def update_cases():
  out = []
  for v, (entry, kw, can_blend) in enumerate(VARIANTS):
    K = lambda probe, **k: out.append(_u(entry, probe, **{**kw, **k}))
    cond = entry in ("sched", "invert") and not kw.get("guided", 1)
    inv = entry == "invert"
    rng = entry.endswith("_rng") or bool(kw.get("rng"))
    hist = entry in ("plms", "plms_rng", "ms", "ms_rng") or (entry == "sched" and kw.get("weights", 1))
    odd = entry in ("ddim", "ddim_masked")                                   # the scalar body takes any n
    # the four sample lengths, both x_unet types, idx of every residue and 0, the halves of eps_all
    K("xt", n=12, idx=1, xd=F32, gs=1)
    K("census" if inv else "eps", n=1020, idx=2, xd=BF, gs=1, dec=0)
    if not cond:
      K("census" if inv else "eps", n=1028, idx=3, xd=F32, gs=0)
    K("census", n=4, idx=0, xd=BF, gs=3, a_prev=1 if inv else 0, blend=can_blend)      # idx = 0: the blend is skipped
    K("census", n=1028, idx=5, xd=BF, gs=3, a_prev=1, alias=1, blend=can_blend, mask="mix", qc=(2, 0 if rng else 1), d=1)
    K("census", n=12, idx=4, xd=None, gs=3, a_prev=1 if inv else 0, pred=0, dec=0, d=2)
    K("census", n=1020, idx=7, xd=F32, gs=3, a_prev=1 if inv else 0, blend=can_blend, mask="mix", qc=(2, 0 if rng else 1),
      d=3, qs=2, pitch=20)
    if odd:
      K("xt", n=7, idx=1, ch=7, xd=F32)
      K("census", n=1021, idx=2, ch=1, xd=BF, gs=3, a_prev=0, mask="mix", qc=(2, 1))
      for ns in (0, 1, 2):
        K("noise", n=12, idx=(3, 1, 6)[ns], ns=ns, xd=(F32, BF, None)[ns])
        K("census_sigma", n=1020, idx=(2, 5, 3)[ns], ns=ns, gs=3, a_prev=0, clip=ns == 1, mask="mix", qc=(2, 1))
      K("census", n=12, idx=1, gs=3, a_prev=1, clip=1)
    if entry == "ddim_rng":
      for n in (4, 12, 1020, 1028):
        K("draw_eta", n=n, idx=(0, 1, 6, 3)[n % 4 if n < 1000 else 2 + (n == 1028)], xd=BF if n == 12 else F32)
      K("draw_eta", n=1028, idx=2, blend=1, qc=(1, 0))
      K("census", n=12, idx=1, gs=3, a_prev=1, clip=1)
    if can_blend:
      # the mask broadcast for every channel count, z0 / Q selected by q_coef; the three Q strides
      for s, (n, ch) in enumerate(BLEND_SHAPES):
        sel_q = s % 2 == 1
        K("draw_q" if (rng and sel_q) else "xt", n=n, ch=ch, idx=1 + (s + v) % 5, blend=1, qc=(0, 1) if sel_q else (1, 0),
          qs=(s // 2) % 3, xd=(F32, BF)[s % 2], gs=s % 2 if not cond else 1)
      if rng:
        K("draw_q", n=4, idx=1, blend=1, qc=(0, 1))
        K("draw_q", n=1028, idx=6, blend=1, qc=(0, 1), ch=4, xd=BF)
    if hist:
      # start - idx over every order and both clamps, every ring residue, both pitches, every one-hot weight
      for k, d in enumerate(ORDERS):
        K("census", n=12, idx=(k + v) % 4 + (4 if d == -1 else 0), d=d, gs=3, a_prev=k % 2, pitch=(16, 20)[k % 2],
          xd=(F32, BF)[k % 2], blend=can_blend and k % 3 == 0, mask="mix", qc=(2, 0 if rng else 1))
      if entry not in ("plms", "plms_rng"):
        for hot in range(4):
          K("eps", n=12, idx=hot + 1, d=3, hot=hot, gs=1, pitch=(20, 16)[hot % 2])
          K("eps", n=1028, idx=7 - hot, d=max(hot, 1), hot=hot, gs=0 if not cond else 1, pitch=(16, 20)[hot % 2], xd=BF)
  # one pass exactly, and one quad (one element) past it, per body
  out.append(_u("ddim_masked", "census", B=2, n=ONE_PASS[1] // 2, ch=4, idx=3, gs=3, a_prev=0, mask="mix", qc=(2, 1),
                xd=BF, tag="one-pass"))
  out.append(_u("ddim_masked", "census", B=5, n=(ONE_PASS[1] + 1) // 5, ch=1, idx=2, gs=3, a_prev=0, mask="mix", qc=(2, 1),
                xd=F32, alias=1, tag="past-one-pass"))
  out.append(_u("ms", "census", B=2, n=ONE_PASS[WIDE] // 2, ch=4, idx=3, d=2, gs=3, a_prev=0, blend=1, mask="mix", qc=(2, 1),
                xd=F32, tag="one-pass"))
  out.append(_u("ms", "census", B=5, n=(ONE_PASS[WIDE] + 4) // 5, ch=4, idx=2, d=3, gs=3, a_prev=0, blend=1, mask="mix",
                qc=(2, 1), xd=BF, alias=1, pitch=20, tag="past-one-pass"))
  out.append(_u("ddim_rng", "draw_eta", B=5, n=(ONE_PASS[WIDE] + 4) // 5, ch=4, idx=1, xd=None, pred=0, tag="past-one-pass"))
  return out


def _f(entry, probe="x", B=3, n=12, xd=F32, ns=1, use_index=True, idx=2, stream=R.Q_STREAM + 4, tag=""):
  c = NS(entry=entry, probe=probe, B=B, n=n, xd=xd, use_index=bool(use_index), idx=idx, stream=stream, ch=1)
  c.noise_stride = (0, B * n, B * n + 4)[ns]
  c.P, c.mult = 8191, 1
  c.id = "-".join([entry, probe, f"B{B}n{n}", DTN[xd]] + ([f"i{idx}ns{ns}" if use_index else "noindex"] if entry == "q_sample"
                                                         else []) + ([tag] if tag else []))
  return c


def fill_cases():
  out = []
  for k, n in enumerate((4, 12, 1020, 1028)):
    out.append(_f("q_sample", "x", n=n, xd=(F32, BF)[k % 2], ns=k % 3, idx=k + 1))
    out.append(_f("q_sample", "noise", n=n, xd=(BF, None)[k % 2], ns=(k + 1) % 3, idx=k, use_index=k != 3))
    out.append(_f("q_sample_rng", "x", n=n, xd=(F32, BF)[k % 2]))
    out.append(_f("q_sample_rng", "noise", n=n, xd=(BF, None, F32)[k % 3], stream=R.Q_STREAM + k))
    out.append(_f("normal_fill", "noise", n=n, xd=(None, F32, BF)[k % 3], stream=R.ETA_STREAM + k))
    out.append(_f("philox_u32", "noise", n=n, xd=None, stream=R.XT_STREAM + 3 * k))
  out.append(_f("q_sample", "x", n=7, xd=F32, ns=2))
  out.append(_f("q_sample", "noise", n=1021, xd=BF, ns=0))
  for past in (0, 1):
    tag = "past-one-pass" if past else "one-pass"
    out.append(_f("q_sample", "x", B=5 if past else 2, n=(ONE_PASS[1] + 1) // 5 if past else ONE_PASS[1] // 2, xd=BF, tag=tag))
    for e, probe in (("q_sample_rng", "noise"), ("normal_fill", "noise"), ("philox_u32", "noise")):
      out.append(_f(e, probe, B=5 if past else 2, n=(ONE_PASS[WIDE] + 4) // 5 if past else ONE_PASS[WIDE] // 2,
                    xd=None if e == "philox_u32" else (F32, BF)[past], tag=tag))
  out.append(_f("q_sample_rng", "x", B=5, n=(ONE_PASS[WIDE] + 4) // 5, xd=F32, tag="past-one-pass"))
  return out


# ============================================================================================================
# inputs
# ============================================================================================================
A_EU, A_EC, A_XT, A_RING, A_Z0, A_Q, A_ETA = 0, 1, 2, 3, 7, 8, 8 + N_ROWS


def codes(c, a, total):
  """The position codes of array `a`: float64 [total]."""
  return (c.mult * ((torch.arange(total, dtype=I64) + 37 * a) % c.P)).to(F64)


def surrogate_draws(c):
  """stream -> float64 [B n]: the integer stand-in of the draws of one stream on the CPU (Philox word >> 12)."""
  def f(stream):
    return torch.from_numpy((R.words(SEED, FIRST, stream, c.B, c.n) >> np.uint32(12)).astype(np.float64)).reshape(-1)
  return f


def _table(total, stride, rows, last, fn):
  """A [rows] table of [total] rows `stride` apart in a NaN-filled flat buffer; row `last` is written last (stride 0:
  it is the one buffer)."""
  flat = torch.full(((rows - 1) * stride + total,), NAN, dtype=F64)
  for r in list(range(rows)) + [last]:
    flat[r * stride:r * stride + total] = fn(r)
  return flat


def mask_values(c):
  """[B, n / ch]: cell (b, p) takes value (b + p + p // 2) % 2 of {0, 1} (sel) or % 3 of {0, 0.5, 1} (mix)."""
  npix = c.n // c.ch
  b, p = torch.meshgrid(torch.arange(c.B), torch.arange(npix), indexing="ij")
  s = b + p + p // 2
  return (s % 2).to(F64) if c.mask == "sel" else torch.tensor([0.0, 0.5, 1.0], dtype=F64)[s % 3]


def coef_row(c):
  if c.probe in ("xt", "draw_q"):
    row = [1.0, 0.0, 1.0, 0.0]
  elif c.probe == "eps":
    row = [0.0, -1.0, 0.0, 0.0]
  elif c.probe in ("noise", "draw_eta"):
    row = [0.0, 0.0, 0.0, 1.0]
  elif c.probe == "census_sigma":
    row = [2.0, 4.0, 0.0, 1.0]
  else:
    row = [2.0, 4.0, float(c.a_prev), 0.0]
  if not is_ddim(c):
    row[3] = NAN                                              # the sigma column is not read
  return row


def weight_row(c):
  j = order(c)
  if c.probe.startswith("census"):
    return [1.0, 2.0, -4.0, 8.0][:j + 1]
  return [1.0 if m == c.hot else 0.0 for m in range(j + 1)]


def build(c, draws=None):
  """The operands of one launch: float64 / int tensors on the CPU, NaN wherever the launch must not read."""
  draws = draws or surrogate_draws(c)
  total = c.B * c.n
  if c.entry in FILL_ENTRIES:
    return _build_fill(c, draws, total)
  f = form(c)
  p = NS(idx=c.idx, start=c.start, gs=1.0 if c.entry == "sched" else float(c.gs))   # (what ldm_cfg_sched_update passes on)
  p.eps = torch.cat([codes(c, A_EU, total), codes(c, A_EC, total)])
  if f[2] == "cond":
    p.eps[:total] = NAN
  p.xt = codes(c, A_XT, total)
  p.coef = torch.full((N_ROWS * 4,), NAN, dtype=F64)
  p.coef[c.idx * 4:c.idx * 4 + 4] = torch.tensor(coef_row(c), dtype=F64)
  p.gtab = None
  if c.entry == "sched":
    p.gtab = torch.full((N_ROWS,), NAN, dtype=F64)
    if c.guided:
      p.gtab[c.idx] = float(c.gs)
  p.ring = p.weights = None
  j = order(c)
  if has_hist(c):
    p.ring = torch.full((4 * total,), NAN, dtype=F64)
    for m in range(1, j + 1):
      s = (c.idx + m) & 3
      p.ring[s * total:(s + 1) * total] = codes(c, A_RING + s, total)
  if has_weights(c):
    p.weights = torch.full((N_ROWS * c.pitch,), NAN, dtype=F64)
    o = c.idx * c.pitch + 4 * j
    p.weights[o:o + j + 1] = torch.tensor(weight_row(c), dtype=F64)
  p.noise = None
  if c.entry in ("ddim", "ddim_masked") and c.probe in ("noise", "census_sigma"):
    p.noise = _table(total, c.noise_stride, N_ROWS, c.idx, lambda r: codes(c, A_ETA + r, total))
  p.z0 = p.mask = p.q = p.qcoef = None
  if c.blend:
    on = c.idx >= 1
    p.z0 = codes(c, A_Z0, total) if on else torch.full((total,), NAN, dtype=F64)
    p.mask = mask_values(c).reshape(-1)
    p.qcoef = torch.full((N_ROWS * 2,), NAN, dtype=F64)
    if on:
      p.qcoef[(c.idx - 1) * 2:(c.idx - 1) * 2 + 2] = torch.tensor(c.qc, dtype=F64)
    if not f[3]:
      p.q = _table(total, c.q_stride, N_ROWS, c.idx - 1, lambda r: codes(c, A_Q + r, total)) if on else \
          torch.full(((N_ROWS - 1) * c.q_stride + total,), NAN, dtype=F64)
  p.eta_draw = draws(R.ETA_STREAM + c.idx) if c.entry == "ddim_rng" and coef_row(c)[3] != 0 else None
  p.q_draw = draws(R.Q_STREAM + c.idx - 1) if f[3] and blend_on(c) else None
  return p


def q_times(B):
  return torch.tensor(([-1, Q_STEPS + 5, 3, 6, 9] if B > 1 else [Q_STEPS + 5])[:B], dtype=I64)


def _build_fill(c, draws, total):
  p = NS(idx=c.idx, stream=c.stream)
  if c.entry in ("q_sample", "q_sample_rng"):
    p.x0 = codes(c, A_XT, total)
    p.t = q_times(c.B)
    scale = torch.pow(torch.tensor(2.0, dtype=F64), -(torch.arange(Q_STEPS) % 8).to(F64))
    zero = torch.zeros(Q_STEPS, dtype=F64)
    p.sac, p.s1m = (scale, zero) if c.probe == "x" else (zero, scale)
  if c.entry == "q_sample":
    rows = N_ROWS if c.use_index else 1
    p.noise = _table(total, c.noise_stride if c.use_index else 0, rows, c.idx if c.use_index else 0,
                     lambda r: codes(c, A_ETA + r, total))
  if c.entry in ("q_sample_rng", "normal_fill", "philox_u32"):
    p.draw = draws(c.stream)
  return p


# ============================================================================================================
# the reference, written out from include/ldm_hip.h (float64, whole arrays, no decomposition)
# ============================================================================================================
class Tracker:
  """Collects every intermediate of `reference`: the largest magnitude and whether all are multiples of `unit`."""

  def __init__(self, unit):
    self.unit, self.worst, self.dyadic = unit, 0.0, True

  def __call__(self, v, bound=None):
    t = torch.as_tensor(v, dtype=F64)
    t = t[~torch.isnan(t)]
    if t.numel():
      s = t / self.unit
      self.dyadic = self.dyadic and bool((s == s.round()).all())
      self.worst = max(self.worst, float(s.abs().max()))
    if bound is not None:
      self.worst = max(self.worst, float(torch.as_tensor(bound, dtype=F64).max()) / self.unit)
    return v


def _no_track(v, bound=None):
  return v


def reference(c, p, track=None):
  """The outputs of one launch by the header's formulas: NS(xt_out, pred_x0, ring, x_unet, index), float64 (x_unet
  rounded to its type).  Draws enter as p.eta_draw / p.q_draw / p.draw and are not tracked (weight exactly 0 or 1)."""
  T = track or _no_track
  total = c.B * c.n
  if c.entry in FILL_ENTRIES:
    return _reference_fill(c, p, T, total)
  i = c.idx
  c1, c2, a_prev, sigma = [float(v) for v in p.coef[4 * i:4 * i + 4]]
  eu, ec = p.eps[:total], p.eps[total:]
  f = form(c)
  if f[2] == "cond":
    e_i = ec
  else:
    gs = float(p.gtab[i]) if c.entry == "sched" else p.gs
    e_i = T(eu + T(gs * T(ec - eu)), eu.abs() + abs(gs) * (ec.abs() + eu.abs()))
  j = order(c)
  e = [e_i] + [p.ring[((i + m) & 3) * total:(((i + m) & 3) + 1) * total] for m in range(1, j + 1)]
  if c.entry in ("plms", "plms_rng"):
    num, den = (((1,), 1), ((3, -1), 2), ((23, -16, 5), 12), ((55, -59, 37, -9), 24))[j]
    acc = sum(w * v for w, v in zip(num, e))
    ep = T(T(acc, sum(abs(w) * v.abs() for w, v in zip(num, e))) / den)
  elif has_weights(c):
    w = [float(v) for v in p.weights[i * c.pitch + 4 * j:i * c.pitch + 4 * j + j + 1]]
    ep = T(w[0] * e[0])
    for m in range(1, j + 1):
      ep = T(ep + T(w[m] * e[m]))
    T(0, sum(abs(wm) * v.abs() for wm, v in zip(w, e)))
  else:
    ep = e_i
  x = p.xt
  if c.entry == "invert":
    sa, sb = np.sqrt(a_prev), np.sqrt(1 - a_prev)
    x0 = T(T(x - T(sb * ep), x.abs() + sb * ep.abs()) / sa)
    o = T(T(x0 + T(c2 * ep), x0.abs() + abs(c2) * ep.abs()) / c1)
  else:
    x0 = T(T(c1 * x) - T(c2 * ep), abs(c1) * x.abs() + abs(c2) * ep.abs())
    if is_ddim(c):
      if c.clip:
        x0 = x0.clamp(-1, 1)
      sa, sb = np.sqrt(a_prev), np.sqrt(1 - a_prev - sigma * sigma)
      o = T(T(sa * x0) + T(sb * ep), sa * x0.abs() + sb * ep.abs())
      if c.entry == "ddim_rng":
        if sigma != 0:
          o = o + p.eta_draw * sigma                       # (o is exactly 0 here: coef_row)
      elif p.noise is not None:
        nz = p.noise[i * c.noise_stride:i * c.noise_stride + total]
        o = T(o + T(nz * sigma), o.abs() + nz.abs() * sigma)
    else:
      sa, sb = np.sqrt(a_prev), np.sqrt(1 - a_prev)
      o = T(T(sa * x0) + T(sb * ep), sa * x0.abs() + sb * ep.abs())
  if blend_on(c):
    qa, qb = [float(v) for v in p.qcoef[2 * (i - 1):2 * (i - 1) + 2]]
    m = p.mask.view(c.B, c.n // c.ch, 1).expand(c.B, c.n // c.ch, c.ch).reshape(-1)
    if f[3]:
      qs = T(qa * p.z0) + qb * p.q_draw                     # (qb is 0, or qa is 0 and qb is 1)
    else:
      qn = p.q[(i - 1) * c.q_stride:(i - 1) * c.q_stride + total]
      qs = T(T(qa * p.z0) + T(qb * qn), abs(qa) * p.z0.abs() + abs(qb) * qn.abs())
    if track is not None and not f[3]:
      T(m * qs)
      T((1 - m) * o)
    o = m * qs + (1 - m) * o
    if track is not None and p.q_draw is None:
      T(o, m * qs.abs() + (1 - m) * o.abs())
  out = NS(xt_out=o, pred_x0=x0 if c.pred else None, ring=None, index=i - (1 if c.dec else 0))
  if has_hist(c):
    out.ring = p.ring.clone()
    out.ring[(i & 3) * total:((i & 3) + 1) * total] = e_i
  out.x_unet = None if c.xd is None else torch.cat([o, o]).to(F32).to(c.xd).to(F64)
  return out


def _reference_fill(c, p, T, total):
  if c.entry in ("normal_fill", "philox_u32"):
    o = p.draw
  else:
    tc = p.t.clamp(0, Q_STEPS - 1)
    sa = p.sac[tc][:, None].expand(c.B, c.n).reshape(-1)
    sb = p.s1m[tc][:, None].expand(c.B, c.n).reshape(-1)
    if c.entry == "q_sample":
      off = p.idx * c.noise_stride if c.use_index else 0
      nz = p.noise[off:off + total]
      o = T(T(sa * p.x0) + T(sb * nz))
    else:
      o = T(sa * p.x0) + sb * p.draw                         # (sb is 0, or sa is 0 and sb a power of two)
  xu = None if c.xd is None else torch.cat([o, o]).to(F32).to(c.xd).to(F64)
  return NS(xt_out=o, pred_x0=None, ring=None, index=None, x_unet=xu)


# ============================================================================================================
# the model: the kernels' index arithmetic, with faults
# ============================================================================================================
FAULTS = ("drop_last", "skip_second_pass", "overlap_second_pass", "xunet_half_at_n", "xunet_from_x0", "mask_quad_base",
          "mask_no_sample", "b_per_block", "ring_slot_plus1", "ring_stores_ep", "q_row_idx", "eta_row_idx_minus1",
          "coef_stride3", "w_pitch16", "w_row_jm1", "gtab_ignored", "cond_takes_uncond", "blend_at_idx0", "pred_x0_blended",
          "ring_blended", "t_off_by_one", "t_unclamped", "tmpl_blend", "tmpl_rng", "tmpl_scale", "tmpl_hist")


def G(flat, idx):
  """flat[idx], NaN where idx is outside the array or there is no array."""
  idx = torch.as_tensor(idx, dtype=I64)
  out = torch.full(idx.shape, NAN, dtype=F64)
  if flat is None:
    return out
  ok = (idx >= 0) & (idx < flat.numel())
  out[ok] = flat[idx[ok]]
  return out


def _sqrt(v):
  return float(torch.sqrt(torch.tensor(float(v), dtype=F64)))       # (NaN below 0, as sqrtf)


def g1(flat, k):
  return float(G(flat, torch.tensor([k]))[0])


def decomposition(total, W, fault=None):
  """Element i belongs to work item i // W; item t is taken by pass t // (grid * 256)."""
  items = total // W
  grid = max(1, min(CAP, -(-items // BLOCK)))
  S = grid * BLOCK
  i = torch.arange(total, dtype=I64)
  item = i // W
  written = torch.ones(total, dtype=torch.bool)
  if fault == "drop_last":
    written &= item != items - 1
  if fault == "skip_second_pass":
    written &= item // S != 1
  # `i += stride - one item`: the first item of a pass is also the last of the one before
  twice = (item % S == S - 1) & (item + 1 < items) if fault == "overlap_second_pass" else torch.zeros(total, dtype=torch.bool)
  return NS(i=i, item=item, base=item * W, written=written, twice=twice, block_first=(item - item % BLOCK) * W)


def model_draw(c, stream, b, q, k):
  """The CPU stand-in of word k of counter (q, FIRST + b, stream, 0)."""
  w = R.philox4x32_10((q.numpy().astype(np.uint64), (FIRST + b.numpy()).astype(np.uint64) & np.uint64(R.MASK),
                       int(stream) & R.MASK, 0), R.key_of(SEED))
  w = np.stack([np.broadcast_to(x, q.shape) for x in w], axis=-1)
  sel = np.take_along_axis(w, k.numpy()[:, None].astype(np.int64), axis=1)[:, 0]
  return torch.from_numpy((sel.astype(np.uint64) >> np.uint64(12)).astype(np.float64))


def _bq(c, d, fault):
  """(sample, quad of it) the four-wide bodies key the draws of element i by."""
  first = d.block_first if fault == "b_per_block" else d.base
  b = first // c.n
  return b, (d.base - b * c.n) >> 2


def _update_values(c, p, d, xt, fault):
  body, H, S, Rng, Blend = form(c)
  if fault == "tmpl_blend":
    Blend = not Blend
  if fault == "tmpl_rng":
    Rng = not Rng
  if fault == "tmpl_scale":
    S = {"arg": "cond", "table": "arg", "cond": "table"}[S]
  if fault == "tmpl_hist":
    H = {"ab": "table", "table": "ab"}[H]
  weights = p.weights if H == "table" else None
  total, i, idx = c.B * c.n, d.i, p.idx
  cs = 3 if fault == "coef_stride3" else 4
  c1, c2, a_prev = g1(p.coef, idx * cs), g1(p.coef, idx * cs + 1), g1(p.coef, idx * cs + 2)
  sigma = g1(p.coef, idx * cs + 3) if H == "ddim" else 0.0
  hist = H == "ab" or (H == "table" and weights is not None)
  j = max(0, min(3, p.start - idx)) if hist else 0
  w = [1.0, 0.0, 0.0, 0.0]
  if H == "table" and weights is not None:
    pitch = 16 if fault == "w_pitch16" else c.pitch
    o = idx * pitch + 4 * (j - 1 if fault == "w_row_jm1" else j)
    w = [g1(weights, o + m) if m <= j else 0.0 for m in range(4)]
  gs = p.gs
  if S == "table" and fault != "gtab_ignored":
    gs = g1(p.gtab, idx)
  if S == "table" and fault == "gtab_ignored":
    gs = 1.0                                                # what ldm_cfg_sched_update puts into a.gs
  ec = G(p.eps, total + i)
  if S == "cond":
    e0 = G(p.eps, i) if fault == "cond_takes_uncond" else ec
  else:
    eu = G(p.eps, i)
    e0 = eu + gs * (ec - eu)
  h = [None] + [G(p.ring, ((idx + m + (1 if fault == "ring_slot_plus1" else 0)) & 3) * total + i) if hist and m <= j else None
                for m in (1, 2, 3)]
  if H == "ab":
    ep = (e0, None, None, None)[j] if j == 0 else \
        (3 * e0 - h[1]) / 2 if j == 1 else \
        (23 * e0 - 16 * h[1] + 5 * h[2]) / 12 if j == 2 else (55 * e0 - 59 * h[1] + 37 * h[2] - 9 * h[3]) / 24
  elif H == "table":
    ep = w[0] * e0
    for m in range(1, j + 1):
      ep = w[m] * h[m] + ep
  else:
    ep = e0
  sa = _sqrt(a_prev)
  sb = _sqrt(1 - a_prev - sigma * sigma) if H == "ddim" else _sqrt(1 - a_prev)
  if H == "invert":
    x0 = (xt - sb * ep) / sa
    o = (x0 + c2 * ep) / c1
  else:
    x0 = c1 * xt - c2 * ep
    if H == "ddim" and c.clip:
      x0 = torch.where(torch.isnan(x0), x0, x0.clamp(-1, 1))
    o = sa * x0 + sb * ep
  if H == "ddim":
    row = idx - 1 if fault == "eta_row_idx_minus1" else idx
    if body == "scalar":
      if p.noise is not None:
        o = o + G(p.noise, row * c.noise_stride + i) * sigma
    elif sigma != 0:
      b, q = _bq(c, d, fault)
      o = o + model_draw(c, R.ETA_STREAM + row, b, q, i - d.base) * sigma
  on = Blend and p.z0 is not None and (idx >= 1 or fault == "blend_at_idx0")
  e_store, x0_store = (ep if fault == "ring_stores_ep" else e0), x0
  if on:
    qa, qb = g1(p.qcoef, (idx - 1) * 2), g1(p.qcoef, (idx - 1) * 2 + 1)
    row = idx if fault == "q_row_idx" else idx - 1
    if Rng:
      b, q = _bq(c, d, fault)
      qe = model_draw(c, R.Q_STREAM + row, b, q, i - d.base)
    else:
      qe = G(p.q, row * c.q_stride + i)
    mi = d.base if fault == "mask_quad_base" else i
    if fault == "mask_no_sample":
      mi = mi % c.n
    m = G(p.mask, mi // c.ch)
    qs = qa * G(p.z0, i) + qb * qe
    o = m * qs + (1 - m) * o
    if fault == "pred_x0_blended":
      x0_store = m * qs + (1 - m) * x0
    if fault == "ring_blended":
      e_store = m * qs + (1 - m) * e0
  return NS(o=o, x0=x0_store, e=e_store, hist=hist, xu=x0 if fault == "xunet_from_x0" else o)


def _x_unet(c, d, v, fault):
  total = c.B * c.n
  xu = torch.full((2 * total,), NAN, dtype=F64)
  w = d.written
  xu[d.i[w]] = v[w]
  xu[(c.n if fault == "xunet_half_at_n" else total) + d.i[w]] = v[w]
  return xu.to(F32).to(c.xd).to(F64)


def model(c, p, fault=None):
  """The outputs of one launch as the kernel's decomposition produces them (NS like `reference`); NaN where nothing is
  stored (the value before the launch where the output is the input)."""
  total = c.B * c.n
  if c.entry in FILL_ENTRIES:
    return _model_fill(c, p, fault, total)
  d = decomposition(total, width(c), fault)
  v = _update_values(c, p, d, p.xt, fault)
  if bool(d.twice.any()) and c.alias:                     # an element computed twice in place: f(f(x))
    v2 = _update_values(c, p, d, torch.where(d.twice, v.o, p.xt), fault)
    for name in ("o", "x0", "e", "xu"):
      setattr(v, name, torch.where(d.twice, getattr(v2, name), getattr(v, name)))
  keep = p.xt if c.alias else torch.full((total,), NAN, dtype=F64)
  out = NS(xt_out=torch.where(d.written, v.o, keep), index=p.idx - (1 if c.dec else 0))
  out.pred_x0 = torch.where(d.written, v.x0, torch.tensor(NAN, dtype=F64)) if c.pred else None
  out.ring = None
  if p.ring is not None:
    out.ring = p.ring.clone()
    if v.hist:
      s = (p.idx & 3) * total
      out.ring[s:s + total] = torch.where(d.written, v.e, p.ring[s:s + total])
  out.x_unet = None if c.xd is None else _x_unet(c, d, v.xu, fault)
  return out


def _model_fill(c, p, fault, total):
  d = decomposition(total, width(c), fault)
  i = d.i
  if c.entry == "q_sample":
    b = i // c.n
  else:
    b, q = _bq(c, d, fault)
  if c.entry in ("normal_fill", "philox_u32"):
    o = model_draw(c, p.stream, b, q, i - d.base)
  else:
    tb = (b - 1).clamp(min=0) if fault == "t_off_by_one" else b
    t = p.t[tb]
    if fault != "t_unclamped":
      t = t.clamp(0, Q_STEPS - 1)
    sa, sb = G(p.sac, t), G(p.s1m, t)
    if c.entry == "q_sample":
      row = (p.idx - 1 if fault == "eta_row_idx_minus1" else p.idx) if c.use_index else 0
      nz = G(p.noise, row * c.noise_stride + i)
    else:
      nz = model_draw(c, p.stream, b, q, i - d.base)
    o = sa * G(p.x0, i) + sb * nz
  out = NS(xt_out=torch.where(d.written, o, torch.tensor(NAN, dtype=F64)), pred_x0=None, ring=None, index=None, x_unet=None)
  if c.xd is not None:
    out.x_unet = _x_unet(c, d, o, fault)
  return out


# ============================================================================================================
# which cases a fault can show in
# ============================================================================================================
def _o_is_x0(c):
  """The launch's xt' equals its x0 element for element (so x_unet_out taken from x0 would not show)."""
  if blend_on(c):
    return False
  if c.entry == "invert":
    return c.probe == "xt"
  if c.probe in ("xt", "eps"):
    return True
  return c.probe == "census" and c.a_prev == 1


def _eps_shows(c):
  """A change of e_0 reaches an output: the ring stores it, or the table row gives e' a weight (under clip_denoised
  x0 is -1, 0 or 1 whatever e' is)."""
  if has_hist(c):
    return True
  if c.probe == "census_sigma":
    return c.pred and not c.clip
  return c.probe in ("eps", "census") and not c.clip


def mutation_applies(c, f):
  """Whether fault `f` changes what the kernel of case `c` computes.  The exemptions, by name:"""
  upd = c.entry in UPDATE_ENTRIES
  npass = passes(c)[0]
  wide = width(c) == WIDE
  if f == "drop_last":
    return True
  if f == "skip_second_pass":
    return npass >= 2
  if f == "overlap_second_pass":                 # shows only where an element is computed twice IN PLACE and f(f(x)) != f(x)
    return npass >= 2 and upd and c.alias and c.probe.startswith("census")
  if f == "xunet_half_at_n":
    return c.xd is not None and c.B > 1
  if f == "t_off_by_one":
    return c.entry in ("q_sample", "q_sample_rng") and c.B > 1
  if f == "t_unclamped":
    return c.entry in ("q_sample", "q_sample_rng")
  if f == "b_per_block":                         # a sample boundary inside a workgroup's 1024 elements, and draws that count
    drawn = c.probe in ("draw_eta", "draw_q") if upd else (c.entry != "q_sample" and c.probe == "noise")
    return wide and drawn and c.B > 1 and c.n % (BLOCK * WIDE) != 0
  if f == "eta_row_idx_minus1":
    if c.entry == "q_sample":
      return c.use_index and c.noise_stride != 0 and c.probe == "noise"
    if c.entry == "ddim_rng":
      return c.probe == "draw_eta"
    return c.entry in ("ddim", "ddim_masked") and c.probe in ("noise", "census_sigma") and c.noise_stride != 0
  if not upd:
    return False
  body, H, S, Rng, Blend = form(c)
  j = order(c)
  if f == "xunet_from_x0":
    return c.xd is not None and not _o_is_x0(c)
  if f == "mask_quad_base":                      # a quad straddles two pixels
    return blend_on(c) and wide and c.ch % 4 != 0
  if f == "mask_no_sample":
    return blend_on(c) and c.B > 1
  if f == "ring_slot_plus1":
    return has_hist(c) and j >= 1
  if f == "ring_stores_ep":                      # e' == e_0 at j = 0 and under a one-hot row at m = 0
    return has_hist(c) and j >= 1 and not (has_weights(c) and not c.probe.startswith("census") and c.hot == 0)
  if f == "q_row_idx":                           # Q counts (q_coef[1] != 0) and its rows are apart
    return blend_on(c) and c.qc[1] != 0 and (Rng or c.q_stride != 0)
  if f == "coef_stride3":
    return c.idx >= 1
  if f == "w_pitch16":
    return has_weights(c) and c.pitch != 16 and c.idx >= 1
  if f == "w_row_jm1":
    return has_weights(c)
  if f == "gtab_ignored":
    return S == "table" and c.gs != 1 and _eps_shows(c)
  if f == "cond_takes_uncond":
    return S == "cond"
  if f == "blend_at_idx0":
    return c.blend and c.idx == 0
  if f == "pred_x0_blended":
    return blend_on(c) and c.pred
  if f == "ring_blended":
    return blend_on(c) and has_hist(c)
  if f == "tmpl_blend":                          # Blend = false -> true only adds a run-time test of z0
    return blend_on(c)
  if f == "tmpl_rng":                            # kDdim is instantiated with Rng only, kInvert without
    return blend_on(c) and wide and H in ("ab", "table") and (Rng or c.qc[1] != 0)      # (a table Q counts only then)
  if f == "tmpl_scale":                          # the scalar body has no Scale; at gs = 1 the three forms are one sum
    return wide and (S == "cond" or (c.gs != 1 and _eps_shows(c)))
  if f == "tmpl_hist":                           # Adams-Bashforth <-> table; at j = 0 both are e' = e_0 (w[0] = 1)
    return H == "ab" or (H == "table" and has_weights(c) and j >= 1)
  raise KeyError(f)


# the entries a fault can occur in (every one must have a case that catches it)
def fault_entries(f):
  blendable = ("ddim_masked", "ddim_rng", "plms", "plms_rng", "ms", "ms_rng", "sched")
  wide_blend = blendable[1:]
  histe = ("plms", "plms_rng", "ms", "ms_rng", "sched")
  return {
      "drop_last": UPDATE_ENTRIES + FILL_ENTRIES,
      "skip_second_pass": ("ddim_masked", "ms", "ddim_rng") + FILL_ENTRIES,       # per BODY: one entry of each
      "overlap_second_pass": ("ddim_masked", "ms"),
      "xunet_half_at_n": UPDATE_ENTRIES + ("q_sample", "q_sample_rng", "normal_fill"),
      "xunet_from_x0": UPDATE_ENTRIES,
      "mask_quad_base": wide_blend, "mask_no_sample": blendable,
      "b_per_block": ("ddim_rng", "plms_rng", "ms_rng", "sched", "q_sample_rng", "normal_fill", "philox_u32"),
      "ring_slot_plus1": histe, "ring_stores_ep": histe, "ring_blended": histe,
      "q_row_idx": blendable, "eta_row_idx_minus1": ("ddim", "ddim_masked", "ddim_rng", "q_sample"),
      "coef_stride3": UPDATE_ENTRIES, "w_pitch16": ("ms", "ms_rng", "sched"), "w_row_jm1": ("ms", "ms_rng", "sched"),
      "gtab_ignored": ("sched",), "cond_takes_uncond": ("sched", "invert"), "blend_at_idx0": blendable,
      "pred_x0_blended": blendable, "t_off_by_one": ("q_sample", "q_sample_rng"), "t_unclamped": ("q_sample", "q_sample_rng"),
      "tmpl_blend": blendable, "tmpl_rng": ("plms", "plms_rng", "ms", "ms_rng", "sched"), "tmpl_scale": UPDATE_ENTRIES[2:],
      "tmpl_hist": histe,
  }[f]


# ============================================================================================================
# comparing
# ============================================================================================================
OUTPUTS = ("xt_out", "pred_x0", "ring", "x_unet", "index")


def same(a, b):
  """Equal, NaN where NaN (None where None)."""
  if a is None or b is None:
    return a is None and b is None
  if not torch.is_tensor(a):
    return a == b
  a, b = a.to(F64), b.to(F64)
  return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def differing(got, want):
  """The names of the outputs in which two results differ."""
  return [k for k in OUTPUTS if not same(getattr(got, k), getattr(want, k))]
