"""The row-panel probes judged on the CPU (no GPU needed): the reference against the oracle, the probes' own exactness
conditions, the measured constants, and the mutation check -- every reference of a subtly wrong kernel in
ffn_probes.MUTATIONS must fail the gate of some probe in every case it applies to."""
import math
import os
import re

import pytest
import torch

import ffn_probes as Fp
import norm_check
from oracle import ldm_oracle as O

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LAUNCHES = {}


def launches(c, probe):
  """(tag, P, gate, ref, info) of a probe in a case, computed once; big cases on four panels (first, the two at the
  pair boundary, last)."""
  key = (c, probe)
  if key not in _LAUNCHES:
    rows = panel_rows(c)
    _LAUNCHES[key] = [(tag, P, gate) + Fp.ref64(P, rnd=gate != "gelu", rows=rows) for tag, P, gate in Fp.PROBES[probe](c)]
  return _LAUNCHES[key]


def panel_rows(c):
  if c.M <= 1024:
    return None
  np_ = c.M // 128
  return torch.cat([torch.arange(128 * p, 128 * p + 128) for p in (0, np_ // 2 - 1, np_ // 2, np_ - 1)])


ALL = Fp.cases() + Fp.big_cases()


def test_switch_over_constant_matches_the_dispatch():
  src = open(os.path.join(ROOT, "ldm_tf2_amd", "csrc", "ffn.hip")).read()
  found = re.findall(r"if \(\(M \+ 127\) / 128 >= (\d+)\)", src)
  assert found == [str(Fp.SWITCH_PANELS)], found
  assert all(c.M // 128 >= Fp.SWITCH_PANELS for c in Fp.big_cases())
  assert all((c.M + 127) // 128 < Fp.SWITCH_PANELS for c in Fp.cases())


def test_open_gate_is_exact_in_float32_and_the_gelu_allowance_covers_the_formula():
  g = torch.tensor([Fp.GELU_G])
  assert float(Fp.gelu_f32(g)) == Fp.GELU_G and float(Fp.gelu_f32(torch.tensor([0.0]))) == 0.0
  assert float(Fp.gelu_f32(torch.tensor([-0.0]))) == 0.0
  grid = Fp.gelu_grid()
  nz = grid != 0
  a = float(((Fp.gelu_as64(grid) - Fp.gelu64(grid)).abs()[nz] / grid.abs()[nz]).max())
  print(f"GELU_A model: {a:.3e} (recorded {Fp.GELU_A_MODEL:.3e})")
  assert a <= Fp.GELU_A_MODEL and a >= 0.5 * Fp.GELU_A_MODEL
  # the float32 transcription itself meets probe 6's gate
  got, ref = Fp.gelu_f32(grid).to(torch.bfloat16).to(F64), Fp.gelu64(grid)
  assert torch.isfinite(got).all()
  assert bool(((got - ref).abs() <= Fp.true_ulp(ref) + Fp.GELU_A * grid.abs()).all())
  far = grid >= 15.0
  assert far.sum() >= 4 and torch.equal(got[far], Fp.rb(grid)[far])
  assert (grid.abs() > 14.4).sum() >= 8 and (grid == 0).sum() == 2 and ((grid > -6) & (grid < 0)).sum() >= 700


@pytest.mark.parametrize("c", ALL, ids=Fp.case_id)
def test_probes_keep_their_own_exactness_conditions(c):
  for probe in Fp.probes_of(c):
    for tag, P, gate, ref, info in launches(c, probe):
      assert torch.isfinite(ref).all(), (probe, tag)
      if gate in ("exact", "ulp") and probe != "p5":        # (probe 5 crosses a softmax: its att2 is no integer)
        assert info.exact, f"{probe} {tag}: a rounding point changes a value"
        assert info.maxint <= 256.0 and float(ref.abs().max()) <= 256.0, (probe, tag, info.maxint)
        assert torch.equal(ref, ref.round()), (probe, tag)
      for n in ("x", "r0", "r1", "wo1", "wq", "k", "v", "wo", "w1", "w2", "wp"):
        t = getattr(P, n)
        assert torch.equal(Fp.rb(t), t), f"{probe} {tag}: {n} is not representable in bf16"
      for n in ("bo1", "qb", "bo", "b1", "b2", "bp"):
        t = getattr(P, n)
        assert torch.equal(t.to(torch.float32).to(F64), t)


def test_ulp_from_the_exponent_bits_is_norm_check_bf16_ulp():
  v = torch.cat([torch.randn(4096, dtype=F64) * 50, torch.tensor([0.0, 2.0 ** -6, 2.0 ** -7, 1.0, 255.0, 256.0, -3.0], dtype=F64),
                 2.0 ** torch.arange(-20, 12, dtype=F64), torch.rand(512, dtype=F64) * 2.0 ** -5])
  assert torch.equal(Fp.bf16_ulp(v), norm_check.bf16_ulp(v))
  assert float(Fp.true_ulp(torch.tensor([1.5e-5], dtype=F64))) == 2.0 ** -24


def test_probe4_rows_have_equal_statistics():
  for mean in (False, True):
    h = Fp.p4_rows(256, mean)
    mu = h.mean(1)
    var = ((h - mu.view(-1, 1)) ** 2).mean(1)
    assert torch.equal(var, torch.full_like(var, 3.5)) and 3.5 + Fp.P4_EPS == 16.0
    assert torch.equal(mu, torch.zeros_like(mu)) if not mean else bool((mu[:16] != mu[16:32]).all())
    assert not any(torch.equal(h[r], h[r ^ 16]) for r in range(256))
  w = Fp.p4_w1()
  cs = w.sum(1)
  assert torch.equal(cs, Fp.p4_cs()) and bool((cs != 0).all())
  for c0 in range(0, Fp.HID, 64):                   # distinct inside a 64-unit chunk, and against the chunk before
    assert cs[c0:c0 + 64].unique().numel() == 64
    assert c0 == 0 or bool((cs[c0:c0 + 64] != cs[c0 - 64:c0]).all())
  assert float(w.abs().sum(1).max()) <= 32.0 and bool(((w != 0).sum(1) == 10).all())
  for b in range(Fp.HID // 32):                     # every K column alive (exactly once) in every 32 hidden units
    assert torch.equal((w[32 * b:32 * b + 32] != 0).sum(0), torch.ones(Fp.C, dtype=torch.int64))


def test_probe5_probabilities_are_exact_powers_of_two():
  for c in Fp.cases():
    if c.entry == "block":
      (_, P, _, ref, info), = launches(c, "p5")
      assert info.pow2 is True and torch.isfinite(ref).all()
      q_cols = (P.wq != 0).sum(0)
      assert torch.equal(q_cols, torch.ones(Fp.C, dtype=torch.int64))       # every K column feeds one live q column
      assert float(P.wq.view(Fp.H, Fp.SP, Fp.C)[:, Fp.S:].abs().max()) == 0.0


def test_census_regions_are_alive():
  """probes 1 - 3, census form: every K column has a non-zero weight in every 64-column wave-tile region (and the A side
  is never zero), so a single lost product is visible."""
  for c in Fp.cases():
    for probe in ("p1", "p2", "p3"):
      if probe not in Fp.probes_of(c):
        continue
      for tag, P, _ in Fp.PROBES[probe](c):
        if not tag.startswith("census"):
          continue
        name = {"p1": "wo1" if c.entry == "block" and tag == "census" else "wo", "p2": "wp", "p3": "w2"}[probe]
        w = getattr(P, name)
        for n0 in range(0, Fp.C, 64):
          assert bool(((w[n0:n0 + 64] != 0).sum(0) > 0).all()), (Fp.case_id(c), probe, tag, n0)
        if probe == "p1" and tag == "census" and c.entry in ("tail", "block"):
          assert bool((P.x != 0).all())
        if probe == "p1" and (c.entry == "xtail" or tag == "census2"):
          assert bool((P.v != 0).all())
  dead = torch.ones(Fp.C, Fp.K0, dtype=F64)
  dead[64:128, 5] = 0.0
  assert float(Fp._revive(dead)[64:128, 5].abs().sum()) == 1.0


def _gauss_case(entry):
  c = {"ffn": Fp.Case("ffn", 200, 0, 0, 0, 0, 200), "tail": Fp.Case("tail", 200, 0, 0, 0, 0, 200),
       "xtail": Fp.Case("xtail", 256, 2, 128, 77, 80, 256), "block": Fp.Case("block", 256, 2, 128, 77, 80, 256)}[entry]
  g = torch.Generator().manual_seed(5)
  rn = lambda *sh, sc=1.0: torch.randn(*sh, generator=g, dtype=F64) * sc
  P = Fp.neutral(c)
  P.x = rn(*P.x.shape)
  P.r0, P.r1 = rn(c.M, Fp.C), rn(c.M, Fp.C)
  P.wo1, P.wo, P.wp = rn(Fp.C, Fp.K0, sc=Fp.K0 ** -0.5), rn(Fp.C, Fp.K0, sc=Fp.K0 ** -0.5), rn(Fp.C, Fp.C, sc=Fp.C ** -0.5)
  P.wq, P.qb = rn(Fp.K0, Fp.C, sc=Fp.C ** -0.5), rn(Fp.K0)
  P.k, P.v = rn(*P.k.shape), rn(*P.v.shape)
  P.w1, P.b1, P.w2 = rn(2 * Fp.HID, Fp.C, sc=Fp.C ** -0.5), rn(2 * Fp.HID), rn(Fp.C, Fp.HID, sc=Fp.HID ** -0.5)
  P.bo1, P.bo, P.b2, P.bp = rn(Fp.C), rn(Fp.C), rn(Fp.C), rn(Fp.C)
  return c, P


@pytest.mark.parametrize("entry", ("ffn", "tail", "xtail", "block"))
def test_reference_agrees_with_the_oracle(entry):
  """The probe reference (unrounded) against oracle.ldm_oracle's dense / layer_norm / gelu in float64 on Gaussian data."""
  c, P = _gauss_case(entry)
  got, _ = Fp.ref64(P, rnd=False)
  one, zero = torch.ones(Fp.C, dtype=F64), torch.zeros(Fp.C, dtype=F64)

  def attend(q):
    qh = q.view(c.R, c.T, Fp.H, Fp.SP)[..., :Fp.S]
    p = torch.softmax(torch.einsum("nqhs,nchs->nhqc", qh, P.k) * math.log(2.0), dim=3)
    o = torch.zeros(c.R, c.T, Fp.H, Fp.SP, dtype=F64)
    o[..., :Fp.S] = torch.einsum("nhqc,nchs->nqhs", p, P.v)
    return o.view(c.M, Fp.K0)

  a = P.x
  if entry == "block":
    h1 = P.r0 + O.dense(a, P.wo1.t(), P.bo1)
    a, res = attend(O.dense(O.layer_norm(h1, one, zero, eps=P.eps), P.wq.t(), P.qb)), h1
  elif entry == "xtail":
    a, res = attend(a), P.r0
  elif entry == "tail":
    res = P.r0
  h = a if entry == "ffn" else res + O.dense(a, P.wo.t(), P.bo)
  f = O.dense(O.layer_norm(h, one, zero, eps=P.eps), P.w1.t(), P.b1)
  y = h + O.dense(f[:, :Fp.HID] * O.gelu(f[:, Fp.HID:]), P.w2.t(), P.b2)
  ref = y if entry == "ffn" else P.r1 + O.dense(y, P.wp.t(), P.bp)
  assert float((got - ref).abs().max()) <= 1e-11 * float(ref.abs().max())


def test_probe7_constants_cover_the_rounded_model():
  for entry in ("ffn", "tail", "xtail", "block"):
    worst = 0.0
    for c in ALL:
      if c.entry != entry:
        continue
      (_, P, _, ref_r, _), = launches(c, "p7")
      ref, info = Fp.ref64(P, rnd=False, rows=panel_rows(c))
      worst = max(worst, Fp.c_needed(ref_r, ref, info.absref))
    print(f"probe 7 c needed, {entry}: {worst:.3f} (recorded {Fp.MODEL_C[entry]})")
    assert worst <= Fp.MODEL_C[entry] and worst >= 0.5 * Fp.MODEL_C[entry]


_ORDER = {"wo1": "p1", "wo": "p1", "wp": "p2", "w2": "p3", "w1": "p4", "wq": "p5", "qb": "p5", "bo": "p7"}
_KIND_ORDER = {"gelu_tanh": "p6", "gelu_relu4": "p6", "stats_xor16": "p4", "ctx_next_sample": "p7", "swap_bias": "p2",
               "swap_res": "p2", "aux_prev_chunk": "p3", "cs_bias_swapped": "p3", "val_gate_swapped": "p3",
               "hidden_cell_shift": "p3"}


def _detected(c, mut):
  if mut[0] in ("store_row_M", "store_pad"):
    (_, _, _, ref, _) = launches(c, "p3")[0]
    M = ref.shape[0]
    for pad in (0, Fp.PAD["out"]):
      before = torch.full((M + Fp.GUARD_ROWS, Fp.C + pad), Fp.SENTINEL, dtype=torch.bfloat16)
      assert Fp.untouched(before, Fp.store(before, ref.to(torch.bfloat16), M), M)
      if not Fp.untouched(before, Fp.store(before, ref.to(torch.bfloat16), M, mut), M):
        return True
    return False
  first = _KIND_ORDER.get(mut[0]) or _ORDER.get(mut[1] if len(mut) > 1 else None)
  order = [p for p in ((first,) if first else ()) + Fp.probes_of(c) if p in Fp.probes_of(c)]
  if mut[0] in ("gelu_tanh", "gelu_relu4"):        # probe 6 itself must catch these
    order = ["p6"]
  for probe in dict.fromkeys(order):
    for tag, P, gate, ref, info in launches(c, probe):
      for view in (("contig", "padded") if mut[0] == "stride_ignored" else ("contig",)):
        bad, _ = Fp.ref64(P, mut=mut, rnd=gate != "gelu", view=view, rows=panel_rows(c))
        if not Fp.judge(gate, bad, ref, info, P, c)[1]:
          return True
  return False


@pytest.mark.parametrize("c", ALL, ids=Fp.case_id)
def test_every_mutation_fails_some_probe(c):
  for tag_probe in Fp.probes_of(c):                # the unmutated reference passes its own gate
    for tag, P, gate, ref, info in launches(c, tag_probe):
      got = Fp.rb(ref) if gate == "gelu" else ref
      assert Fp.judge(gate, got, ref, info, P, c)[1]
  missed = []
  for mut in Fp.MUTATIONS:
    ok, reason = Fp.mutation_applies(mut, c)
    assert ok or reason
    if ok and not _detected(c, mut):
      missed.append(mut)
  assert not missed, f"{Fp.case_id(c)}: undetected mutations {missed}"
