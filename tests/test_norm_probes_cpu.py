"""The norm probes of tests/norm_probes.py checked without a GPU: the float64 reference against the oracle, a float32
emulation of every kernel's arithmetic on every case (exact at the non-deviants, inside the gates at the deviants), every
mutation failing the gates on every case it applies to, the sweep's coverage and its cap of 24 launches, the plan
mirror against the library's host query, and the enumeration that proves the plans (256, 24) and (512, 24) dead."""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_probes as P
from oracle import ldm_oracle as O

BF, F32, F64 = P.BF, P.F32, P.F64
NAN = float("nan")
CASES = P.all_cases()
NORM_CASES = [c for c in CASES if c.kind != "ln_fold"]
FOLD_CASES = [c for c in CASES if c.kind == "ln_fold"]


def _lib():
  from ldm_tf2_amd._lib import BF16, F32 as F32C, lib
  return lib, {BF: BF16, F32: F32C}


def test_case_ids_are_unique():
  ids = [P.case_id(c) for c in CASES]
  assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("kind", ["gn", "ln"])
def test_reference_matches_the_oracle(kind):
  c = P._fused(F32, 320, 3, 35, (2, 5, 256, 8)) if kind == "gn" else P.Case("ln", F32, 33, 1, 328, 1, 4, 0, False, False, (8,))
  gamma, beta = P.params(c)
  g = torch.Generator().manual_seed(5)
  for x in (P.census(c, 0), P.census(c, 0) + torch.randn(c.B * c.HW, c.C, generator=g, dtype=F64)):
    ref = P.reference(c, x, gamma, beta)
    if kind == "gn":
      want = O.group_norm(x.view(c.B, c.HW, 1, c.C), gamma.double(), beta.double(), groups=c.G, eps=P.EPS)
    else:
      want = O.layer_norm(x, gamma.double(), beta.double(), eps=P.EPS)
    assert torch.allclose(ref, want.reshape(ref.shape), rtol=1e-12, atol=1e-12)


def test_census_values():
  """|M_u| in 4 .. 7, neighbours differ, deviants come in +-d pairs inside their own unit, integers exact in bf16."""
  for c in CASES:
    m = P.unit_values(c)
    assert m.abs().min() >= 4 and m.abs().max() <= 7
    assert (m[:, 1:] != m[:, :-1]).all() and (m[1:] != m[:-1]).all()
    assert 1 <= c.p <= 4
    for launch in {0, P.sweep_launches(c) - 1}:
      r, ch, delta, unit = P.deviants(c, launch)
      assert len(torch.unique(r * c.C + ch)) == len(r), "two deviants share a position"
      assert torch.equal(unit, (r // c.HW) * c.G + ch // P.cpg(c))
      assert delta.view(-1, 2).sum(dim=1).abs().max() == 0 and set(delta.abs().tolist()) <= {1.0, 2.0}
      if c.kind == "pair":
        pilot = ((r % c.HW) == 0) & (ch % P.cpg(c) == 0)
        assert int(pilot.sum()) == (c.B * c.G if c.pilot else 0)
    x = P.census(c, 0)
    assert x.abs().max() < 256 and torch.equal(x.to(BF).to(F64), x)
    assert c.HW * P.cpg(c) * 9 < 2 ** 24


@pytest.mark.parametrize("c", CASES, ids=P.case_id)
def test_sweep_covers_every_position_within_the_cap(c):
  L = P.sweep_launches(c)
  assert 1 <= L <= P.MAX_LAUNCHES
  if c.pilot:
    return
  gb, _ = P.sweep_class(c)
  seg = gb * P.cpg(c)
  seen = torch.zeros(c.HW * seg, dtype=torch.bool)
  for launch in range(L):
    seen[P.slab_positions(c, launch)] = True
    if launch == L - 2:
      before = bool(seen.all())
  if c.kind in ("ln_out", "ln_fold") and c.B == 1:
    assert int(seen.sum()) == 2 * c.p * P.MAX_LAUNCHES        # one row: the first 192 columns (module docstring)
    return
  if c.kind == "pair":
    assert gb == 1 and not seen[0] and seen[1:].all()         # every position but the pilot
  else:
    assert seen.all(), f"{int((~seen).sum())} slab positions are never a deviant"
  if L > 1:
    assert not before, "one launch fewer would do"


def _left(c, x):
  e = P.epc(c.dt)
  return torch.cat([torch.full((x.shape[0], e), NAN, dtype=F64), x[:, :c.C - e]], dim=1)


@pytest.mark.parametrize("c", NORM_CASES, ids=P.case_id)
def test_emulation_passes_and_mutations_fail(c):
  gamma, beta = P.params(c)
  L = P.sweep_launches(c)
  small = c.B * c.HW * c.C <= 1 << 20
  for launch in sorted({0, L - 1} if small else {0}):
    x = P.census(c, launch)
    ref = P.reference(c, x, gamma, beta)
    msg, worst = P.gates(c, P.rounded(ref, c.dt), ref, beta, launch, "reference")
    assert msg is None and worst <= 0.5 + 1e-9, msg
    emu = P.EMULATE[c.kind](c, x.to(F32), gamma, beta)
    msg, worst = P.gates(c, emu, ref, beta, launch, "emulation " + P.case_id(c))
    print(f"EMU {P.case_id(c)} launch {launch}: worst deviant {worst:.3f} x gate")
    assert msg is None, msg
    for name in P.MUTATIONS:
      if not P.mutation_applies(c, name):
        continue
      bad = P.reference(c, x, gamma, beta, mut=name, launch=launch, left=_left(c, x) if name == "slice_left" else None)
      msg, _ = P.gates(c, P.rounded(bad, c.dt), ref, beta, launch)
      assert msg is not None, f"mutation {name} passes the gates of {P.case_id(c)} at launch {launch}"


def test_every_mutation_applies_somewhere():
  for name in P.MUTATIONS:
    kinds = {c.kind for c in NORM_CASES if P.mutation_applies(c, name)}
    assert kinds, name
  assert {c.kind for c in NORM_CASES if P.mutation_applies(c, "chunk_tail")} == {"pair"}
  assert {c.kind for c in NORM_CASES if P.mutation_applies(c, "last_vector")} == {"ln"}
  assert {c.kind for c in NORM_CASES if P.mutation_applies(c, "straddle_low")} == {"fused"}


@pytest.mark.parametrize("c", FOLD_CASES, ids=P.case_id)
def test_fold_emulation(c):
  """E[x^2] - mean^2 at |M| <= 7, K = 320 stays inside the 1-ulp gate; a lost deviant does not."""
  N, sel, bias = P.fold_operands(c)
  for launch in range(P.sweep_launches(c)):
    x = P.census(c, launch)
    ref = P.fold_reference(c, x, sel, bias)
    msg, worst = P.fold_gates(c, P.emulate_ln_fold(c, x.to(F32), sel, bias), ref)
    print(f"EMU {P.case_id(c)} launch {launch}: worst {worst:.3f} bf16 ulp")
    assert msg is None, msg
    r, ch, delta, _ = P.deviants(c, launch)
    lost = x.clone()
    lost[r[0], ch[0]] -= delta[0]                       # row r[0] without its first deviant
    bad = P.fold_reference(c, lost, sel, bias)
    bad[:, sel == ch[0]] = ref[:, sel == ch[0]]         # (only the statistics lose it)
    msg, _ = P.fold_gates(c, bad.to(BF), ref)
    assert msg is not None


def test_plan_mirror_matches_the_library():
  lib, code = _lib()
  f = (C.c_int32 * 4)()
  n = 0
  for dt in (BF, F32):
    for Cc, G in [(32, 1), (64, 1), (64, 4), (128, 32), (288, 32), (320, 32), (512, 32), (640, 32), (640, 64), (960, 32),
                  (1280, 32), (1920, 32), (2560, 32), (2560, 16), (100, 32), (330, 32), (4096, 32)]:
      for B in (1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 64, 65):
        for HW in list(range(1, 130)) + [143, 192, 193, 200, 256, 272, 273, 400, 401, 408, 409, 544, 545, 552, 816, 817,
                                         897, 904, 905, 1024, 1088, 1089, 1632, 1633, 2048, 4096, 16384]:
          st = lib.ldm_groupnorm_fused_form(B, HW, Cc, G, code[dt], f)
          want = P.fused_plan(B, HW, Cc, G, dt)
          assert (tuple(f) if st == 0 else None) == want, (dt, Cc, G, B, HW, st, tuple(f), want)
          assert lib.ldm_groupnorm_fused_supported(B, HW, Cc, G, code[dt]) == (1 if want else 0)
          n += st == 0
  assert n > 1000
  assert lib.ldm_groupnorm_fused_form(3, 35, 320, 32, code[BF], None) != 0
  assert lib.ldm_groupnorm_fused_form(3, 35, 320, 32, 99, f) != 0
  for c in CASES:
    if c.kind == "fused":
      assert lib.ldm_groupnorm_fused_form(c.B, c.HW, c.C, c.G, code[c.dt], f) == 0 and tuple(f) == c.form, P.case_id(c)
      assert P.fused_plan(c.B, c.HW, c.C, c.G, c.dt) == c.form
    if c.kind == "pair":
      assert lib.ldm_groupnorm_nchunks(c.B, c.HW, c.C) == P.nchunks_default(c.B, c.HW)
      if c.C // c.G < P.epc(c.dt):
        assert P.fused_plan(c.B, c.HW, c.C, c.G, c.dt) is None
    if c.kind == "ln":
      assert P.ln_lpr(c.C, c.dt) == c.form[0]


def test_plans_256_24_and_512_24_cannot_occur():
  """Enumeration over S = 1 .. 64 and HW = 1 .. 40000: whenever every (NT, 8 | 16) plan refuses a slab, 24 chunks per
  thread at 256 or 512 threads do not hold it either -- the loop that returned them was dead."""
  HW = np.arange(1, 40001)
  for S in range(1, 65):
    need = {NT: -(-HW // (NT // S)) for NT in (256, 512, 1024)}
    reached = (need[256] > 16) & (need[512] > 16) & (need[1024] > 16)
    assert not (reached & ((need[256] <= 24) | (need[512] <= 24))).any(), S
    assert 1024 // S >= 4 * (256 // S) and 1024 // S >= 2 * (512 // S)
  for S, hw in ((5, 817), (5, 3264), (5, 3265), (64, 257), (1, 16385), (20, 817)):
    assert P.old_last_loop(S, hw) is None


def test_case_matrix_reaches_every_form():
  fused = [c for c in CASES if c.kind == "fused"]
  reachable = {(64, 8), (64, 16), (64, 24), (256, 8), (256, 16), (512, 8), (512, 16), (1024, 8), (1024, 16)}
  for dt in (BF, F32):
    mine = [c for c in fused if c.dt == dt]
    assert {c.form[2:] for c in mine} == reachable
    for nt_mc in reachable:
      sub = [c for c in mine if c.form[2:] == nt_mc]
      P_ = [c.form[2] // c.form[1] for c in sub]
      assert any(c.HW % p for c, p in zip(sub, P_)), ("HW % P != 0", dt, nt_mc)
    assert any(c.form[2] % c.form[1] for c in mine) and any(c.form[2] % c.form[1] == 0 for c in mine)
    assert any(P.cpg(c) % P.epc(dt) for c in mine) and any(P.cpg(c) % P.epc(dt) == 0 for c in mine)
    assert any(c.HW < c.form[2] // c.form[1] for c in mine)
    assert any(c.HW == c.form[3] * (c.form[2] // c.form[1]) for c in mine)
    assert any(c.B % 8 for c in mine) and {c.G for c in mine} >= {1, 32, 64}
    assert {c.form[0] for c in ln_of(dt)} == {4, 8, 16, 32, 64}
    assert any((c.C // P.epc(dt)) % c.form[0] for c in ln_of(dt))
    pair = [c for c in CASES if c.kind == "pair" and c.dt == dt]
    assert {c.nchunks for c in pair} >= {0, 1, 3, 7, 128} and {c.G for c in pair} == {8, 32, 64}
    assert {c.B for c in pair} >= {1, 3} and any(c.pilot for c in pair) and max(c.HW for c in pair) <= 1100
    assert any(c.form[0] > -(-c.HW // P.pair_geom(c)[1]) for c in pair), "no case with empty chunks"
    assert any(c.C // P.epc(dt) >= 256 for c in pair) and any(256 % (c.C // P.epc(dt)) for c in pair)
    for c in pair:
      nch, ppc, VT, Pp = P.pair_geom(c)
      assert c.pilot or c.HW % ppc or nch == 1, P.case_id(c)
      assert c.HW % (4 * Pp), P.case_id(c)
  assert any(c.form[0] == 8 for c in fused if c.dt == BF) and any(c.G == 4 for c in fused)
  assert any(c.kind == "pair" and c.dt == BF and P.cpg(c) < 8 for c in CASES)


def ln_of(dt):
  return [c for c in CASES if c.kind == "ln" and c.dt == dt]
