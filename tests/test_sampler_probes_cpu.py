"""Self-check of tests/sampler_probes.py on the CPU: the probes must be able to fail.

Every probe value is exact in its type and every intermediate of the reference is an integer or a fixed dyadic multiple
below 2^24 (so equality is a fair gate on the GPU); the model of the kernels' index arithmetic reproduces every expected
output; every fault of the model changes an output of every case it applies to, and every entry a fault can occur in
has such a case; the written-out reference agrees with the older references of the suite; the numbers and the list of
instantiations are those of csrc/sampler.hip; the case matrix crosses the edges it claims.
"""
import os
import re

import numpy as np
import pytest
import torch

import deis_ref
import guidance_ref
import inversion_ref
import philox_ref as R
import plms_ref
import sampler_probes as P
from oracle import ldm_oracle as O

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ldm_tf2_amd", "csrc")
UPD, FILL = P.update_cases(), P.fill_cases()
BIG = 100000                                  # above this a case is there for the passes: only their faults are run
PASS_FAULTS = ("drop_last", "skip_second_pass", "overlap_second_pass", "b_per_block", "xunet_half_at_n")


def test_numbers_match_the_source():
  txt = open(os.path.join(SRC, "sampler.hip")).read()
  common = open(os.path.join(SRC, "common.h")).read()
  hdr = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
  assert re.search(r"grid_for\(int64_t total, int per_block = 256, int cap = \d+\)", common)
  assert "if (g > cap) g = cap;" in common
  assert txt.count(f"__launch_bounds__({P.BLOCK})") == 6 and txt.count(f"dim3({P.BLOCK})") == 9
  assert f"grid_for(wide ? (int64_t)a.B * a.n / {P.WIDE} : (int64_t)a.B * a.n, {P.BLOCK}, {P.CAP})" in txt
  assert txt.count(f"grid_for((int64_t)B * n_per_sample / {P.WIDE}, {P.BLOCK}, {P.CAP})") == 3
  assert txt.count(f"grid_for((int64_t)B * n_per_sample, {P.BLOCK}, {P.CAP})") == 1
  wide = f"i = ((int64_t)blockIdx.x * {P.BLOCK} + threadIdx.x) * {P.WIDE}; i < total; i += (int64_t)gridDim.x * {P.BLOCK} * {P.WIDE})"
  one = f"i = (int64_t)blockIdx.x * {P.BLOCK} + threadIdx.x; i < total; i += (int64_t)gridDim.x * {P.BLOCK})"
  assert txt.count(wide) == 4 and txt.count(one) == 2
  names = {"kDdim": "ddim", "kAdamsBashforth": "ab", "kTable": "table", "kInvert": "invert", "kScaleArg": "arg",
           "kScaleTable": "table", "kCondOnly": "cond"}
  inst = [("wide", names[h], names[s], r == "true", b == "true")
          for h, s, r, b in re.findall(r"LAUNCH\(cfg_update4_kernel, (\w+), (\w+), (true|false), (true|false)\)", txt)]
  inst += [("scalar", "ddim", "arg", False, b == "true") for b in re.findall(r"LAUNCH\(cfg_ddim_kernel, (true|false)\)", txt)]
  assert len(inst) == 14 and set(inst) == P.INSTANTIATIONS
  for name, val in (("XT", R.XT_STREAM), ("ETA", R.ETA_STREAM), ("ENCODE", R.ENCODE_STREAM), ("Q", R.Q_STREAM)):
    m = re.search(rf"#define LDM_RNG_{name}_STREAM (.*)", hdr)
    assert eval(m.group(1).replace("u", "")) == val


def test_case_ids_are_unique():
  ids = [c.id for c in UPD + FILL]
  assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)


def test_the_matrix_crosses_what_it_claims():
  assert {P.form(c) for c in UPD} == P.INSTANTIATIONS                                       # all 14 behind the switch
  for f in P.INSTANTIATIONS:
    assert {c.xd for c in UPD if P.form(c) == f} >= {F32, BF}, f                            # ... in both x_dtypes
  assert {c.entry for c in FILL} == set(P.FILL_ENTRIES)
  by = lambda e: [c for c in UPD + FILL if c.entry == e]
  for e in P.UPDATE_ENTRIES + P.FILL_ENTRIES:
    cs = by(e)
    assert {c.n for c in cs if c.B == 3} >= {4, 12, 1020, 1028}, e                          # boundaries inside a wave / a workgroup
    if e in P.UPDATE_ENTRIES:
      assert {c.idx % 4 for c in cs} == {0, 1, 2, 3} and any(c.idx == 0 for c in cs), e
      assert any(c.alias for c in cs) and any(not c.alias for c in cs), e
      assert any(c.pred for c in cs) and any(not c.pred for c in cs), e
      assert any(c.dec for c in cs) and any(not c.dec for c in cs), e
      assert any(c.xd is None for c in cs), e
  for e in ("ddim", "ddim_masked", "q_sample"):                                             # the scalar bodies: odd n
    assert any(c.n % 2 for c in by(e)), e
  for e in ("ddim_masked", "ddim_rng", "plms", "plms_rng", "ms", "ms_rng", "sched"):
    on = [c for c in by(e) if P.blend_on(c)]
    assert {c.ch for c in on} >= {1, 2, 3, 4, 6, 8}, e
    assert any(c.blend and c.idx == 0 for c in by(e)), e
    if e not in ("ddim_rng", "plms_rng", "ms_rng"):
      assert {c.q_stride - c.B * c.n for c in on if not P.form(c)[3] and c.q_stride} == {0, 4}, e
      assert any(c.q_stride == 0 for c in on if not P.form(c)[3]), e
  for e in ("plms", "plms_rng", "ms", "ms_rng", "sched"):
    h = [c for c in by(e) if P.has_hist(c)]
    assert {c.start - c.idx for c in h} >= {-1, 0, 1, 2, 3, 7}, e
    assert {(c.idx % 4, P.order(c) > 0) for c in h} >= {(r, True) for r in range(4)}, e      # every ring residue read from
    if e not in ("plms", "plms_rng"):
      assert {c.pitch for c in h} == {16, 20}, e
      assert {(P.order(c), c.hot) for c in h if c.probe == "eps"} >= {(3, m) for m in range(4)}, e
  for e in ("ddim", "ddim_masked", "q_sample"):
    noisy = [c for c in by(e) if c.probe in ("noise", "census_sigma") and getattr(c, "use_index", True)]
    assert {c.noise_stride - c.B * c.n for c in noisy if c.noise_stride} == {0, 4} and any(c.noise_stride == 0 for c in noisy), e
  assert any(not c.use_index for c in by("q_sample"))
  sched = by("sched")
  assert {(c.guided, c.rng, c.weights) for c in sched} >= {(True, False, True), (True, True, True), (False, False, True),
                                                             (False, True, True), (True, False, False), (False, True, False)}
  assert {c.guided for c in by("invert")} == {True, False}
  assert any(c.clip for c in by("ddim")) and any(c.clip for c in by("ddim_masked")) and any(c.clip for c in by("ddim_rng"))
  # per body: one case exactly one pass long, one a quad (an element) past it, and nothing larger
  for body_cases, W in ((by("ddim_masked"), 1), (by("ms") + by("ddim_rng"), 4), (by("q_sample"), 1), (by("q_sample_rng"), 4),
                        (by("normal_fill"), 4), (by("philox_u32"), 4)):
    totals = {c.B * c.n for c in body_cases}
    assert P.ONE_PASS[W] in totals and P.ONE_PASS[W] + W in totals and max(totals) == P.ONE_PASS[W] + W
  for c in UPD + FILL:
    total = c.B * c.n
    assert P.passes(c)[0] == (2 if total > P.ONE_PASS[P.width(c)] else 1)
    # the position code of an element differs from those of its neighbours
    for dist in (1, 4, c.ch, c.n, P.ONE_PASS[P.width(c)], total):
      assert dist % c.P != 0, (c.id, dist)
    assert all((37 * a) % c.P != 0 for a in range(1, P.A_ETA + P.N_ROWS))              # ... and between any two arrays
    assert c.n % c.ch == 0 and (P.width(c) == 1 or c.n % 4 == 0), c.id
  assert any(c.B > 1 and P.passes(c)[0] == 2 and P.form(c)[3] for c in UPD)                # drawn noise in a second pass
  t = P.q_times(5).tolist()
  assert len(set(t)) == 5 and -1 in t and P.Q_STEPS + 5 in t
  assert len({min(max(v, 0), P.Q_STEPS - 1) % 8 for v in t}) == 5                          # five distinct powers of two


def _inputs_are_exact(c, p):
  for name in ("eps", "xt", "ring", "z0", "mask", "q", "noise", "coef", "gtab", "weights", "qcoef", "x0", "sac", "s1m"):
    v = getattr(p, name, None)
    if v is not None:
      ok = torch.isnan(v) | (v.to(F32).to(F64) == v)
      assert bool(ok.all()), name
      if name in ("eps", "xt", "ring", "z0", "q", "noise", "x0"):
        w = v[~torch.isnan(v)]
        assert bool((w == w.round()).all()) and (w.numel() == 0 or float(w.abs().max()) < 2 ** 23), name
        if c.probe.startswith("census"):
          assert bool((w % 24 == 0).all()), name


@pytest.mark.parametrize("c", UPD + FILL, ids=lambda c: c.id)
def test_probe_is_exact_and_the_model_reproduces_it(c):
  p = P.build(c)
  _inputs_are_exact(c, p)
  tr = P.Tracker(2.0 ** -7 if c.entry in ("q_sample", "q_sample_rng") else 0.5)
  want = P.reference(c, p, tr)
  assert tr.dyadic and tr.worst < P.LIMIT, (tr.dyadic, tr.worst)
  assert bool((want.xt_out.to(F32).to(F64) == want.xt_out).all())
  assert want.pred_x0 is None or bool((want.pred_x0.to(F32).to(F64) == want.pred_x0).all())
  assert not bool(torch.isnan(want.xt_out).any())
  assert P.differing(P.model(c, p), want) == []


@pytest.mark.parametrize("c", UPD + FILL, ids=lambda c: c.id)
def test_every_fault_that_applies_is_caught(c):
  p = P.build(c)
  want = P.reference(c, p)
  missed = [f for f in (PASS_FAULTS if c.B * c.n > BIG else P.FAULTS)
            if P.mutation_applies(c, f) and not P.differing(P.model(c, p, f), want)]
  assert missed == []


def test_every_fault_has_a_case_in_every_entry_it_can_occur_in():
  for f in P.FAULTS:
    for e in P.fault_entries(f):
      assert any(c.entry == e and P.mutation_applies(c, f) for c in UPD + FILL), (f, e)


def test_blended_values_stay_out_of_pred_x0_and_the_ring():
  """The guards of the header: pred_x0_out and the ring slot hold the unblended step's values."""
  c = next(c for c in UPD if c.entry == "ms" and P.blend_on(c) and P.order(c) >= 1 and c.pred and c.B * c.n < BIG)
  p = P.build(c)
  want = P.reference(c, p)
  off = P.NS(**{**vars(c), "blend": False})
  p2 = P.build(off)
  assert P.same(want.pred_x0, P.reference(off, p2).pred_x0) and P.same(want.ring, P.reference(off, p2).ring)
  assert not P.same(want.xt_out, P.reference(off, p2).xt_out)


# ---- the written-out reference against the older references of the suite ---------------------------------------------
def _close(a, b):
  a, b = torch.as_tensor(np.asarray(a), dtype=F64), torch.as_tensor(np.asarray(b), dtype=F64)
  return bool((a - b).abs().max() <= 1e-12 * max(1.0, float(b.abs().max())))


def _first(pred):
  return next(c for c in UPD if c.B * c.n < BIG and not c.blend and pred(c))


def _tables(p):
  co = p.coef.view(-1, 4).numpy()
  return co[:, 0], co[:, 1], co[:, 2]


def _hist(c, p, e_i):
  total = c.B * c.n
  return [e_i] + [p.ring[((c.idx + m) & 3) * total:][:total].numpy() for m in range(1, P.order(c) + 1)]


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_reference_agrees_with_plms_ref(j):
  c = _first(lambda c: c.entry == "plms" and P.order(c) == j and c.probe == "census")
  p = P.build(c)
  want = P.reference(c, p)
  total = c.B * c.n
  e_i = (p.eps[:total] + p.gs * (p.eps[total:] - p.eps[:total])).numpy()
  x1, x0 = plms_ref.plms_update(p.xt.numpy(), _hist(c, p, e_i), c.idx, j, *_tables(p))
  assert _close(want.xt_out, x1) and _close(want.pred_x0 if c.pred else x0, x0)


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_reference_agrees_with_deis_ref(j):
  c = _first(lambda c: c.entry == "ms" and P.order(c) == j and c.probe == "census")
  p = P.build(c)
  want = P.reference(c, p)
  total = c.B * c.n
  e_i = (p.eps[:total] + p.gs * (p.eps[total:] - p.eps[:total])).numpy()
  w = p.weights[c.idx * c.pitch + 4 * j:][:j + 1].numpy()
  x1, x0 = deis_ref.ms_update(p.xt.numpy(), _hist(c, p, e_i), c.idx, j, w, *_tables(p))
  assert _close(want.xt_out, x1) and (not c.pred or _close(want.pred_x0, x0))


@pytest.mark.parametrize("guided", [True, False])
def test_reference_agrees_with_guidance_ref(guided):
  c = _first(lambda c: c.entry == "sched" and c.guided == guided and c.weights and P.order(c) >= 2 and c.probe == "census")
  p = P.build(c)
  want = P.reference(c, p)
  total, j = c.B * c.n, P.order(c)
  g = np.where(np.isnan(p.gtab.numpy()), 1.0, p.gtab.numpy())              # (an unguided step is g = 1 there)
  w = p.weights[c.idx * c.pitch + 4 * j:][:j + 1].numpy()
  x1, x0, e_i = guidance_ref.sched_step(p.xt.numpy(), p.eps[:total].numpy() if guided else None, p.eps[total:].numpy(),
                                        _hist(c, p, None)[1:], g, c.idx, j, w, *_tables(p))
  assert _close(want.xt_out, x1) and _close(want.ring[(c.idx & 3) * total:][:total], e_i)


@pytest.mark.parametrize("guided", [True, False])
def test_reference_agrees_with_inversion_ref(guided):
  c = _first(lambda c: c.entry == "invert" and c.guided == guided and c.probe == "census" and (c.gs != 1 or not guided))
  p = P.build(c)
  want = P.reference(c, p)
  total = c.B * c.n
  c1, c2, a_prev = _tables(p)
  x1, x0 = inversion_ref.invert_update(p.xt.numpy(), p.eps[:total].numpy() if guided else None, p.eps[total:].numpy(),
                                       c.gs if guided else 1, c.idx, dict(c1=c1, c2=c2, a_prev=a_prev))
  assert _close(want.xt_out, x1) and (not c.pred or _close(want.pred_x0, x0))


@pytest.mark.parametrize("probe, clip", [("census_sigma", 0), ("census_sigma", 1), ("noise", 0), ("census", 1)])
def test_reference_agrees_with_the_oracle_ddim_update(probe, clip):
  c = _first(lambda c: c.entry == "ddim" and c.probe == probe and bool(c.clip) == bool(clip))
  p = P.build(c)
  want = P.reference(c, p)
  total = c.B * c.n
  co = torch.nan_to_num(p.coef.view(-1, 4), nan=0.0).numpy()
  sched = dict(ddim_sqrt_recip_alphas_cumprod=co[:, 0], ddim_sqrt_recipm1_alphas_cumprod=co[:, 1],
               ddim_alphas_cumprod_prev=co[:, 2], ddim_sigmas=co[:, 3])
  nz = p.noise[c.idx * c.noise_stride:][:total] if p.noise is not None else torch.zeros(total, dtype=F64)
  x1, x0 = O.ddim_update(p.xt, p.eps[:total], p.eps[total:], sched, c.idx, p.gs, nz, dtype=F64, clip_denoised=bool(clip))
  assert _close(want.xt_out, x1) and (not c.pred or _close(want.pred_x0, x0))


def test_q_sample_reference_is_the_gather_of_the_definition():
  c = next(c for c in FILL if c.entry == "q_sample" and c.probe == "x" and c.n == 12)
  p = P.build(c)
  want = P.reference(c, p)
  for b in range(c.B):
    t = min(max(int(p.t[b]), 0), P.Q_STEPS - 1)
    nz = p.noise[c.idx * c.noise_stride + b * c.n:][:c.n]
    assert _close(want.xt_out[b * c.n:(b + 1) * c.n], p.sac[t] * p.x0[b * c.n:(b + 1) * c.n] + p.s1m[t] * nz)
