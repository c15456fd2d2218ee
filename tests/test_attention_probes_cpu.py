"""The attention probes (tests/attn_probes.py) are as sharp as claimed: shown in float64, without a GPU, for every shape
of the matrix test_attention_accounting_gpu.py runs.

* the matrix reaches every Tq / Tk value of every form at least twice and holds the three layout forms;
* probe 1: the reference equals count_d / Tk, one key more or less is >= 8 ulp of the storage type;
* probe 2: the softmax puts >= 1 - 1e-9 on the selected key, the pinned rows hit the tile edges;
* probe 3: integer logits on the two levels, half the rows meet their first high key in the last tile, a quarter start
  with a negative first tile, and sum_k 2^(n_k - n_min) |v_kd| < 2^24 for every row;
* probe 4: the recorded c covers what the bf16 model / the float32 oracle need today;
* mutation check: the reference with key Tk - 1 dropped, with key 0 counted twice, with two query rows swapped FAILS the
  gate.  Two mutations cannot change a correct result and are exempt where that is so: a second copy of the ONLY key
  (Tk = 1: the softmax of one key is 1 either way), and in probe 2 a second copy of a key the one-hot row either
  selects (same value) or does not (weight < 1e-9); doubling is judged by probes 1 and 3, swapping by probe 2.
"""
import math

import pytest
import torch

import attn_probes as A

CASES = A.all_cases()
BY_FORM = {name: [c for c in CASES if c.form == name] for name in A.FORMS}
MS_FORMS = [n for n, f in A.FORMS.items() if f.kind in ("ms", "xtail")]


def test_matrix_reaches_every_size_twice():
  for name, form in A.FORMS.items():
    cs = BY_FORM[name]
    for tq in A.tq_values(form):
      assert len({c.Tk for c in cs if c.Tq == tq}) >= 2, (name, tq)
    for tk in A.tk_values(form):
      assert len({c.Tq for c in cs if c.Tk == tk}) >= 2, (name, tk)
    assert {c.R for c in cs} <= {2, 3} and all(1 <= c.H <= 8 for c in cs)
    assert {c.ldvt_extra for c in cs} == {0, 8}
    if form.kind != "xtail":
      assert any(c.shared_qk and c.Tq == c.Tk for c in cs) and any(c.out_wide for c in cs)
  f4, f8 = A.FORMS["ms4-bf16"], A.FORMS["ms8-bf16"]
  assert max(A.tq_values(f4)) < 256 <= min(A.tq_values(f8))          # both sides of the dispatch's switch
  assert {1, 2, 3, 4} <= {-(-tk // f8.KT) for tk in A.tk_values(f8)}   # 1..4 key tiles for the two-buffer loop


@pytest.mark.parametrize("name", list(A.FORMS))
def test_census_probe_and_its_mutations(name):
  form = A.FORMS[name]
  sc, base = A.scale_base(form, 1)
  for c in BY_FORM[name]:
    q, k, v = A.probe_census(form, c)
    ref, _ = A.attn_ref64(q, k, v, sc, base)
    want = (A.census_counts(c, form.S) / c.Tk).view(c.R, 1, c.H, form.S).expand_as(ref)
    assert (ref - want).abs().max() <= 1e-15, A.case_id(c)
    assert A.census_excess(A.rounded(want, form.dtype), ref, form.dtype) <= 1.0           # the exact answer passes
    # one key more or less moves a non-zero output by 1 / Tk: at least 8 ulp of the storage type
    ulp = A.bf16_ulp(want) if form.dtype == A.BF else 2.0 ** -23 * want.abs()
    assert (1.0 / c.Tk >= 8 * ulp[want > 0]).all(), A.case_id(c)
    for kind in ("drop_last_key", "double_key0"):
      if kind == "double_key0" and c.Tk == 1:
        continue
      bad = A.mutated_ref64(q, k, v, sc, base, kind)
      assert A.census_excess(bad, ref, form.dtype) > 1.0, (A.case_id(c), kind)


@pytest.mark.parametrize("name", list(A.FORMS))
def test_selection_probe_and_its_mutations(name):
  form = A.FORMS[name]
  sc, base = A.scale_base(form, 2)
  worst_oracle = 0.0
  for c in BY_FORM[name]:
    q, k, v, pi = A.probe_selection(form, c)
    assert (A.rounded(q, form.dtype) == q).all() and (A.rounded(k, form.dtype) == k).all()
    gram = A.codes(form.S, c.Tk) @ A.codes(form.S, c.Tk).t()
    assert c.Tk == 1 or torch.triu(gram, 1).max() <= A.max_product(form.S)
    w = A.selected_weight(q, k, sc, base, pi)
    assert w.min() >= 1 - 1e-9, (A.case_id(c), 1 - float(w.min()))
    for row, key in ((0, 0), (31, form.KT - 1), (32, form.KT), (c.Tq - 1, c.Tk - 1)):
      if row < c.Tq and (row == c.Tq - 1) == (key == c.Tk - 1):
        assert (pi[:, :, row] == min(key, c.Tk - 1)).all()
    ref, _ = A.attn_ref64(q, k, v, sc, base)
    sel = torch.gather(v.permute(0, 2, 1, 3), 2, pi.unsqueeze(3).expand(-1, -1, -1, form.S)).permute(0, 2, 1, 3)
    assert (ref - sel).abs().max() <= 1e-8
    assert A.selection_excess(A.rounded(sel, form.dtype), ref, form.dtype) <= 1.0
    for kind in ("drop_last_key", "swap_rows"):
      bad = A.mutated_ref64(q, k, v, sc, base, kind)
      assert A.selection_excess(bad, ref, form.dtype) > 1.0, (A.case_id(c), kind)
    if form.dtype == A.F32:
      worst_oracle = max(worst_oracle, A.selection_excess(A.oracle_f32(q, k, v), ref, A.F32) * A.SELECT_F32_FACTOR)
  if form.dtype == A.F32:
    print(f"{name}: float32 oracle on probe 2: {worst_oracle:.4f} x 2^-24 max(|ref|, 2^-6)")
    assert worst_oracle <= A.ORACLE_SELECT_F32 <= A.SELECT_F32_FACTOR / 2


@pytest.mark.parametrize("name", MS_FORMS)
def test_power_of_two_probe_and_its_mutations(name):
  form = A.FORMS[name]
  sc, base = A.scale_base(form, 3)
  assert (sc, base) == (1.0, 2)
  for c in BY_FORM[name]:
    assert c.Tk <= 512
    q, k, v, logits, rc = A.probe_pow2(form, c)
    for t in (q, k, v):
      assert (A.rounded(t, A.BF) == t).all()
    assert (logits == logits.round()).all()
    l0 = torch.tensor(A.P3_L0, dtype=A.F64)[rc % 4].permute(0, 2, 1).unsqueeze(3)       # [R, H, Tq, 1]
    lv = logits - l0
    low, high = (lv >= 0) & (lv <= 3), (lv >= 9) & (lv <= 11)
    assert (low | high).all() and high.any(dim=3).all()
    last0 = (c.Tk - 1) // form.KT * form.KT
    late = ((rc % 4) < 2).permute(0, 2, 1)                                                # [R, H, Tq]
    first_high = high.to(torch.int64).argmax(dim=3)
    assert (first_high[late] >= last0).all()
    if c.Tq >= 16:
      assert abs(float(late.double().mean()) - 0.5) <= 0.1
      negative_first = (logits[..., :form.KT].max(dim=3).values < 0)
      assert float(negative_first.double().mean()) >= 0.2
    # exactness: every partial sum, scaled to the smallest weight of its row, is an integer below 2^24
    wrel = torch.exp2(logits - logits.min(dim=3, keepdim=True).values)
    assert wrel.max() <= 2.0 ** 11
    bound = torch.einsum("nhqc,nchs->nqhs", wrel, v.abs())
    assert max(float(bound.max()), float(wrel.sum(dim=3).max())) < 2.0 ** 24, A.case_id(c)
    ref, _ = A.attn_ref64(q, k, v, sc, base)
    assert A.selection_excess(A.rounded(ref, A.BF), ref, A.BF) <= 1.0
    for kind in ("drop_last_key", "double_key0"):
      if kind == "double_key0" and c.Tk == 1:
        continue
      bad = A.mutated_ref64(q, k, v, sc, base, kind)
      assert A.selection_excess(bad, ref, A.BF) > 1.0, (A.case_id(c), kind)


@pytest.mark.parametrize("name", list(A.FORMS))
def test_running_bound_constant_covers_the_reference_computation(name):
  """c of probe 4 is 4 x what a reference computation of the storage type needs: the recorded figure must cover this
  form's shapes (and the gate then leaves that computation a factor >= 4 / (1 + 1 / c) of room)."""
  form = A.FORMS[name]
  sc, base = A.scale_base(form, 4)
  for variant in A.P4_VARIANTS:
    need = 0.0
    for c in BY_FORM[name]:
      q, k, v = A.probe_random(form, c, variant)
      for t in (q, k, v):
        assert (A.rounded(t, form.dtype) == t).all()
      ref, absref = A.attn_ref64(q, k, v, sc, base)
      if form.dtype == A.BF:
        models = [A.bf16_model(q, k, v, sc, base, rd) for rd in (False, True)]
      else:
        models = [A.oracle_f32(q, k, v)]
      for m in models:
        need = max(need, A.c_needed(m, ref, absref, form.dtype))
        assert A.bound_excess(m, ref, absref, form.dtype, variant) <= 1.0
    print(f"{name} {variant}: reference computation needs c = {need:.2f}, gate uses {A.c_of(form.dtype, variant):.1f}")
    assert need <= A.MODEL_C[(form.dtype, variant)]
    assert A.c_of(form.dtype, variant) == max(2.0, 4 * A.MODEL_C[(form.dtype, variant)])


def test_pack_and_unpack_are_inverse_and_pads_are_nan():
  for name in ("attn96-bf16", "ms4-bf16", "wide-f32"):
    form = A.FORMS[name]
    for c in BY_FORM[name][-3:]:
      q, k, v = A.probe_random(form, c, "plain")
      qd, kd, vt, out, ob = A.pack(form, c, q, k, v, "cpu")
      W = c.H * form.Sp
      assert qd.shape == (c.R, c.Tq, W) and kd.shape == (c.R, c.Tk, W) and vt.shape[:2] == (c.R, W)
      assert vt.shape[2] == A.roundup8(c.Tk) + c.ldvt_extra and torch.isnan(vt[:, :, c.Tk:]).all()
      assert torch.isnan(ob).all() and qd.stride(0) > c.Tq * qd.stride(1)
      if c.shared_qk:
        assert qd.stride(1) == kd.stride(1) == 2 * W and qd.data_ptr() != kd.data_ptr()
      assert (qd.double().reshape(c.R, c.Tq, c.H, form.Sp)[..., :form.S] == q).all()
      assert (vt[:, :, :c.Tk].double().permute(0, 2, 1).reshape(c.R, c.Tk, c.H, form.Sp)[..., :form.S] == v).all()
      if form.kind == "ms":
        assert (kd.double().reshape(c.R, c.Tk, c.H, form.Sp)[..., A.MS_DIM] == 1).all()
      out.copy_(qd)
      got, pad, rest = A.unpack(form, c, out, ob)
      assert (got == q).all() and (pad == 0).all() and (rest is None or torch.isnan(rest).all())
