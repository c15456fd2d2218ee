"""The activation-epilogue probes of tests/gemm_probes.py are as sharp as claimed, shown without a GPU for every case
test_zz_gemm_epilogue_gpu.py runs.

* adding `act` to gemm_probes.Case left the accounting matrix alone: the ids of all_cases() equal the list recorded from
  the parent commit (tests/golden/gemm_case_ids.json);
* per case: every operand is exact in its storage type, every pre-activation value z is a multiple of 2^-4 with
  |z| <= 4 and exact in float32; for GEGLU the gate differs between neighbouring columns and from its value column;
* every mutation of gemm_probes.EPI_MUTATIONS moves some element of the reference by more than 8 times that element's
  ceiling wherever it applies;
* the matrix holds every store path per activation and form, and the rejections;
* reference_act equals oracle.ldm_oracle's gelu / silu once per activation;
* host plan (no launch): GEGLU that cannot take the vector epilogue is never planned on a 16x16x32 tile unsplit.
"""
import ctypes as C
import json
import os

import pytest
import torch

import gemm_probes as G

CASES = G.epilogue_cases()
HERE = os.path.dirname(os.path.abspath(__file__))


def test_accounting_case_ids_unchanged():
  want = json.load(open(os.path.join(HERE, "golden", "gemm_case_ids.json")))
  assert [G.case_id(c) for c in G.all_cases()] == want
  assert all(c.act == 0 and not c.boff and not c.lnf and not c.rej for c in G.all_cases())


def test_one_grid_step_moves_the_activations():
  """On the 2^-4 grid up to |z| = 4 a step moves GELU and SiLU by at least 3.4e-5: 17 float32 ceilings."""
  z = torch.arange(-64, 65, dtype=G.F64) / 16
  for f in (G.gelu64, G.silu64):
    assert float((f(z[1:]) - f(z[:-1])).abs().min()) >= 3.4e-5 > 8 * G.CEIL_F32


def test_matrix_coverage():
  assert len(CASES) <= 430
  run = [c for c in CASES if not c.rej]
  for act, tiles in (("gelu", G._EPI_TILES), ("silu", G._EPI_TILES), ("geglu", G._GEGLU_TILES)):
    for name in G._forms_of(tiles):
      f = G.FORMS[name]
      tags = {c.tag for c in CASES if c.form == name and c.act == act and c.kind == "plain"}
      assert tags >= ({"vec", "off8", "ldc4", "boff"} | ({"sk2", "sk2off8"} if f.tile else set())), (name, act, tags)
    mine = [c for c in run if c.act == act and c.kind == "plain" and G.FORMS[c.form].tile not in G.PERSISTENT]
    wide = 64 if act == "geglu" else 8
    assert {c.M == 1 for c in mine} == {True, False}
    assert {c.N == wide for c in mine} == {True, False}
    assert {(c.bias, c.addend, c.res) for c in mine} == ({(1, 0, 0), (1, 0, 1)} | ({(1, 1, 0)} if act != "geglu" else set()))
    assert all(c.add_rows < c.M for c in mine if c.addend and c.M > 1) and any(c.addend and c.M > 1 for c in mine) or act == "geglu"
    assert all(c.ldr_x for c in mine if c.res)
    assert {(G.FORMS[c.form].dt, c.odt) for c in mine} == {(G.BF, G.BF), (G.BF, G.F32), (G.F32, G.F32)}
    assert any(c.defer for c in mine)
    pers = [c for c in run if c.act == act and G.FORMS[c.form].tile in G.PERSISTENT]
    assert {G.FORMS[c.form].wg for c in pers} == {-1, 0}
    assert {G.FORMS[c.form].tile for c in pers} == ({14} if act == "geglu" else {13, 14})
  assert sum(c.lnf for c in run) == 2 and all(c.act == "geglu" for c in run if c.lnf)
  assert {(G.FORMS[c.form].tile, c.act) for c in run if c.kind == "tstore"} >= {(2, "gelu"), (2, "silu"), (11, "gelu"), (11, "silu")}
  assert {G.FORMS[c.form].tile for c in run if c.kind == "conv" and c.act == "silu"} == {2, 11}
  rej = [c for c in CASES if c.rej]
  assert {c.rej for c in rej} == {G.ALIGN_REJ, G.ADDEND_REJ, "no kernel for this epilogue", "GEGLU needs a tile"}
  # finding 1: unsplit GEGLU on the 16x16x32 tiles off the vector epilogue; finding 2: GEGLU with an addend
  assert {(G.FORMS[c.form].tile, c.tag) for c in rej if c.rej == G.ALIGN_REJ} == {(t, p) for t in (11, 12) for p in ("off8", "ldc4", "boff")}
  assert {G.FORMS[c.form].tile for c in rej if c.rej == G.ADDEND_REJ} == set(G._GEGLU_TILES)
  assert {c.tag for c in rej if c.rej == G.ADDEND_REJ} == {"vec", "off8", "sk2", "defer"}


@pytest.mark.parametrize("act", ["gelu", "silu", "geglu"])
def test_exactness_and_mutations(act):
  for c in CASES:
    if c.act != act:
      continue
    cid = G.epi_id(c)
    f = G.FORMS[c.form]
    d = G.probe_epilogue(c)
    for name, t in (("a", f.dt), ("w", f.dt), ("bias", G.F32), ("addend", G.F32), ("res", c.odt), ("cs", G.F32)):
      if name in d:
        assert G.representable(d[name], t), (cid, name)
    z = G.reference_pre(c, d)
    assert float(z.abs().max()) <= 4.0 and bool((z * 16 == (z * 16).round()).all()) and G.representable(z, G.F32), cid
    assert len(torch.unique(z)) >= min(16, z.numel() // 4), cid
    if act == "geglu":
      nv, ng = G.geglu_cols(c)
      g = z[..., ng]
      assert float((g != z[..., (ng + 1) % c.N]).double().mean()) > 0.8, cid
      assert float((g != z[..., nv]).double().mean()) > 0.8, cid
    ref, ce = G.reference_act(c, d), G.ceiling(c, d)
    assert bool(torch.isfinite(ref).all()) and tuple(ref.shape) == (1, c.M, G.nout_of(c)), cid
    for kind in G.EPI_MUTATIONS:
      if G.epi_mutation_applies(c, kind):
        assert bool(G.exceeds(G.reference_act(c, d, kind), ref, ce, G.MUTATION_FACTOR).any()), (cid, kind)
    groups = G.uniformity_groups(c, d)
    assert G.not_uniform(ref, groups) == 0, cid
    if c.M > 1:
      assert int(groups.max()) + 1 < groups.numel(), cid                    # some (z, residual) occurs twice


def test_mutations_are_all_exercised():
  for kind in G.EPI_MUTATIONS:
    assert any(G.epi_mutation_applies(c, kind) for c in CASES), kind
  # the two findings as the matrix holds them: the mutation exists for the cases that must now be rejected
  assert all(c.rej == G.ADDEND_REJ for c in CASES if G.epi_mutation_applies(c, "geglu_gate_addend_missing"))


@pytest.mark.parametrize("act", ["gelu", "silu", "geglu"])
def test_reference_against_the_oracle(act):
  from oracle import ldm_oracle as O
  c = next(c for c in CASES if c.act == act and c.M > 1 and c.res and not c.rej and c.odt == G.F32)
  d = G.probe_epilogue(c)
  z = G.reference_pre(c, d)[0]
  if act == "geglu":
    zz = z.reshape(c.M, c.N // 64, 2, 32)                                  # blocks of 64 = 32 value rows, 32 gate rows
    want = (zz[:, :, 0] * O.gelu(zz[:, :, 1])).reshape(c.M, c.N // 2)
  else:
    want = (O.gelu if act == "gelu" else O.silu)(z)
  want = want + d["res"][:, :G.nout_of(c)]
  assert float((G.reference_act(c, d)[0] - want).abs().max()) <= 4e-15
  assert float((G.oracle_act(c, d, O)[0] - want).abs().max()) <= 1e-5       # the float32 oracle of the measured gate


def _geglu_params(L, tile, split, M, N, K, out=0x1000, ldc=None, bias=0x2000, addend=0):
  p = L.GemmParams()
  p.a, p.w, p.out, p.bias, p.addend = 0x100000, 0x200000, out, bias, addend or None
  p.M, p.N, p.K, p.batch = M, N, K, 1
  p.lda, p.ldc_m, p.ldc_n = K, (N // 2 if ldc is None else ldc), 1
  p.add_rows = M
  p.act, p.dtype, p.out_dtype, p.alpha = L.ACT_GEGLU, L.BF16, L.BF16, 1.0
  p.tile, p.split_k = tile, split
  p.workspace, p.workspace_bytes = 0x400000, 96 << 20
  return p


def test_plan_keeps_unaligned_geglu_off_the_16x16x32_tiles():
  """Host queries only: nothing is launched.  With today's step times the cost model prefers tile 2 to tile 11 for every
  GEGLU shape, so this holds before the guard in choose() as well; it pins the guard against a retuned model."""
  from ldm_tf2_amd import _lib as L
  t, s = C.c_int(), C.c_int()
  for M, N, K in ((8192, 2560, 320), (4096, 1280, 1280), (257, 192, 128), (64, 5120, 640), (1, 64, 2560)):
    for kw in (dict(), dict(out=0x1008), dict(ldc=N // 2 + 4), dict(bias=0x2004)):
      p = _geglu_params(L, 0, 0, M, N, K, **kw)
      assert L.lib.ldm_gemm_plan(C.byref(p), C.byref(t), C.byref(s)) == 0
      assert L.lib.ldm_gemm_splits(C.byref(p)) == s.value
      assert t.value in (1, 2, 5, 11, 12, 19), (M, N, K, kw, t.value)
      assert not kw or t.value not in (11, 12) or s.value > 1, (M, N, K, kw, t.value, s.value)
