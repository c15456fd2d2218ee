"""Self-check of tests/small_probes.py on the CPU: the probes must be able to fail.

For every entry point a plain model of the kernel's work decomposition (which item exists, which grid-stride pass owns
it, which lane owns which codebook row, which block owns which slice) reproduces every probe's expected output exactly,
and every switchable fault of that model is caught by at least one case of the entry point; all probe values are exact
in the types used; the case lists cross the thresholds they claim, computed from the numbers in csrc/misc.hip.
"""
import os
import re

import pytest
import torch

import small_probes as P

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldm_tf2_amd", "csrc")


def same(a, b):
  """Equal, NaN where NaN."""
  a, b = a.to(F64), b.to(F64)
  return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_numbers_match_the_source():
  txt = open(os.path.join(SRC, "misc.hip")).read()
  common = open(os.path.join(SRC, "common.h")).read()
  assert f"grid_for(((npix + 3) / 4) * (Cout / 8), 256, {P.LDS_CAP})" in txt             # conv_items' `sized` for the LDS kernel
  assert "const int64_t total = (int64_t)B * H * wg4 * c8n;" in txt and "wg4 = (W + 3) >> 2" in txt   # ... and its items
  assert f"grid_for(npix * (Cout / 4), 256, {P.IN_CAP})" in txt
  assert f"grid_for(npix, {P.OUT_PIX_PER_WG}, {P.OUT_CAP})" in txt
  assert "sizeof(float) <= 64 * 1024" in txt and P.LDS_BYTES == 64 * 1024
  assert f"constexpr int kMinmaxBlocks = {P.MINMAX_BLOCKS};" in txt
  assert f"constexpr int RT = {P.GEMV_RT};" in txt
  assert re.search(rf"grid_for\(int64_t total, int per_block = 256, int cap = {P.DEFAULT_CAP}\)", common)
  for entry in ("ldm_cast", "ldm_embedding", "ldm_post_quant"):         # these take grid_for's defaults
    body = txt[txt.index(f'extern "C" int {entry}('):]
    assert re.search(r"dim3 g\(grid_for\([^,]*\)\);", body[:body.index("return ldm_launch_status")]), entry
  assert "grid_for(pixels * C, 256, 4096)" in txt


# ---- convs ---------------------------------------------------------------------------------------------------
def _conv_probes(c):
  yield "census", P.conv_census(c)
  for ph in c.phases:
    yield f"selection{ph}", P.conv_selection(c, ph)


def _conv_flat(c, x):
  return P.strided(c.B * c.H * c.W, c.Cin, c.xoff, c.xpad, F64, x)[0]


def test_conv_cases_cover_kernels_types_and_thresholds():
  cs = P.conv_cases()
  assert {(c.kernel, c.idt) for c in cs} == {(k, t) for k in ("lds", "in", "out") for t in (F32, BF)}
  for k in ("lds", "in", "out"):
    assert any(P.passes(*P.conv_items(c))[0] >= 2 for c in cs if c.kernel == k), k          # the grid-stride loop runs
    assert any(P.passes(*P.conv_items(c))[0] == 1 for c in cs if c.kernel == k), k
  lds = [c for c in cs if c.kernel == "lds"]
  assert {c.W % 4 for c in lds} == {0, 1, 2, 3}
  assert any(c.W % 4 and P.passes(*P.conv_items(c))[0] >= 2 for c in lds)                  # ragged AND past the cap
  assert any(9 * 4 * c.Cout * 4 <= P.LDS_BYTES < 9 * 4 * (c.Cout + 8) * 4 for c in lds)     # the largest width that fits
  assert any(c.kernel == "in" and c.Cin == 4 and c.Cout % 8 == 0 and 9 * 4 * (c.Cout - 8) * 4 <= P.LDS_BYTES for c in cs)
  out = [c for c in cs if c.kernel == "out"]
  assert {c.Cout for c in out} == {1, 2, 3, 4}
  assert any((c.B * c.H * c.W) % P.OUT_PIX_PER_WG for c in out)
  nvec = {c.Cin // (8 if c.idt == BF else 4) for c in out}
  assert any(n % 8 for n in nvec) and any(n > 8 for n in nvec) and any(n < 8 for n in nvec)
  assert any(c.Cin == 128 and c.Cout == 3 and c.idt == BF and c.H * c.W == 384 * 384 for c in out)
  assert any(c.Cin == 320 and c.Cout == 4 for c in out)
  assert any(c.xoff and c.xpad and c.ooff and c.opad for c in cs)


@pytest.mark.parametrize("c", P.conv_cases(), ids=lambda c: c.id)
def test_conv_probes_are_exact_and_the_model_reproduces_them(c):
  for name, (x, w, bias, exp) in _conv_probes(c):
    assert P.representable(x, c.idt) and P.representable(w, F32) and P.representable(exp, c.odt), name
    assert bias is None or P.representable(bias, F32)
    # every partial sum is a multiple of the smallest term below 2^24 of them: exact in float32 in any order
    if name == "census":
      assert float(exp.abs().max()) / 2.0 ** -3 < 2 ** 24
    assert torch.equal(P.conv_model(c, _conv_flat(c, x), w, bias), exp), name
    assert torch.equal(P.conv_ref64(x, w, bias), exp), name


def test_every_conv_fault_is_caught():
  caught = {(k, f): [] for k in ("lds", "in", "out") for f in P.CONV_FAULTS}
  for c in P.conv_cases():
    big = c.B * c.H * c.W > 10000           # the large cases are here for the passes: the census and the faults of a pass
    probes = [("census", P.conv_census(c))] if big else list(_conv_probes(c))
    faults = ("drop_ragged_group", "skip_second_pass", "one_chunk_pass") if big else P.CONV_FAULTS
    for name, (x, w, bias, exp) in probes:
      flat = _conv_flat(c, x)
      for f in faults:
        if not same(P.conv_model(c, flat, w, bias, f), exp):
          caught[(c.kernel, f)].append(c.id + ":" + name)
  exempt = {("in", "drop_ragged_group"), ("out", "drop_ragged_group"), ("lds", "one_chunk_pass"), ("in", "one_chunk_pass")}
  for key, ids in caught.items():
    assert bool(ids) != (key in exempt), (key, ids[:3])
  # the ragged group and the second pass are caught by the census, the swap by the selection
  assert any(i.endswith("census") for i in caught[("lds", "drop_ragged_group")])
  assert all("selection" in i for i in caught[("lds", "swap_kh_kw")])


# ---- gemv ------------------------------------------------------------------------------------------------------
def test_gemv_cases_and_faults():
  cs = P.gemv_cases()
  assert {c.rows for c in cs} == {1, 3, 5, 64} and {c.N for c in cs} == {1, 6, 1280} and {c.K for c in cs} == {8, 320, 1280, 2048}
  for wdt, epc in ((F32, 4), (BF, 8)):
    mine = [c for c in cs if c.wdt == wdt]
    assert any(c.K < 64 * epc // 8 for c in mine) and any(c.K > 64 * epc for c in mine)      # idle lanes; several passes
    assert any(c.rows > P.GEMV_RT for c in mine) and any(c.N % 4 for c in mine)
    assert any(c.xpad for c in mine) and any(c.ypad for c in mine)
  caught = {f: 0 for f in P.GEMV_FAULTS}
  for c in cs:
    x, w, b = P.gemv_exact(c)
    exp = x @ w.t() + b
    assert float(x.abs().max() * w.abs().max()) * c.K + 9 < 2 ** 24
    assert P.representable(x, F32) and P.representable(w, c.wdt) and P.representable(exp, F32)
    flat = P.strided(c.rows, c.K, 0, c.xpad, F64, x)[0]
    assert torch.equal(P.gemv_model(c, flat, w, b), exp)
    for f in P.GEMV_FAULTS:
      caught[f] += not same(P.gemv_model(c, flat, w, b, f), exp)
  assert all(caught.values()), caught


# ---- vq_nearest --------------------------------------------------------------------------------------------------
def test_vq_cases_and_faults():
  cs = P.vq_cases()
  assert {c.V for c in cs} >= {1, 63, 64, 65, 1000, 16384} and {c.C for c in cs} >= {1, 3, 4, 8}
  assert any(c.rows % 4 for c in cs) and any(c.rows % 4 == 0 for c in cs)
  kinds = set()
  caught = {f: 0 for f in P.VQ_FAULTS}
  for c in cs:
    z, cb, idx, q = P.vq_data(c)
    d = (z[:, None, :] - cb[None, :, :]).pow(2).sum(-1)
    assert float(d.max()) < 2 ** 24 and P.representable(z, F32) and P.representable(cb, F32)
    # the kernel's form |z|^2 + |e|^2 - 2 z.e in integers: the same distances
    assert torch.equal((z * z).sum(1)[:, None] + (cb * cb).sum(1)[None, :] - 2 * z @ cb.t(), d)
    assert torch.equal(idx, torch.argmin(d, dim=1))
    for s in P.vq_plants(c.V, c.C):
      rows = (idx == s[0]).nonzero().flatten() if len(s) == 1 else (idx == min(s)).nonzero().flatten()
      assert rows.numel(), (c.id, s)                                   # some z row aims at every plant
      if len(s) == 2:
        assert bool((d[rows][:, s[0]] == d[rows][:, s[1]]).all())     # a real tie
        a, b = s
        kinds.add("same_lane" if a % 64 == b % 64 else ("low_index_high_lane" if min(s) % 64 > max(s) % 64 else "other"))
        kinds.add("last_row" if max(s) == c.V - 1 else "")
    assert torch.equal(P.vq_model(c, z, cb), idx), c.id
    for f in P.VQ_FAULTS:
      caught[f] += not torch.equal(P.vq_model(c, z, cb, f), idx)
  assert {"same_lane", "low_index_high_lane", "last_row"} <= kinds
  assert all(caught.values()), caught


def test_vq_all_distances_infinite():
  """The case the kernel's lane seeding exists for: the model with seeded lanes gives the oracle's indices (row 0 where
  every distance is +inf); a model whose lanes hold no row until a distance is below +inf does not."""
  from oracle import ldm_oracle as O
  z, cb = P.vq_overflow_data()
  assert bool(torch.isfinite(z).all()) and int(torch.isinf((z * z).sum(1)).sum()) == 3
  d = P.vq_distances_f32(z, cb)
  over = torch.isinf(d).all(1)
  assert int(over.sum()) == 3 and bool(torch.isfinite(d[~over]).all())
  _, idx = O.vq_nearest(z, cb)
  assert bool((idx[over] == 0).all()) and torch.equal(idx[~over], P.first_min(d[~over]))
  c = P.NS(V=cb.shape[0], C=cb.shape[1], rows=z.shape[0])
  assert torch.equal(P.vq_model(c, z, cb, d=d), idx)
  for f in P.VQ_OVERFLOW_FAULTS:
    bad = P.vq_model(c, z, cb, f, d=d)
    assert bool((bad[over] == 0x7fffffff).all()) and torch.equal(bad[~over], idx[~over])


# ---- minmax_u8 -----------------------------------------------------------------------------------------------
def test_minmax_cases_and_faults():
  assert P.u8_safe() == list(range(256))                 # (v / 255) * 255 truncates back to v for every byte value
  cs = P.minmax_cases()
  assert {c.n for c in cs} >= {2, 255, 256, 257, 64 * 256 - 1, 64 * 256 + 1} and any(c.n % 256 and c.n > 100000 for c in cs)
  assert {c.dt for c in cs} == {F32, BF}
  placed = set()
  caught = {f: 0 for f in P.MINMAX_FAULTS}
  for c in cs:
    x = P.minmax_data(c)
    assert int(x.min()) == 0 and int(x.max()) == 255 and P.representable(x.to(F64), c.dt)
    for b, (mn, mx) in enumerate(c.places):
      assert int((x[b] == 0).sum()) == 1 and int((x[b] == 255).sum()) == 1
      placed |= {("min", mn, b > 0), ("max", mx, b > 0)}
      pos = P.minmax_positions(c.n)
      if "blk63" in pos:
        assert (pos["blk63"] // 256) % P.MINMAX_BLOCKS == P.MINMAX_BLOCKS - 1
    assert torch.equal(P.minmax_model(c, x), x), c.id
    for f in P.MINMAX_FAULTS:
      caught[f] += not torch.equal(P.minmax_model(c, x, f), x)
  assert placed == {(m, p, b) for m in ("min", "max") for p in ("first", "last", "blk63") for b in (False, True)}
  assert all(caught.values()), caught


# ---- cast --------------------------------------------------------------------------------------------------------
def test_cast_cases_and_faults():
  cs = P.cast_cases()
  assert {(c.idt, c.odt) for c in cs} == {(a, b) for a in (F32, BF) for b in (F32, BF)}
  assert all(any(c.rows * c.cols > P.DEFAULT_CAP * 256 and (c.idt, c.odt) == k for c in cs) for k in {(c.idt, c.odt) for c in cs})
  sp = torch.tensor(P.CAST_SPECIAL, dtype=torch.int64)
  ties = sp[(sp & 0xffff) == 0x8000]
  assert {int(v) & 1 for v in (ties >> 16)} == {0, 1}                   # both parities of the lower neighbour
  assert {0x80000000, 0x7f800000, 0xff800000, 0x7fc00000} <= set(P.CAST_SPECIAL)
  caught = {f: 0 for f in P.CAST_FAULTS}
  for c in cs:
    x = P.cast_data(c)
    if c.idt == F32:
      assert torch.equal(P.bits_of(x).flatten()[:len(sp)].to(torch.int64) & 0xffffffff, sp)
    flat, view = P.strided(c.rows, c.cols, c.xoff, c.xpad, c.idt)
    view.copy_(x)
    want = x.to(c.odt)
    assert P.same_bits(P.cast_model(c, flat), want)
    for f in P.CAST_FAULTS:
      caught[f] += not P.same_bits(P.cast_model(c, flat, f), want)
  assert all(caught.values()), caught


# ---- embedding -------------------------------------------------------------------------------------------------
def test_embedding_cases_and_faults():
  cs = P.embedding_cases()
  assert {c.odt for c in cs} == {F32, BF} and any(c.rows * c.T * c.D > P.DEFAULT_CAP * 256 for c in cs)
  caught = {f: 0 for f in P.EMB_FAULTS}
  for c in cs:
    ids, tok, pos = P.embedding_data(c)
    assert {-1, c.vocab, c.vocab + 5} <= set(ids.flatten().tolist())
    want = (tok[ids.clamp(0, c.vocab - 1)] + pos[None]).to(c.odt)
    assert torch.equal(P.embedding_model(c, ids, tok, pos), want)
    for f in P.EMB_FAULTS:
      caught[f] += not same(P.embedding_model(c, ids, tok, pos, f), want)
  assert all(caught.values()), caught


# ---- the float64 comparisons: the case lists and the references ----------------------------------------------------
def test_float64_case_lists():
  from oracle import ldm_oracle as O
  pq = P.post_quant_cases()
  assert {(c.C, c.sf, c.bias, c.odt) for c in pq} >= {(a, s, b, t) for a in (3, 4, 8) for s in (0.18215, 1.0) for b in (0, 1) for t in (F32, BF)}
  assert any(c.shape[0] * c.shape[1] * c.shape[2] > P.DEFAULT_CAP * 256 for c in pq)
  c = pq[0]
  z, k, b = P.post_quant_data(c)
  assert float((O.dense(z / c.sf, k, b).to(F64) - P.post_quant_ref64(c, z, k, b)).abs().max()) < 1e-4
  g = P.gaussian_cases()
  assert any(c.shape[0] * c.shape[1] * c.shape[2] * c.C > 4096 * 256 for c in g)
  mom, noise = P.gaussian_data(g[0])
  assert float((O.diagonal_gaussian(mom, noise)[2].to(F64) * g[0].scale - P.gaussian_ref64(g[0], mom, noise)).abs().max()) < 1e-2
  sm = P.softmax_cases()
  assert {(c.cols, c.idt, c.odt) for c in sm} == {(n, a, b) for n in P.SOFTMAX_COLS for a in (F32, BF) for b in (F32, BF)}
  assert set(P.SOFTMAX_COLS) >= {1, 63, 64, 65, 255, 256, 257, 1000, 4096}
  for c in sm[:9]:
    x = P.softmax_data(c)
    assert P.representable(x, c.idt)
    ref = P.softmax_ref64(c, x)
    assert float((ref.sum(1) - 1).abs().max()) < 1e-12
    if c.cols > 1:
      assert float(ref[2].max()) > 0.99                                   # the dominant logit
  # the conv reference against the oracle's convolution
  cc = P.conv_cases()[0]
  x, w, bias = P.conv_random(cc)
  assert float((P.conv_ref64(x, w, bias) - O.conv2d(x, w, bias)).abs().max()) < 1e-12
  gm = P.gemv_cases()[5]
  x, w, b = P.gemv_random(gm)
  for ai, ao in P.GEMV_ACTS.values():
    assert float((P.gemv_ref64(x, w, b, ai, ao) - P.gemv_oracle(x, w, b, ai, ao, O)).abs().max()) < 1e-4
  assert sorted(P.GEMV_ACTS.values()) == [(0, 0), (0, 1), (1, 0)]


def test_time_embedding_model_and_faults():
  from oracle import ldm_oracle as O
  steps = P.step_table()
  assert len(steps) == 50
  caught = {f: 0 for f in P.TIME_FAULTS}
  for channels in P.TIME_CHANNELS:
    t = torch.arange(1000, dtype=torch.int32)
    ref = P.time_ref64(t, channels)
    assert float((O.get_time_embedding(t.numpy(), channels).to(F64) - ref).abs().max()) < 2e-3
    assert torch.equal(P.time_model(t, None, None, 1000, channels), ref)
    for i in (0, 7, 49):
      refi = P.time_ref64(steps[i:i + 1], channels).expand(3, -1)
      assert torch.equal(P.time_model(None, steps, i, 3, channels), refi)
      for f in P.TIME_FAULTS:
        caught[f] += not same(P.time_model(None, steps, i, 3, channels, f), refi)
  assert all(caught.values()), caught
  # the frequency check sees an error in the 6th digit of the constant, and the float32 oracle passes it
  for channels in (320, 321, 1280):
    f, k = P.freqs_from_sines(O.get_time_embedding([1], channels)[0], channels)
    want = P.freqs64(channels)[k]
    assert float(((f - want).abs() / want).max()) <= P.FREQ_BOUND
    half = channels // 2
    wrong = torch.sin(torch.exp(-9.2104 * torch.arange(half, dtype=F64) / half)).to(F32)      # ln(1e4) = 9.21034...
    fw, _ = P.freqs_from_sines(torch.cat([torch.zeros(half), wrong]), channels)
    assert float(((fw - want).abs() / want).max()) > P.FREQ_BOUND


def test_every_gate_is_set_with_one_significant_digit():
  """Every (entry point, type) a GPU case asks for has a measured gate: a finite number with one significant digit."""
  keys = {("conv_" + c.kernel, P.DTN[c.idt], P.DTN[c.odt]) for c in P.conv_cases() if c.rand}
  keys |= {("gemv", P.DTN[c.wdt]) for c in P.gemv_cases()} | {("post_quant", P.DTN[c.odt]) for c in P.post_quant_cases()}
  keys |= {("softmax_rows", P.DTN[c.idt], P.DTN[c.odt]) for c in P.softmax_cases()}
  keys |= {("gaussian_sample", "f32"), ("time_embedding", "f32")}
  assert set(P.GATES) == keys
  for k, v in P.GATES.items():
    assert 0 < v < 1e3 and P.one_digit_up(v) == v, (k, v)
  assert P.one_digit_up(2.3) == 3.0 and P.one_digit_up(0.95) == 1.0 and P.one_digit_up(14.0) == 20.0
