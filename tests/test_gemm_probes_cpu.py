"""The GEMM / convolution probes (tests/gemm_probes.py) are as sharp as claimed: shown on the reference alone, without a
GPU, for every case of the matrix test_gemm_accounting_gpu.py runs.

* the tile table agrees with the library's own (ldm_gemm_tile_info), with ops._TILE_DIMS and with the plan ldm_gemm makes;
* the matrix holds, per form, every M, N and K-tile edge value relative to that form's bm, bn and ring depth, every
  image geometry and convolution form, the layouts and the split-K shapes;
* per case: every stored value is exactly representable (|ref| <= 256 where the output is bf16), every partial sum is
  below 2^24, every K column is alive in every (M-tile, N-tile), the slab count is what ldm_gemm_splits answers;
* probe 1: the position code differs between neighbours, the phases select every K-tile (hence every tap);
* every mutation of gemm_probes.MUTATIONS changes the reference wherever it applies;
* the reference equals oracle.ldm_oracle.conv2d / upsample_nearest2x / a float64 matmul once per mode.
"""
import ctypes as C

import pytest
import torch

import gemm_probes as G

CASES = G.all_cases()
BY_FORM = {name: [c for c in CASES if c.form == name] for name in G.FORMS}


def test_tile_table_matches_the_sources():
  from ldm_tf2_amd import _lib as L, ops
  lib, info, rows = L.lib, L.TileInfo(), {}
  assert lib.ldm_gemm_tile_count() == 20
  for t in (0, 20, -1):
    assert lib.ldm_gemm_tile_info(t, C.byref(info)) == L.ERR_ARG
  for t in range(1, 20):
    assert lib.ldm_gemm_tile_info(t, C.byref(info)) == 0
    rows[t] = (info.bm, info.bn, info.resident, info.flags)
  for t, tile in G.TILES.items():
    assert rows[t][:2] == (tile.bm, tile.bn), t
    assert bool(rows[t][3] & L.TILE_BF16_ONLY) == tile.bf16_only, t
  with_flag = lambda f: {t for t, r in rows.items() if r[3] & f}
  assert with_flag(L.TILE_PERSISTENT) == set(G.PERSISTENT) and with_flag(L.TILE_HALO) == set(G.HALO)
  # resident workgroups per CU: what the LDS ring (stages x (bm + bn) x 128 bytes, + 2 halo patches) leaves of 160 KiB,
  # as the cost model counts them; GEGLU: the tiles whose width is a multiple of 64 and whose epilogue pairs value / gate
  assert [rows[t][2] for t in range(1, 20)] == [1, 2, 3, 5, 1, 2, 1, 1, 1, 2, 1, 2, 1, 1, 1, 1, 2, 2, 1]
  assert with_flag(L.TILE_GEGLU) == {1, 2, 5, 11, 12, 14, 19} and with_flag(L.TILE_GEGLU_VEC) == {11, 12}
  assert all(G.TILES[t].bn % 64 == 0 for t in with_flag(L.TILE_GEGLU))
  assert ops._TILE_DIMS == {t: r[:3] for t, r in rows.items() if t != 5}
  assert ops._BF16_TILES == tuple(t for t in range(1, 20) if G.TILES[t].bf16_only)
  assert set(ops._PERSISTENT_TILES) == set(G.PERSISTENT) and set(ops._HALO_RING_TILES) == set(G.HALO)
  # ring depths: gemm_kernel.h NSTAGE = NS, else 3 for the halo ring, else 3 where two stages already fill a CU's LDS for
  # one 8-wave workgroup and three still fit, else 2; the persistent kernel: 3 (gemm3_kernel.h)
  waves8 = {1, 7, 8, 9, 11}                                       # gemm_tiles.h: the 8-wave (wm x wn) forms
  for t, tile in G.TILES.items():
    stage = (tile.bm + tile.bn) * 128
    want = {17: 4, 18: 3, 19: 3}.get(t, 3 if t in G.PERSISTENT + G.HALO else
                                     3 if (4 * stage > 160 * 1024 >= 3 * stage and t in waves8) else 2)
    assert tile.stages == want, t


def test_matrix_coverage():
  for name, f in G.FORMS.items():
    cs, t, bke = BY_FORM[name], G.tile_of(f), G.bke_of(f)
    plain = [c for c in cs if c.kind == "plain"]
    conv = [c for c in cs if c.kind == "conv"]
    if f.tile in G.HALO:
      assert {(c.H, c.W) for c in conv} >= {(16, 16), (32, 16), (48, 16), (8, 32), (16, 32), (24, 32), (40, 32)}
      assert {c.B for c in conv} == {1, 3} and {c.Cin // 64 for c in conv} >= {1, 2, 3, 5}
      assert {G.expected_slabs(c) for c in conv} >= {1, 2, 3} and any(c.in_slice for c in conv)
      assert any(G.ktiles_of(c) % G.expected_slabs(c) for c in conv)                     # a short last slab
      assert all(c.M % 256 == 0 and c.N % t.bn == 0 for c in conv)
      continue
    assert set(G.m_values(t)) <= {c.M for c in plain}, name
    assert set(G.kt_values(t)) <= {G.ktiles_of(c) for c in plain}, name
    if f.tile in G.PERSISTENT:
      assert all(c.N % t.bn == 0 and c.odt == G.BF and c.alpha == 1.0 for c in cs)
      assert {c.split for c in cs if c.kind != "lint"} == {f.wg} and any(c.kind == "lint" for c in cs)
    else:
      assert set(G.n_values(t)) <= {c.N for c in plain}, name
      assert len({c.N for c in plain if c.N % 8}) >= 2 and any(c.off8 for c in plain)
      assert any(c.lda_x and c.ldc_x and c.ldr_x for c in plain)
      assert any(c.addend and t.bm % c.add_rows for c in plain)
      assert {c.alpha for c in plain} == {1.0, 0.5, 2.0}
      assert any(c.K2 and c.lda2_x for c in plain)
      bmm = {(c.shared_w, c.trans) for c in cs if c.kind == "bmm" and c.Bt == 3}
      assert bmm == {(0, 0), (0, 1), (1, 0), (1, 1)}, name
      assert any(c.odt != f.dt for c in cs)
    if f.tile and f.tile not in G.PERSISTENT:
      assert any(c.kind == "out2" for c in cs)
      for group in (plain, conv) if f.tile != 5 else (plain,):
        sk = [c for c in group if c.split > 1]
        kinds = {("even" if G.ktiles_of(c) % c.split == 0 else
                  "dropped" if G.expected_slabs(c) < c.split else "short") for c in sk}
        assert kinds == {"even", "dropped", "short"}, (name, kinds)
        assert any(c.defer for c in sk) and any(c.N % 8 or c.off8 for c in sk) or group is conv
      assert any(c.split > 1 and (c.N % 8 or c.off8) and c.bias and c.addend and c.res for c in plain)   # scalar reduce
    if f.tile == 5:
      continue
    geoms = {(c.H, c.W) for c in conv}
    assert geoms >= set(G.GEOMS), name
    assert {c.B for c in conv} == {1, 2, 3, 5} or {c.B for c in conv} >= {1, 3, 5}
    assert {c.Cin // bke for c in conv} >= {1, 2, 3, 5}
    s2, nlp, up = ([c for c in conv if c.stride == 2 and not c.nlp], [c for c in conv if c.nlp], [c for c in conv if c.up])
    for group in (s2, nlp):
      assert any(c.H % 2 == 0 and c.W % 2 == 0 for c in group) and any(c.H % 2 and c.W % 2 for c in group), name
    assert any((c.H, c.W) == (1, 1) for c in up) and any(c.H % 2 or c.W % 2 for c in up)
    assert any(c.in_slice for c in conv) and any(c.out_slice for c in conv)
    epis = {(c.bias, c.addend, c.res) for c in conv}
    assert epis >= {(1, 0, 0), (1, 1, 0), (1, 0, 1)} and ((1, 1, 1) in epis or f.tile in G.PERSISTENT)
    if f.tile not in G.PERSISTENT:
      assert {c.N for c in conv} >= {8, t.bn, t.bn + 8} and any(c.K2 and c.in_slice for c in conv)
    # probe 1 on every mode at the two smallest and the two most ragged geometries at least
    for mode in ({}, dict(stride=2, nlp=0), dict(nlp=1), dict(up=1)):
      sel = {(c.H, c.W) for c in conv if c.sel and all(getattr(c, k) == v for k, v in mode.items())
             and (mode or (c.stride == 1 and not c.up))}
      assert len(sel) >= 4, (name, mode, sel)
    assert sum(c.sel for c in plain) >= 4


def _lib():
  from ldm_tf2_amd import _lib
  return _lib


def _plan_params(c):
  """The host-query parameters of a case (what ops hands to ldm_gemm, without pointers)."""
  L = _lib()
  f = G.FORMS[c.form]
  p = L.GemmParams()
  p.M, p.N, p.K, p.batch = c.M, c.N, c.K, c.Bt
  p.dtype, p.out_dtype = (L.BF16 if f.dt == G.BF else L.F32), (L.BF16 if c.odt == G.BF else L.F32)
  p.tile, p.split_k, p.alpha = f.tile, c.split, c.alpha
  p.workspace, p.workspace_bytes = 1, 96 << 20
  if c.kind == "conv":
    _, _, oh, ow = G.conv_dims(c)
    p.conv, p.B, p.H, p.W, p.Cin, p.OH, p.OW = 1, c.B, c.H, c.W, c.Cin, oh, ow
    p.stride, p.upsample, p.no_lead_pad = c.stride, c.up, c.nlp
  if c.K2:
    p.a2, p.Cin2 = 1, c.K2
  return p


@pytest.mark.parametrize("name", list(G.FORMS))
def test_conditions_and_mutations(name):
  f = G.FORMS[name]
  lib = _lib().lib
  for c in BY_FORM[name]:
    cid = G.case_id(c)
    if c.kind in ("plain", "conv") and f.tile:
      p = _plan_params(c)
      t, s = C.c_int(), C.c_int()
      assert lib.ldm_gemm_plan(C.byref(p), C.byref(t), C.byref(s)) == 0 and t.value == f.tile, cid
      assert lib.ldm_gemm_splits(C.byref(p)) == G.expected_slabs(c), cid
    d = G.probe_census(c)
    ref = G.reference(c, d)
    cap = 256 if c.odt == G.BF else 2 ** 24 - 1
    assert float(ref.abs().max()) <= cap and G.representable(ref, c.odt), (cid, float(ref.abs().max()))
    assert G.partial_sum_bound(c, d) < 2 ** 24, cid
    assert G.alive_everywhere(c, d), cid
    dens = float((d["w"] != 0).double().mean())
    assert dens <= min(0.25, 360.0 / c.K) * 1.6 + 0.02, (cid, dens)
    for kind in G.MUTATIONS:
      if G.mutation_applies(c, kind):
        assert not torch.equal(G.reference(c, d, kind), ref), (cid, kind)
    if c.sel:
      cs = G.as_selection(c)
      ph = G.phases(cs)
      kt = G.ktile_of_col(cs)
      hit = set()
      for p_ in ph:
        hit |= set(kt[G.selected_column(cs, p_)].tolist())
      assert hit == set(range(G.ktiles_of(cs))) and 1 <= len(ph) <= G.MAX_PHASES, (cid, ph)
      d1 = G.probe_selection(cs, ph[0])
      r1 = G.reference(cs, d1)
      assert float(r1.abs().max()) <= 127 and G.partial_sum_bound(cs, d1) < 2 ** 24, cid


def test_position_code_separates_neighbours():
  p = torch.arange(0, 6000).view(-1, 1)
  ch = torch.arange(0, 640).view(1, -1)
  v = G.code(p, ch)
  assert int(v.abs().min()) >= 1 and int(v.abs().max()) <= 127
  widths = sorted({c.W for c in CASES if c.kind == "conv"})
  areas = sorted({c.H * c.W for c in CASES if c.kind == "conv"})
  deltas = {1} | set(widths) | {w + 1 for w in widths} | {abs(w - 1) for w in widths if w > 1}
  for dp in sorted(deltas | set(areas)):                             # +-1 pixel / row, +-1 line (and diagonals), +-1 image
    assert dp % 127 != 0, dp
    assert bool((v[dp:] != v[:-dp]).all()), dp
  for dc in (8, 32, 64):                                             # one 16-byte chunk, one K-tile
    assert bool((v[:, dc:] != v[:, :-dc]).all()), dc


def test_reference_against_the_oracle_once_per_mode():
  from oracle import ldm_oracle as O
  want = {"s1": None, "s2": None, "nlp": None, "up": None, "plain": None}
  for c in BY_FORM["t2-f32"]:
    mode = ("plain" if c.kind == "plain" and not c.K2 else "up" if c.up else "nlp" if c.nlp else
            "s2" if c.stride == 2 else "s1" if c.kind == "conv" and not c.K2 else None)
    if mode in want and want[mode] is None and c.M > 30 and not (c.kind == "conv" and c.H * c.W < 15):
      want[mode] = c
  assert all(v is not None for v in want.values()), want
  for mode, c in want.items():
    d = G.probe_census(c)
    ref = G.reference(c._replace(bias=0, addend=0, res=0, alpha=1.0), d)[0]
    w = d["w"][0].double()
    if mode == "plain":
      got = d["a"][0].double() @ w.t()
    else:
      x = d["a"].double()
      k = w.view(c.N, 3, 3, c.Cin).permute(1, 2, 3, 0).contiguous()                    # OHWI -> HWIO
      if c.up:
        x = O.upsample_nearest2x(x)
      if c.nlp:
        got = O.conv2d(x, k, None, stride=2, pad=((0, 1), (0, 1)))                     # pad [[0, 1], [0, 1]] + VALID
      else:
        got = O.conv2d(x, k, None, stride=c.stride)
      got = got.reshape(c.M, c.N)
    assert torch.equal(got.double(), ref), (mode, G.case_id(c))
