"""Device noise source on the GPU, all through the C ABI: the integer generator word for word
against tests/philox_ref.py, the normals against its float64 form, sharding, the fused entries against the table
entries fed ldm_normal_fill's tables, graph reuse across seeds, the launches of a step, the untouched default, and
whole loops against the oracle composition fed the restatement's noise.

Gates.  Normals: 4 x the worst error of the float32 NumPy restatement against the float64 one on the same words.
Fused against table: per element 2^-23 (|mean| + |noise sigma|), the same form for the blend and for q_sample (one
FMA-contraction choice); the numbers drawn are identical by construction.  Loops: the host-source loop's error
against the same oracle in the same run times 20/3 (the factor of tests/test_plms_gpu.py), and the project's loop
gates.  Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.
"""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import philox_ref as R  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
import test_plms_gpu as PL  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, HW, N, LDM = T.B, T.HW, T.N, T.LDM
NPS = HW * HW * 4
GS = 5.
SHAPE = [B, HW, HW, 4]
SEED = (1 << 32) + 7                  # both key words in use
EPS = 2.0 ** -23


def _rng(dev, seed, first):
  seed = int(seed) % (1 << 64)
  w = np.array([seed & 0xffffffff, seed >> 32, first, 0], dtype=np.uint32)
  return torch.from_numpy(w.view(np.int32).copy()).to(dev)


def _sampler(dev, dtype, unet_w, txt_w, kl_w, noise_source="device", eta=1., sampler="ddim", use_graph=True,
             temb_table=True, kwarg=True):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**T.UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=T.CTX_DIM)
  ae = AutoencoderKL(**T.KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**T.TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  kw = dict(noise_source=noise_source) if kwarg else {}
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, temb_table=temb_table,
                                     sampler=sampler, **kw, **dict(LDM, eta=eta))


# ---- 1. the integer part, exact ---------------------------------------------------------------------------
def _device_words(dev, seed, first, stream, b, n):
  out = torch.zeros(b, n, dtype=torch.int32, device=dev)
  ops.philox_u32(out, _rng(dev, seed, first), stream)
  return out.cpu().numpy().view(np.uint32)


def test_philox_words_known_answer(dev):
  w = _device_words(dev, 0, 0, 0, 1, 16)
  assert [hex(int(x)) for x in w[0, :4]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
  # the third published vector's key and first three counter words (the layout fixes the fourth at 0)
  seed = (0x299f31d0 << 32) | 0xa4093822
  w = _device_words(dev, seed, 0x85a308d3 - 1, 0x13198a2e, 2, 4 * (0x10 + 1))
  assert np.array_equal(w, R.words(seed, 0x85a308d3 - 1, 0x13198a2e, 2, 4 * (0x10 + 1)))


@pytest.mark.parametrize("n", [16, 4096, 16384])
def test_philox_words_equal_the_restatement(dev, n):
  g = np.random.default_rng(n)
  cases = [(0, 0, 0), (1 << 32, 0, 1), ((1 << 64) - 1, (1 << 32) - 2, (1 << 32) - 1)]
  for _ in range(4):
    cases.append((int(g.integers(0, 1 << 63)) * 2 + 1, int(g.integers(0, 1 << 32)), int(g.integers(0, 1 << 32))))
  cases += [(SEED, 3, R.ETA_STREAM + 9), (SEED, 3, R.Q_STREAM + 9), (SEED + (1 << 64), 3, R.ENCODE_STREAM)]
  for seed, first, stream in cases:
    got = _device_words(dev, seed, first, stream, 3, n)
    assert np.array_equal(got, R.words(seed, first, stream, 3, n)), (hex(seed), first, stream)


def test_rejects_what_it_cannot_vectorise(dev):
  from ldm_tf2_amd._lib import LdmHipError
  rng = _rng(dev, 0, 0)
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.normal_fill(torch.zeros(2, 3, 3, 3, device=dev), rng, 0)
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.philox_u32(torch.zeros(2, 27, dtype=torch.int32, device=dev), rng, 0)
  with pytest.raises(LdmHipError, match="aligned"):
    ops.normal_fill(torch.zeros(2 * 16 + 1, device=dev)[1:].view(2, 16), rng, 0)
  i = torch.zeros(1, dtype=torch.int32, device=dev)
  x = torch.zeros(2, 3, 3, 3, device=dev)
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.cfg_ddim_update_rng(torch.zeros(4, 3, 3, 3, device=dev), x, x.clone(), torch.zeros(10, 4, device=dev), i, rng, GS)


# ---- 2. the normals -------------------------------------------------------------------------------------
def test_normals_against_float64_restatement(dev):
  b, n = 16, 1 << 16                                     # 2^20 normals
  out = torch.empty(b, n, device=dev)
  xu = torch.empty(2 * b, n, device=dev, dtype=torch.bfloat16)
  ops.normal_fill(out, _rng(dev, 1234, 0), 7, x_unet_out=xu)
  got = out.cpu().numpy()
  w = R.words(1234, 0, 7, b, n)
  z64 = R.normals_from_words(w, np.float64)
  z32 = R.normals_from_words(w, np.float32)
  base = float(np.abs(z32.astype(np.float64) - z64).max())
  err = float(np.abs(got.astype(np.float64) - z64).max())
  print(f"normals: device max |err| {err:.3e}; float32 NumPy restatement {base:.3e}; gate {4 * base:.3e}")
  assert np.isfinite(got).all()
  assert err <= 4 * base, (err, base)
  R.check_moments(got, "device normals")
  bound = R.moment_bounds(n)[4]
  assert abs(float(np.corrcoef(got[0], got[1])[0, 1])) < bound
  assert abs(float(np.corrcoef(got[0, :-1], got[0, 1:])[0, 1])) < bound
  assert torch.equal(xu[:b].cpu(), out.cpu().to(torch.bfloat16)) and torch.equal(xu[b:], xu[:b])
  xf = torch.empty(2 * b, n, device=dev)
  again = torch.empty_like(out)
  ops.normal_fill(again, _rng(dev, 1234, 0), 7, x_unet_out=xf)
  assert torch.equal(again, out) and torch.equal(xf[:b], out) and torch.equal(xf[b:], out)


# ---- 3. sharding -------------------------------------------------------------------------------------------
def test_normal_fill_is_independent_of_sharding(dev):
  whole = torch.empty(4, HW, HW, 4, device=dev)
  ops.normal_fill(whole, _rng(dev, SEED, 0), R.Q_STREAM + 3)
  for first in (0, 2):
    part = torch.empty(2, HW, HW, 4, device=dev)
    ops.normal_fill(part, _rng(dev, SEED, first), R.Q_STREAM + 3)
    assert torch.equal(part, whole[first:first + 2])
  assert not torch.equal(whole[:2], whole[2:])


def _ids(b):
  one = T._ids()
  return np.concatenate([np.tile(one[:1], (b, 1)), np.tile(one[-1:], (b, 1))], 0)


def test_txt2img_loop_is_independent_of_sharding(dev, unet_w, txt_w, kl_w):
  """x_T and the eta noise of every step drawn on the device: B = 4 at 0 against two B = 2 runs at 0 and 2."""
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  s.ddim_p_sample_loop(_ids(4), [4, HW, HW, 4], GS, seed=SEED, first_sample_index=0)
  whole = s._xt.cpu().clone()
  for first in (0, 2):
    s.ddim_p_sample_loop(_ids(2), [2, HW, HW, 4], GS, seed=SEED, first_sample_index=first)
    assert torch.equal(s._xt.cpu(), whole[first:first + 2]), first
  assert not torch.equal(whole[:2], whole[2:])


def test_inpainting_loop_is_independent_of_sharding(dev, unet_w, txt_w, kl_w):
  """The whole loop, the encoder included: with the device source every image is encoded in a pass of its own
  (the launch plans of an encoder pass depend on its batch, so one pass over B images gives an image other bits
  at B = 4 than at B = 2), and every number drawn is keyed by the global sample index."""
  g = np.random.default_rng(33)
  img = (g.random((4, 8 * HW, 8 * HW, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
  mask = T._inputs(0.)[4][0]
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  s.ddim_p_sample_loop_img2img(_ids(4), img, GS, strength=0.8, mask=mask, seed=SEED, first_sample_index=0)
  whole = s._xt.cpu().clone()
  for first in (0, 2):
    s.ddim_p_sample_loop_img2img(_ids(2), img[first:first + 2], GS, strength=0.8, mask=mask, seed=SEED,
                                 first_sample_index=first)
    part = s._xt.cpu()
    r = PL.rel64(part, whole[first:first + 2].double().numpy())
    print(f"samples {first}..{first + 1}: B=2 run against its rows of the B=4 run: rel {r:.3e}")
    assert torch.equal(part, whole[first:first + 2]), (first, r)
  assert not torch.equal(whole[:2], whole[2:])


# ---- 4. the fused entries against the table entries -----------------------------------------------------------
def _fused_inputs(dev, eta):
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  m = LatentDiffusionModel(None, None, None, **dict(LDM, eta=eta))
  m.device = dev
  g = torch.Generator().manual_seed(4)
  t = dict(eps_all=torch.randn(2 * B, HW, HW, 4, generator=g), xt=torch.randn(B, HW, HW, 4, generator=g),
           ring=torch.randn(4, B, HW, HW, 4, generator=g), z0=torch.randn(B, HW, HW, 4, generator=g),
           mask=torch.rand(B, HW, HW, generator=g))
  t["mask"][:, 0, :] = 1.
  t["mask"][:, 1, :] = 0.
  t = {k: v.to(dev).contiguous() for k, v in t.items()}
  rng = _rng(dev, SEED, 5)
  noise = torch.empty(N, B, HW, HW, 4, device=dev)
  qfull = torch.full((N + 1, B, HW, HW, 4), float("nan"), device=dev)     # row 0 = index -1: never read
  for i in range(N):
    ops.normal_fill(noise[i], rng, R.ETA_STREAM + i)
    ops.normal_fill(qfull[i + 1], rng, R.Q_STREAM + i)
  assert np.array_equal(noise[3].cpu().numpy(), ops.normal_fill(torch.empty(B, NPS, device=dev), rng,
                                                                R.ETA_STREAM + 3).cpu().numpy().reshape(B, HW, HW, 4))
  return m, t, rng, noise, qfull[1:]


def _gate(m, t, idx, noise_row, q_row, masked, ep=None):
  """Per-element 2^-23 (|mean| + |noise sigma|), then the same form through the blend; float64 on the inputs."""
  d = lambda a: a.double().cpu().numpy()
  coef = m._coef_dev.double().cpu().numpy()[idx]
  c1, c2, a_prev, sigma = coef
  if ep is None:
    eu, ec = d(t["eps_all"][:B]), d(t["eps_all"][B:])
    ep = eu + GS * (ec - eu)
    sb = np.sqrt(1 - a_prev - sigma * sigma)
  else:
    sigma, sb = 0., np.sqrt(1 - a_prev)
  x0 = c1 * d(t["xt"]) - c2 * ep
  mean = np.sqrt(a_prev) * x0 + sb * ep
  nz = d(noise_row) * sigma if sigma else 0. * mean
  gate = EPS * (np.abs(mean) + np.abs(nz))
  o = mean + nz
  if masked and idx >= 1:
    qa, qb = m._device_q_tables()[2].double().cpu().numpy()[idx - 1]
    ta, tb = qa * d(t["z0"]), qb * d(q_row)
    mk = d(t["mask"])[..., None]
    gate = mk * EPS * (np.abs(ta) + np.abs(tb)) + (1 - mk) * gate + EPS * (np.abs(mk * (ta + tb)) + np.abs((1 - mk) * o))
  return gate


def _within(what, got, want, gate, equal):
  diff = np.abs(got.double().cpu().numpy() - want.double().cpu().numpy())
  bits = torch.equal(got, want)
  equal.append(bits)
  worst = float((diff / np.maximum(gate, 1e-300)).max())
  print(f"{what}: bit-equal {bits}; max |diff| {diff.max():.3e}, worst diff / gate {worst:.3f}")
  assert bool(torch.isfinite(got).all()) and (diff <= gate).all(), (what, float(diff.max()))


@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("eta", [0., 1.], ids=["sigma0", "sigma"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_fused_ddim_against_table_entry(dev, masked, eta, x_dtype):
  m, t, rng, noise, Q = _fused_inputs(dev, eta)
  equal = []
  for idx in (N - 1, 5, 1, 0):
    res = {}
    for fused in (False, True):
      out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
      xu = torch.empty(2 * B, HW, HW, 4, device=dev, dtype=x_dtype)
      index = torch.tensor([idx], dtype=torch.int32, device=dev)
      kw = dict(x_unet_out=xu, pred_x0_out=px, dec_index=bool(idx & 1))
      if fused:
        bl = dict(z0=t["z0"], mask=t["mask"], q_coef=m._device_q_tables()[2]) if masked else {}
        ops.cfg_ddim_update_rng(t["eps_all"], t["xt"], out, m._coef_dev, index, rng, GS, **bl, **kw)
      elif masked:
        ops.cfg_ddim_update_masked(t["eps_all"], t["xt"], out, m._coef_dev, index, GS, t["z0"], t["mask"], Q,
                                   m._device_q_tables()[2], noise=noise, noise_index_stride=noise[0].numel(),
                                   q_index_stride=Q[0].numel(), **kw)
      else:
        ops.cfg_ddim_update(t["eps_all"], t["xt"], out, m._coef_dev, index, GS, noise=noise,
                            noise_index_stride=noise[0].numel(), **kw)
      assert index.item() == (idx - 1 if idx & 1 else idx)
      assert torch.equal(xu[:B], out.to(x_dtype)) and torch.equal(xu[B:], out.to(x_dtype))
      res[fused] = (out, px)
    gate = _gate(m, t, idx, noise[idx], Q[idx - 1] if idx else None, masked)
    _within(f"ddim idx={idx} masked={masked} eta={eta}", res[True][0], res[False][0], gate, equal)
    assert torch.equal(res[True][1], res[False][1])                 # pred_x0: no noise in it
  print(f"bit equality at all four indices: {all(equal)}")


@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fused_plms_against_table_entry(dev, x_dtype):
  m, t, rng, _, Q = _fused_inputs(dev, 0.)
  equal = []
  for idx in (N - 1, 5, 1, 0):
    for masked in (True, False):
      res = {}
      start = min(idx + 3, N - 1)
      for fused in (False, True):
        out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
        xu = torch.empty(2 * B, HW, HW, 4, device=dev, dtype=x_dtype)
        ring = t["ring"].clone()
        index = torch.tensor([idx], dtype=torch.int32, device=dev)
        st = torch.tensor([start], dtype=torch.int32, device=dev)
        kw = dict(x_unet_out=xu, pred_x0_out=px, dec_index=bool(idx & 1))
        if masked:
          kw.update(z0=t["z0"], mask=t["mask"], q_coef=m._device_q_tables()[2])
        if fused:
          ops.cfg_plms_update_rng(t["eps_all"], t["xt"], out, ring, m._coef_dev, index, st, rng, GS, **kw)
        else:
          if masked:
            kw.update(q_noise=Q, q_index_stride=Q[0].numel())
          ops.cfg_plms_update(t["eps_all"], t["xt"], out, ring, m._coef_dev, index, st, GS, **kw)
        assert torch.equal(xu[:B], out.to(x_dtype)) and torch.equal(xu[B:], out.to(x_dtype))
        res[fused] = (out, px, ring)
      # e' of the step in float64 from the ring the kernels read
      d = lambda a: a.double().cpu().numpy()
      e_i = d(t["eps_all"][:B]) + GS * (d(t["eps_all"][B:]) - d(t["eps_all"][:B]))
      j = start - idx
      hist = [e_i] + [d(t["ring"][(idx + k) & 3]) for k in range(1, j + 1)]
      ep = sum(w * e for w, e in zip(PL.P.WEIGHTS[j], hist))
      gate = _gate(m, t, idx, None, Q[idx - 1] if idx else None, masked, ep=ep)
      _within(f"plms idx={idx} j={j} masked={masked}", res[True][0], res[False][0], gate, equal)
      assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
      if not masked:
        assert torch.equal(res[True][0], res[False][0])             # nothing is drawn: the same arithmetic
  print(f"bit equality in all cases: {all(equal)}")


@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fused_q_sample_against_table_entry(dev, x_dtype):
  m, t, rng, _, Q = _fused_inputs(dev, 0.)
  sa, sb, _ = m._device_q_tables()
  equal = []
  for k in (N, 6, 2, 1):
    tt = torch.full((B,), int(m._ddim_steps[k - 1]), dtype=torch.int32, device=dev)
    res = {}
    for fused in (False, True):
      out = torch.empty(B, HW, HW, 4, device=dev)
      xu = torch.empty(2 * B, HW, HW, 4, device=dev, dtype=x_dtype)
      if fused:
        ops.q_sample_rng(t["z0"], rng, R.Q_STREAM + k - 1, tt, sa, sb, out, x_unet_out=xu)
      else:
        ops.q_sample(t["z0"], Q[k - 1], tt, sa, sb, out, x_unet_out=xu)
      assert torch.equal(xu[:B], out.to(x_dtype)) and torch.equal(xu[B:], out.to(x_dtype))
      res[fused] = out
    a, b_ = float(sa[int(m._ddim_steps[k - 1])]), float(sb[int(m._ddim_steps[k - 1])])
    gate = EPS * (np.abs(a * t["z0"].double().cpu().numpy()) + np.abs(b_ * Q[k - 1].double().cpu().numpy()))
    _within(f"q_sample k={k}", res[True], res[False], gate, equal)
  print(f"bit equality at all four indices: {all(equal)}")


# ---- 5. one graph for every seed --------------------------------------------------------------------------------
def test_one_graph_serves_every_seed(dev, unet_w, txt_w, kl_w):
  img, _, _, _, mask = T._inputs(0.)
  ids = T._ids()
  run = lambda s, seed: s.ddim_p_sample_loop_img2img(ids, img, GS, strength=0.8, mask=mask, seed=seed,
                                                     first_sample_index=3).clone()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  graph, got = None, {}
  for seed in (11, SEED, 11 + (1 << 40)):
    got[seed] = run(s, seed)
    assert s._graph is not None and (graph is None or s._graph is graph)
    graph = s._graph
    assert "device" in s._graph_key and seed not in s._graph_key
  assert not torch.equal(got[11], got[SEED]) and not torch.equal(got[11], got[11 + (1 << 40)])
  for seed, want in got.items():
    assert torch.equal(run(_sampler(dev, torch.float32, unet_w, txt_w, kl_w), seed), want)       # a fresh graph
    eager = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
    assert torch.equal(run(eager, seed), want) and eager._graph is None                           # no graph
  # txt2img on the same sampler: another graph key, x_T drawn on the device, and again one graph per key
  a = s.ddim_p_sample_loop(ids, SHAPE, GS, seed=5).clone()
  g2 = s._graph
  b_ = s.ddim_p_sample_loop(ids, SHAPE, GS, seed=6).clone()
  assert s._graph is g2 and g2 is not graph and not torch.equal(a, b_)
  assert torch.equal(_sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False).ddim_p_sample_loop(
      ids, SHAPE, GS, seed=6), b_)


# ---- 6. no tables, the same launches --------------------------------------------------------------------------
@pytest.mark.parametrize("temb_table", [True, False])
def test_no_tables_and_the_host_steps_launches(dev, unet_w, txt_w, kl_w, monkeypatch, temb_table):
  img, E, Q, noises, mask = T._inputs(1.)
  calls = {}
  for sampler, eta in (("ddim", 1.), ("plms", 0.)):
    for source in ("host", "device"):
      s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, noise_source=source, eta=eta, sampler=sampler,
                   use_graph=False, temb_table=temb_table)
      s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=0.5, mask=mask, seed=3, record=[])
      tables = [hasattr(s, "_noise_buf"), hasattr(s, "_q_buf")]
      assert tables == ([eta != 0., True] if source == "host" else [False, False]), (sampler, source, tables)
      for masked in (False, True):
        s._index_dev.fill_(s._loop_start_index(4))
        s._set_loop_start(3)
        proxy = T._CountingLib(ops.lib)
        monkeypatch.setattr(ops, "lib", proxy)
        s._step(GS, False, getattr(s, "_noise_buf", None), dec_index=True, masked=masked, rng=source == "device")
        monkeypatch.setattr(ops, "lib", proxy._lib)
        torch.cuda.synchronize()
        calls[sampler, source, masked] = proxy.calls
  for sampler in ("ddim", "plms"):
    for masked in (False, True):
      host_entry = ("ldm_cfg_plms_update" if sampler == "plms" else
                    "ldm_cfg_ddim_update_masked" if masked else "ldm_cfg_ddim_update")
      rng_entry = f"ldm_cfg_{sampler}_update_rng"
      host, device = calls[sampler, "host", masked], calls[sampler, "device", masked]
      assert host.count(host_entry) == 1 and device.count(rng_entry) == 1
      assert [rng_entry if c == host_entry else c for c in host] == device and len(device) > 1
      assert not any(c in ("ldm_normal_fill", "ldm_philox_u32", "ldm_q_sample", "ldm_q_sample_rng") for c in device)
  print({k: len(v) for k, v in calls.items()})


def test_given_tables_run_the_table_entries_with_the_fused_numbers(dev, unet_w, txt_w, kl_w):
  """`noises=` (or `q_noises=`) wins and the step runs the table entry; the table the caller did not give is filled
  on the device with the streams of the fused path, so giving the fused path's own eta noise changes nothing."""
  img, _, _, _, mask = T._inputs(0.)
  ids = T._ids()
  kw = dict(strength=0.8, mask=mask, seed=SEED, first_sample_index=2)
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  fused = s.ddim_p_sample_loop_img2img(ids, img, GS, **kw).clone()
  assert not hasattr(s, "_q_buf") and not hasattr(s, "_noise_buf")
  rng = _rng(dev, SEED, 2)
  eta_tab = torch.stack([ops.normal_fill(torch.empty(B, HW, HW, 4, device=dev), rng, R.ETA_STREAM + i) for i in range(N)])
  q_tab = torch.stack([ops.normal_fill(torch.empty(B, HW, HW, 4, device=dev), rng, R.Q_STREAM + i) for i in range(N)])
  a = s.ddim_p_sample_loop_img2img(ids, img, GS, noises=eta_tab, **kw).clone()
  assert hasattr(s, "_q_buf") and torch.equal(s._q_buf[:8], q_tab[:8])
  b_ = s.ddim_p_sample_loop_img2img(ids, img, GS, q_noises=q_tab, **kw).clone()
  assert torch.equal(s._noise_buf, eta_tab)
  r = [T.rel_err(x, fused.cpu())[0] for x in (a, b_)]
  print(f"table entries with the fused path's numbers against the fused loop: rel {r[0]:.3e}, {r[1]:.3e}; "
        f"bit-equal {torch.equal(a, fused)}, {torch.equal(b_, fused)}")
  assert torch.equal(a, b_) and max(r) < 1e-5
  other = s.ddim_p_sample_loop_img2img(ids, img, GS, noises=eta_tab.flip(0), **kw)
  assert T.rel_err(other, fused.cpu())[0] > 1e-3
  # an explicit x_T / encode_noise wins for that one input
  x_T = np.random.default_rng(9).standard_normal((B, HW, HW, 4)).astype(np.float32)
  assert not torch.equal(s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T, seed=SEED).clone(),
                         s.ddim_p_sample_loop(ids, SHAPE, GS, seed=SEED))
  e = ops.normal_fill(torch.empty(B, HW, HW, 4, device=dev), _rng(dev, SEED, 2), R.ENCODE_STREAM)
  assert torch.equal(s.get_latents(img, seed=SEED, first_sample_index=2), s.get_latents(img, noise=e))


# ---- 7. the default is untouched --------------------------------------------------------------------------------
def test_host_source_is_the_default(dev, unet_w, txt_w, kl_w):
  img, _, _, _, mask = T._inputs(0.)
  ids = T._ids()
  out = {}
  for kwarg in (False, True):
    s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, noise_source="host", kwarg=kwarg)
    assert s._noise_source == "host"
    out[kwarg] = (s.ddim_p_sample_loop(ids, SHAPE, GS, seed=4).clone(),
                  s.ddim_p_sample_loop_img2img(ids, img, GS, strength=0.8, mask=mask, seed=4).clone())
    assert s._rng is None and hasattr(s, "_noise_buf") and hasattr(s, "_q_buf")
  assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])
  dev_s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  assert not torch.equal(dev_s.ddim_p_sample_loop(ids, SHAPE, GS, seed=4), out[True][0])   # other numbers, by design


# ---- 8. whole loops against the oracle fed the restatement's noise ----------------------------------------------
_CACHE = {}


def _noise(stream, first=0):
  return R.normals(SEED, first, stream, B, NPS).astype(np.float32).reshape(B, HW, HW, 4)


def _tables():
  if "tables" not in _CACHE:
    _CACHE["tables"] = dict(x_T=_noise(R.XT_STREAM), E=_noise(R.ENCODE_STREAM),
                            eta=np.stack([_noise(R.ETA_STREAM + i) for i in range(N)]),
                            Q=np.stack([_noise(R.Q_STREAM + i) for i in range(N)]))
  return _CACHE["tables"]


def _oracle(kind, w):
  """kind: "txt2img" (eta 1, with the progressive frames), ("img2img", k), ("inpaint", k), ("plms", k)."""
  if kind in _CACHE:
    return _CACHE[kind]
  tb, ids = _tables(), T._ids()
  img, _, _, _, mask = T._inputs(0.)
  if kind == "txt2img":
    out = O.ddim_p_sample_loop_progressive(ids, tb["x_T"], w, dict(LDM, eta=1.), guidance_scale=GS, record_freq=5,
                                           noises=tb["eta"])
  elif kind[0] == "plms":
    sched = O.make_schedule(LDM["num_steps"], LDM["beta_start"], LDM["beta_end"], 0., N)
    context = O.text_encoder(ids, w["cond_stage_model"], torch.float32)
    _, _, sample = O.diagonal_gaussian(O.encoder_forward(torch.from_numpy(img), w["autoencoder"]), tb["E"])
    z0 = np.float32(LDM["scale_factor"]) * sample
    k = kind[1]
    x = T.q_sample_ref(sched["alphas_cumprod"], z0, [sched["ddim_steps"][k - 1]] * B, tb["Q"][k - 1])
    rec = PL._oracle_plms(context, w["unet"], sched, x, k - 1, (mask, z0, tb["Q"]))
    out = (O.decoder_forward(rec[-1][0] / LDM["scale_factor"], w["autoencoder"]), rec[-1][0])
  else:
    saved = dict(T._ORACLE)                              # (its cache is keyed without the noise: keep it as it was)
    T._ORACLE.clear()
    images, _, rec = T.oracle_img2img(ids, img, w, dict(LDM, eta=1.), kind[1], tb["E"], tb["Q"], tb["eta"],
                                      mask if kind[0] == "inpaint" else None, gs=GS)
    T._ORACLE.clear()
    T._ORACLE.update(saved)
    out = (images, rec[-1])
  _CACHE[kind] = out
  return out


def _loop_check(what, dtype, device_got, host_got, ref):
  r, base = T.rel_err(device_got, ref)[0], T.rel_err(host_got, ref)[0]
  print(f"{what} [{dtype}]: device source {r:.3e}; host source on the same numbers {base:.3e}; "
        f"gate {base * 20 / 3:.3e}; the project's loop gate {T.LOOP_REL[dtype]:.1e}")
  assert r <= base * 20. / 3. and r < T.LOOP_REL[dtype], (what, r, base)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_txt2img_and_progressive_loops_against_oracle(dev, dtype, unet_w, txt_w, kl_w):
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  tb, ids = _tables(), T._ids()
  ref_img, ref_sp, ref_xp = _oracle("txt2img", w)
  host = _sampler(dev, dtype, unet_w, txt_w, kl_w, noise_source="host")
  h_img, h_sp, h_xp = host.ddim_p_sample_loop_progressive(ids, SHAPE, GS, record_freq=5, x_T=tb["x_T"], noises=tb["eta"])
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  got = s.ddim_p_sample_loop(ids, SHAPE, GS, seed=SEED).clone()
  assert not hasattr(s, "_noise_buf")
  _loop_check("txt2img eta=1 images", dtype, got, h_img, ref_img)
  d_img, d_sp, d_xp = s.ddim_p_sample_loop_progressive(ids, SHAPE, GS, record_freq=5, seed=SEED)
  assert torch.equal(d_img, got) and not hasattr(s, "_noise_buf")
  _loop_check("progressive samples", dtype, d_sp, h_sp, ref_sp)
  _loop_check("progressive pred_x0", dtype, d_xp, h_xp, ref_xp)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", [("img2img", 5), ("inpaint", 8), ("plms", 8)], ids=lambda k: k[0])
def test_img2img_loops_against_oracle(dev, dtype, kind, unet_w, txt_w, kl_w):
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  tb, ids = _tables(), T._ids()
  img, _, _, _, mask = T._inputs(0.)
  ref_img, ref_lat = _oracle(kind, w)
  cfg = dict(eta=0., sampler="plms") if kind[0] == "plms" else dict(eta=1.)
  kw = dict(strength=kind[1] / N, mask=None if kind[0] == "img2img" else mask)
  host = _sampler(dev, dtype, unet_w, txt_w, kl_w, noise_source="host", **cfg)
  h_img = host.ddim_p_sample_loop_img2img(ids, img, GS, encode_noise=tb["E"], q_noises=tb["Q"],
                                          noises=None if kind[0] == "plms" else tb["eta"], **kw)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w, **cfg)
  d_img = s.ddim_p_sample_loop_img2img(ids, img, GS, seed=SEED, **kw)
  assert not hasattr(s, "_noise_buf") and not hasattr(s, "_q_buf")
  _loop_check(f"{kind[0]} k={kind[1]} latents", dtype, s._xt, host._xt, ref_lat)
  _loop_check(f"{kind[0]} k={kind[1]} images", dtype, d_img, h_img, ref_img)


# ---- 9. CLI ---------------------------------------------------------------------------------------------------
def test_cli_noise_source_key(dev, tmp_path):
  from ldm_tf2_amd import run_ldm_sampler as RL
  from ldm_tf2_amd.tokenizer import get_token_ids
  unet = dict(model_channels=64, out_channels=4, num_blocks=2, attention_resolutions=[4, 2, 1], dropout_rate=0.1,
              channel_mult=[1, 2, 4, 4], num_heads=8)
  txt = dict(vocab_size=200, encoder_stack_size=2, hidden_size=128, num_heads=4, size_per_head=32,
             max_seq_len=77, filter_size=256, dropout_rate=0.1)
  kl = dict(latent_channels=4, channels=64, num_blocks=2, attention_resolutions=[], dropout_rate=0.,
            multipliers=[1, 2, 4, 4], resample_with_conv=True)
  prompt = "a painting of a virus monster playing guitar"
  words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "painting", "of", "virus", "monster", "play", "##ing",
           "guitar", "the", ","]
  words += [f"tok{i}" for i in range(200 - len(words))]
  (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n", encoding="utf-8")
  cfg = {
      "ldm_sampling": {"autoencoder_type": "kl", "latent_shape": [2, 16, 16, 4], "guidance_scale": 5.0,
                       "text_prompt": prompt, "vocab_dir": str(tmp_path), "sample_save_progress": False},
      "pre_ckpt_paths": {"cond_stage_model": None, "unet": None, "autoencoder": None},
      "cond_stage_model": txt, "autoencoder_kl": kl, "unet": unet, "ldm": dict(LDM, eta=1.),
  }
  path = tmp_path / "config.yaml"
  out = {}
  for name in ("device", "host"):
    cfg["ldm_sampling"]["noise_source"] = name
    path.write_text(yaml.safe_dump(cfg))
    RL.main(["--config_path", str(path), "--dtype", "f32", "--seed", "7", "--out", str(tmp_path / f"{name}.npy")])
    out[name] = np.load(tmp_path / f"{name}.npy")
    assert out[name].dtype == np.uint8 and out[name].shape == (2, 128, 128, 3)
  cfg["ldm_sampling"]["noise_source"] = "device"
  s = RL.build_from_config(cfg, dtype=torch.float32, verbose=False)
  assert s._noise_source == "device"
  ids = get_token_ids(prompt, 2, str(tmp_path), 77)
  images = s.ddim_p_sample_loop(ids, [2, 16, 16, 4], 5.0, seed=7)
  assert np.array_equal(out["device"], RL.tensor_to_image(images))
  assert not np.array_equal(out["device"], out["host"])
