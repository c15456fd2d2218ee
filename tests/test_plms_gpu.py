"""PLMS sampler on the GPU, all through the C ABI: the fused update kernel against the
float64 restatement (tests/plms_ref.py), the slots it must not read, the ring under graph replay and across loops,
whole loops against the oracle composition, the launch count, the untouched DDIM path and the CLI key.

Gates.  Kernel: the error of the existing ldm_cfg_ddim_update(_masked) against the same restatement on the same
inputs at sigma = 0, floored at 2^-23 relative, times 2 * sum_k |w_jk| (1, 2, 11/3, 20/3 for j = 0..3: what the
weights do to a rounding error in eps; 2 for rounding order).  Loops: the DDIM loop's error against
O.ddim_p_sample_loop on the same weights, x_T and dtype, measured in the same run, times 20/3.
Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.
"""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import plms_ref as P  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, HW, N, LDM = T.B, T.HW, T.N, T.LDM
GS = 5.
SHAPE = [B, HW, HW, 4]
FLOOR = 2.0 ** -23


def _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="plms", use_graph=True, temb_table=True):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**T.UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=T.CTX_DIM)
  ae = AutoencoderKL(**T.KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**T.TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, temb_table=temb_table,
                                     sampler=sampler, **LDM)


def _x_T():
  return np.random.default_rng(9).standard_normal((B, HW, HW, 4)).astype(np.float32)


def rel64(got, ref):
  got = np.asarray(got.detach().float().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
  return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


# ---- 1. the kernel against the float64 restatement ------------------------------------------------------
def _kernel_inputs(dev):
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  m = LatentDiffusionModel(None, None, None, **LDM)
  g = torch.Generator().manual_seed(4)
  t = dict(eps_all=torch.randn(2 * B, HW, HW, 4, generator=g), xt=torch.randn(B, HW, HW, 4, generator=g),
           ring=torch.randn(4, B, HW, HW, 4, generator=g), z0=torch.randn(B, HW, HW, 4, generator=g),
           Q=torch.randn(N, B, HW, HW, 4, generator=g), mask=torch.rand(B, HW, HW, generator=g))
  t["mask"][:, 0, :] = 1.
  t["mask"][:, 1, :] = 0.
  # the tables as the device sees them: cast to float32 first (`_extract`), widened for the restatement
  f = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
  tab = dict(c1=f(m._ddim_sqrt_recip_alphas_cumprod), c2=f(m._ddim_sqrt_recipm1_alphas_cumprod),
             a_prev=f(m._ddim_alphas_cumprod_prev), qa=f(m._sqrt_alphas_cumprod)[m._ddim_steps],
             qb=f(m._sqrt_one_minus_alphas_cumprod)[m._ddim_steps])
  return m, t, tab


def _restated(t, tab, idx, j, masked):
  """(x', x0, e_i) of the specification in float64 on the float32 inputs."""
  d = lambda a: a.double().numpy()
  eu, ec = d(t["eps_all"][:B]), d(t["eps_all"][B:])
  e_i = eu + GS * (ec - eu)
  hist = [e_i] + [d(t["ring"][(idx + k) & 3]) for k in range(1, j + 1)]
  x, x0 = P.plms_update(d(t["xt"]), hist, idx, j, tab["c1"], tab["c2"], tab["a_prev"])
  if masked and idx >= 1:
    q = tab["qa"][idx - 1] * d(t["z0"]) + tab["qb"][idx - 1] * d(t["Q"][idx - 1])
    mk = d(t["mask"])[..., None]
    x = mk * q + (1 - mk) * x
  return x, x0, e_i


def _run_plms(dev, m, t, idx, start, masked, x_dtype, dec, ring=None):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
  xu = torch.empty(2 * B, HW, HW, 4, device=dev, dtype=x_dtype)
  ring = d(t["ring"] if ring is None else ring)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  st = torch.tensor([start], dtype=torch.int32, device=dev)
  kw = {}
  if masked:
    kw = dict(z0=d(t["z0"]), mask=d(t["mask"]), q_noise=d(t["Q"]), q_coef=m._device_q_tables()[2],
              q_index_stride=t["Q"][0].numel())
  ops.cfg_plms_update(d(t["eps_all"]), d(t["xt"]), out, ring, m._coef_dev, index, st, GS, x_unet_out=xu,
                      dec_index=dec, pred_x0_out=px, **kw)
  assert index.item() == (idx - 1 if dec else idx) and st.item() == start
  return out.cpu(), px.cpu(), xu.cpu(), ring.cpu()


def _run_ddim(dev, m, t, idx, masked):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  if masked:
    ops.cfg_ddim_update_masked(d(t["eps_all"]), d(t["xt"]), out, m._coef_dev, index, GS, d(t["z0"]), d(t["mask"]),
                               d(t["Q"]), m._device_q_tables()[2], q_index_stride=t["Q"][0].numel(), pred_x0_out=px)
  else:
    ops.cfg_ddim_update(d(t["eps_all"]), d(t["xt"]), out, m._coef_dev, index, GS, pred_x0_out=px)
  return out.cpu(), px.cpu()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_kernel_against_float64_restatement(dev, x_dtype, masked):
  m, t, tab = _kernel_inputs(dev)
  worst = {}
  for idx in (N - 1, 5, 1, 0):
    want_d, want_d0, _ = _restated(t, tab, idx, 0, masked)          # sigma = 0 DDIM == order 0
    dd, dd0 = _run_ddim(dev, m, t, idx, masked)
    base, base0 = max(rel64(dd, want_d), FLOOR), max(rel64(dd0, want_d0), FLOOR)
    for j in range(4):
      want, want0, e_i = _restated(t, tab, idx, j, masked)
      dec = bool((idx + j) & 1)
      got, px, xu, ring = _run_plms(dev, m, t, idx, idx + j, masked, x_dtype, dec)
      r, r0 = rel64(got, want), rel64(px, want0)
      gate = 2 * P.ABS_WEIGHT_SUMS[j]
      print(f"idx={idx} j={j} masked={masked}: plms {r:.3e} / x0 {r0:.3e}; ddim {base:.3e} / x0 {base0:.3e}; "
            f"gate x{gate:.2f}")
      worst[j] = max(worst.get(j, 0.), r / base, r0 / base0)
      assert r <= gate * base and r0 <= gate * base0, (idx, j, r, r0, base, base0)
      # both halves of the next U-Net input are the rounded output
      assert torch.equal(xu[:B], got.to(x_dtype)) and torch.equal(xu[B:], got.to(x_dtype))
      # the ring: e_i in slot idx & 3 (three roundings of operands up to (1 + 2 s) |eps|), the others untouched
      assert rel64(ring[idx & 3], e_i) <= 8 * 2.0 ** -24
      for k in range(1, 4):
        assert torch.equal(ring[(idx + k) & 3], t["ring"][(idx + k) & 3])
      if masked and idx == 0:                                     # nothing is blended at index 0
        plain = _run_plms(dev, m, t, idx, idx + j, False, x_dtype, dec)
        assert torch.equal(got, plain[0]) and torch.equal(xu, plain[2])
      if masked and idx >= 1:                                     # pred_x0 and the ring keep the unblended step's values
        plain = _run_plms(dev, m, t, idx, idx + j, False, x_dtype, dec)
        assert torch.equal(px, plain[1]) and torch.equal(ring, plain[3]) and not torch.equal(got, plain[0])
        assert torch.equal(got[:, 1], plain[0][:, 1])             # mask row 1 = 0: regenerated cells
  print("worst error in units of the DDIM kernel's:", {j: round(v, 3) for j, v in worst.items()})


def test_start_below_index_and_far_above_clamp(dev):
  m, t, _ = _kernel_inputs(dev)
  a = _run_plms(dev, m, t, 5, 5, False, torch.float32, False)
  b = _run_plms(dev, m, t, 5, 2, False, torch.float32, False)       # start < idx: order 0
  assert torch.equal(a[0], b[0])
  c = _run_plms(dev, m, t, 5, 8, False, torch.float32, False)
  e = _run_plms(dev, m, t, 5, 9, False, torch.float32, False)       # start - idx > 3: order 3
  assert torch.equal(c[0], e[0]) and not torch.equal(a[0], c[0])


def test_rejects_what_it_cannot_vectorise(dev):
  from ldm_tf2_amd._lib import LdmHipError
  i = torch.zeros(1, dtype=torch.int32, device=dev)
  coef = torch.zeros(10, 4, device=dev)
  x = torch.zeros(2, 3, 3, 3, device=dev)                           # n_per_sample = 27
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.cfg_plms_update(torch.zeros(4, 3, 3, 3, device=dev), x, x.clone(), torch.zeros(4, 2, 3, 3, 3, device=dev),
                        coef, i, i.clone(), GS)


# ---- 2. slots beyond j are not read -----------------------------------------------------------------------
def test_slots_beyond_j_are_not_read(dev, unet_w, txt_w, kl_w):
  m, t, _ = _kernel_inputs(dev)
  for idx in (N - 1, 5, 0):
    for j in (0, 1, 2):
      rings = []
      for fill in (float("nan"), 0.):
        ring = torch.full_like(t["ring"], fill)
        for k in range(1, j + 1):
          ring[(idx + k) & 3] = t["ring"][(idx + k) & 3]
        rings.append(_run_plms(dev, m, t, idx, idx + j, True, torch.float32, False, ring=ring))
      (a, a0, au, _), (z, z0, zu, _) = rings
      assert bool(torch.isfinite(a).all() and torch.isfinite(a0).all() and torch.isfinite(au).all())
      assert torch.equal(a, z) and torch.equal(a0, z0) and torch.equal(au, zu)
  # a whole loop on a ring full of NaN
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  first = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T()).clone()
  s._ring.fill_(float("nan"))
  again = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T())
  assert bool(torch.isfinite(again).all()) and torch.equal(first, again)


# ---- 3. ring and graph ------------------------------------------------------------------------------------
def test_graph_replay_eager_and_ring(dev, unet_w, txt_w, kl_w, monkeypatch):
  ids, x_T = T._ids(), _x_T()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=True)
  got = s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T).clone()
  assert s._graph is not None
  ring_graph = s._ring.clone()
  again = s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T)
  assert torch.equal(got, again)                                    # a second replay reproduces the run
  s2 = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  guided = []
  real = ops.cfg_plms_update

  def spy(eps_all, *a, **k):
    guided.append((eps_all[:B] + GS * (eps_all[B:] - eps_all[:B])).cpu())
    return real(eps_all, *a, **k)
  monkeypatch.setattr(ops, "cfg_plms_update", spy)
  rec = []
  eager = s2.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T, record=rec)
  monkeypatch.setattr(ops, "cfg_plms_update", real)
  assert len(rec) == N and len(guided) == N and s2._graph is None
  assert torch.equal(got, eager)                                    # eager == graph replay
  assert torch.equal(ring_graph, s2._ring)
  for slot in range(4):                                             # e_3 .. e_0 in slots 3 .. 0 (guided[k] is index N-1-k)
    assert rel64(s2._ring[slot], guided[N - 1 - slot].double().numpy()) < 1e-6
    assert rel64(s2._ring[slot], guided[N - 1 - slot - 4].double().numpy()) > 1e-3
  assert s2._start.item() == N - 1


def test_no_stale_history_between_loops(dev, unet_w, txt_w, kl_w):
  ids, x_T = T._ids(), _x_T()
  img, E, Q, _, mask = T._inputs(0.)
  kw = dict(strength=0.5, encode_noise=E, q_noises=Q)
  fresh_img = _sampler(dev, torch.float32, unet_w, txt_w, kl_w).ddim_p_sample_loop_img2img(ids, img, GS, **kw).clone()
  fresh_inp = _sampler(dev, torch.float32, unet_w, txt_w, kl_w).ddim_p_sample_loop_img2img(ids, img, GS, mask=mask,
                                                                                             **kw).clone()
  fresh_txt = _sampler(dev, torch.float32, unet_w, txt_w, kl_w).ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T).clone()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T), fresh_txt)
  assert torch.equal(s.ddim_p_sample_loop_img2img(ids, img, GS, **kw), fresh_img)          # img2img right after txt2img
  assert s._start.item() == 4
  assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T), fresh_txt)             # txt2img after img2img
  assert torch.equal(s.ddim_p_sample_loop_img2img(ids, img, GS, mask=mask, **kw), fresh_inp)
  assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T), fresh_txt)
  assert not torch.equal(fresh_img, fresh_inp)


def test_sample_is_independent_of_batching(dev, unet_w, txt_w, kl_w):
  ids = T._ids()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  s.ddim_p_sample_loop(ids, SHAPE, GS, seed=3, first_sample_index=0)
  both = s._xt.cpu().clone()
  for i in range(B):
    s.ddim_p_sample_loop(ids[[i, B + i]], [1, HW, HW, 4], GS, seed=3, first_sample_index=i)
    one = s._xt.cpu()
    r = rel64(one[0], both[i].double().numpy())
    print(f"sample {i}: B=1 run against its row of the B=2 run: rel {r:.3e}")
    assert torch.equal(one[0], both[i]), (i, r)
  # the update kernel itself: one launch on both samples == one launch per sample
  m, t, _ = _kernel_inputs(dev)
  whole = _run_plms(dev, m, t, 5, 8, True, torch.float32, False)[0]
  d = lambda a: a.to(dev).contiguous()
  for i in range(B):
    out = torch.empty(1, HW, HW, 4, device=dev)
    ops.cfg_plms_update(d(t["eps_all"][[i, B + i]]), d(t["xt"][i:i + 1]), out, d(t["ring"][:, i:i + 1]), m._coef_dev,
                        torch.tensor([5], dtype=torch.int32, device=dev),
                        torch.tensor([8], dtype=torch.int32, device=dev), GS, z0=d(t["z0"][i:i + 1]),
                        mask=d(t["mask"][i:i + 1]), q_noise=d(t["Q"][:, i:i + 1]), q_coef=m._device_q_tables()[2],
                        q_index_stride=t["Q"][0, 0].numel())
    assert torch.equal(out.cpu()[0], whole[i])


# ---- 4. whole loops against the oracle composition ---------------------------------------------------------
_CACHE = {}


def _oracle_plms(context, w_unet, sched, x, start, blend=None):
  """`start + 1` steps of the specification: O.unet_forward on [x; x], CFG and plms_ref.plms_update in float32
  torch, the tables cast to float32 first; blend = (mask, z0, Q) pins kept cells for the next index.
  Returns [(x after the step, its pred_x0)]."""
  f = lambda name: np.asarray(sched[name]).astype(np.float32)
  c1, c2, a_prev = f("ddim_sqrt_recip_alphas_cumprod"), f("ddim_sqrt_recipm1_alphas_cumprod"), f("ddim_alphas_cumprod_prev")
  steps, ac = sched["ddim_steps"], sched["alphas_cumprod"]
  x = torch.as_tensor(x, dtype=torch.float32)
  hist, rec = [], []
  for i in range(start, -1, -1):
    t = np.full([2 * B], steps[i], dtype=np.int32)
    eps_all = O.unet_forward(torch.cat([x, x], 0), t, context, w_unet, torch.float32)
    hist.insert(0, eps_all[:B] + np.float32(GS) * (eps_all[B:] - eps_all[:B]))
    del hist[4:]
    x, x0 = P.plms_update(x, hist, i, min(start - i, 3), c1, c2, a_prev)
    assert x.dtype == torch.float32
    if blend is not None and i >= 1:
      mask, z0, Q = blend
      x = T.blend_ref(mask, T.q_sample_ref(ac, z0, [steps[i - 1]] * B, Q[i - 1]), x)
    rec.append((x.clone(), x0.clone()))
  return rec


def _oracle(kind, w):
  if kind in _CACHE:
    return _CACHE[kind]
  ids = T._ids()
  sched = O.make_schedule(LDM["num_steps"], LDM["beta_start"], LDM["beta_end"], 0., N)
  dec = lambda z: O.decoder_forward(z / LDM["scale_factor"], w["autoencoder"])
  if kind == "ddim":
    out = O.ddim_p_sample_loop(ids, _x_T(), w, LDM, guidance_scale=GS)
  else:
    context = O.text_encoder(ids, w["cond_stage_model"], torch.float32)
    if kind == "txt2img":
      rec = _oracle_plms(context, w["unet"], sched, _x_T(), N - 1)
      out = dict(images=dec(rec[-1][0]), rec=rec)
    else:
      k, masked = kind
      img, E, Q, _, mask = T._inputs(0.)
      _, _, sample = O.diagonal_gaussian(O.encoder_forward(torch.from_numpy(img), w["autoencoder"]), E)
      z0 = np.float32(LDM["scale_factor"]) * sample
      x = T.q_sample_ref(sched["alphas_cumprod"], z0, [sched["ddim_steps"][k - 1]] * B, Q[k - 1])
      rec = _oracle_plms(context, w["unet"], sched, x, k - 1, (mask, z0, Q) if masked else None)
      out = dict(images=dec(rec[-1][0]), rec=rec)
  _CACHE[kind] = out
  return out


def _ddim_loop_error(dev, dtype, w):
  """The existing DDIM loop against O.ddim_p_sample_loop, same weights, x_T and dtype: the base of the loop gates."""
  key = ("base", dtype)
  if key not in _CACHE:
    s = _sampler(dev, dtype, w["unet"], w["cond_stage_model"], w["autoencoder"], sampler="ddim")
    got = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T())
    _CACHE[key] = T.rel_err(got, _oracle("ddim", w))[0]
  return _CACHE[key]


def _loop_check(what, got, ref, dtype, base):
  r = T.rel_err(got, ref)[0]
  print(f"{what} [{dtype}]: plms loop {r:.3e}; ddim loop {base:.3e}; gate {base * 20 / 3:.3e}; "
        f"the project's loop gate {T.LOOP_REL[dtype]:.1e}")
  assert r <= base * 20. / 3., (what, r, base)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_txt2img_loop_against_oracle(dev, dtype, unet_w, txt_w, kl_w):
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = _ddim_loop_error(dev, dtype, w)
  ref = _oracle("txt2img", w)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  got = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T())
  _loop_check("txt2img latents", s._xt, ref["rec"][-1][0], dtype, base)
  _loop_check("txt2img images", got, ref["images"], dtype, base)
  # PLMS is not DDIM: the two float32 oracles differ by far more than the float32 gate
  assert T.rel_err(ref["images"], _oracle("ddim", w))[0] > 100 * base or dtype == torch.bfloat16


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("strength", [0.3, 1.0])
def test_img2img_loop_against_oracle(dev, dtype, strength, unet_w, txt_w, kl_w):
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = _ddim_loop_error(dev, dtype, w)
  k = int(strength * N)
  ref = _oracle((k, False), w)
  img, E, Q, _, _ = T._inputs(0.)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  got = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=strength, encode_noise=E, q_noises=Q)
  assert s._start.item() == k - 1
  _loop_check(f"img2img k={k} latents", s._xt, ref["rec"][-1][0], dtype, base)
  _loop_check(f"img2img k={k} images", got, ref["images"], dtype, base)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_inpainting_loop_against_oracle(dev, dtype, unet_w, txt_w, kl_w):
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = _ddim_loop_error(dev, dtype, w)
  ref = _oracle((8, True), w)
  img, E, Q, _, mask = T._inputs(0.)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  got = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=0.8, mask=mask, encode_noise=E, q_noises=Q)
  _loop_check("inpainting latents", s._xt, ref["rec"][-1][0], dtype, base)
  _loop_check("inpainting images", got, ref["images"], dtype, base)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_progressive_frames_against_oracle(dev, dtype, unet_w, txt_w, kl_w):
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = _ddim_loop_error(dev, dtype, w)
  ref = _oracle("txt2img", w)
  freq = 5
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  gi, gs, gx = s.ddim_p_sample_loop_progressive(T._ids(), SHAPE, GS, record_freq=freq, x_T=_x_T())
  assert tuple(gs.shape) == (B, N // freq, 8 * HW, 8 * HW, 3) and tuple(gx.shape) == tuple(gs.shape)
  dec = lambda z: O.decoder_forward(z / LDM["scale_factor"], w["autoencoder"])
  _loop_check("progressive images", gi, ref["images"], dtype, base)
  for r in range(N // freq):                                        # slot r keeps the step at index r * freq
    x, x0 = ref["rec"][N - 1 - r * freq]
    _loop_check(f"progressive sample frame {r}", gs[:, r], dec(x), dtype, base)
    _loop_check(f"progressive pred_x0 frame {r}", gx[:, r], dec(x0), dtype, base)
  plain = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T())
  assert torch.equal(plain, gi)


# ---- 5. no extra launch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("temb_table", [True, False])
def test_plms_step_has_the_ddim_steps_launches(dev, unet_w, txt_w, kl_w, monkeypatch, temb_table):
  img, E, Q, _, mask = T._inputs(0.)
  calls = {}
  for name in ("ddim", "plms"):
    s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, use_graph=False, temb_table=temb_table)
    s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=0.5, mask=mask, encode_noise=E, q_noises=Q, record=[])
    for masked in (False, True):
      s._index_dev.fill_(s._loop_start_index(4))
      s._set_loop_start(3)
      proxy = T._CountingLib(ops.lib)
      monkeypatch.setattr(ops, "lib", proxy)
      s._step(GS, False, None, dec_index=True, masked=masked)
      monkeypatch.setattr(ops, "lib", proxy._lib)
      torch.cuda.synchronize()
      calls[name, masked] = proxy.calls
  for masked in (False, True):
    ddim_entry = "ldm_cfg_ddim_update_masked" if masked else "ldm_cfg_ddim_update"
    assert calls["ddim", masked].count(ddim_entry) == 1 and calls["plms", masked].count("ldm_cfg_plms_update") == 1
    assert not any(c.startswith("ldm_cfg_ddim") for c in calls["plms", masked])
    swapped = ["ldm_cfg_plms_update" if c == ddim_entry else c for c in calls["ddim", masked]]
    assert swapped == calls["plms", masked] and len(swapped) > 1
  print({k: len(v) for k, v in calls.items()})


# ---- 6. sampler="ddim" is untouched ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_ddim_loop_is_the_direct_ddim_update_loop(dev, dtype, unet_w, txt_w, kl_w):
  """The default sampler's loop (graph replay) gives the bytes of U-Net + ldm_cfg_ddim_update called directly, step
  by step, as the loop did before the sampler switch existed; it owns no PLMS state."""
  ids, x_T = T._ids(), _x_T()
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="ddim")
  got = s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T).clone()
  lat = s._xt.clone()
  assert not hasattr(s, "_ring") and not hasattr(s, "_start") and s._graph_key[-1] == "ddim"
  xt = torch.from_numpy(x_T).to(dev)
  x2 = torch.empty_like(s._x2).copy_(torch.cat([xt, xt], 0))
  eps = torch.empty(2 * B, HW, HW, 4, device=dev)
  index = torch.zeros(1, dtype=torch.int32, device=dev)
  for i in range(N - 1, -1, -1):
    index.fill_(i)
    s._unet.forward(x2, steps=s._steps_dev, index=index, out=eps, paired_rows=True)
    ops.cfg_ddim_update(eps, xt, xt, s._coef_dev, index, GS, x_unet_out=x2)
  assert torch.equal(xt, lat)
  assert torch.equal(s.decode_first_stage(xt), got)


# ---- 7. CLI ---------------------------------------------------------------------------------------------------
def test_cli_sampler_key(dev, tmp_path, monkeypatch):
  from ldm_tf2_amd import run_ldm_sampler as R
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
                       "text_prompt": prompt, "vocab_dir": str(tmp_path), "sample_save_progress": False,
                       "sampler": "plms"},
      "pre_ckpt_paths": {"cond_stage_model": None, "unet": None, "autoencoder": None},
      "cond_stage_model": txt, "autoencoder_kl": kl, "unet": unet, "ldm": LDM,
  }
  path = tmp_path / "config.yaml"
  path.write_text(yaml.safe_dump(cfg))
  out = {}
  for name in ("plms", "ddim"):
    cfg["ldm_sampling"]["sampler"] = name
    path.write_text(yaml.safe_dump(cfg))
    R.main(["--config_path", str(path), "--dtype", "f32", "--seed", "7", "--out", str(tmp_path / f"{name}.npy")])
    out[name] = np.load(tmp_path / f"{name}.npy")
    assert out[name].dtype == np.uint8 and out[name].shape == (2, 128, 128, 3)
  # the Python call on the same configuration
  cfg["ldm_sampling"]["sampler"] = "plms"
  s = R.build_from_config(cfg, dtype=torch.float32, verbose=False)
  assert s._sampler == "plms"
  ids = get_token_ids(prompt, 2, str(tmp_path), 77)
  images = s.ddim_p_sample_loop(ids, [2, 16, 16, 4], 5.0, seed=7)
  assert np.array_equal(out["plms"], R.tensor_to_image(images))
  assert not np.array_equal(out["plms"], out["ddim"])
