"""img2img (SDEdit) and masked inpainting on the DDIM loop: the two kernels, the
latents of an image, and the whole loop against the CPU oracle composed step by step.

Restated here from the reference (LatentDiffusionModelTrainer, model_runners.py:580-625) and the
semantics of DESIGN.md section 7:
  q_sample(x0, t, eps) = _extract(sqrt_ac, t) * x0 + _extract(sqrt_1m_ac, t) * eps   (:580-600)
  z0 = scale_factor * posterior.sample(E) (KL) | scale_factor * encode(only_encode=True) (VQ)   (:602-625)
  k = int(strength * N); x = q_sample(z0, steps[k-1], Q[k-1]); DDIM indices k-1 .. 0;
  before the step at every index i < k-1: x <- m * q_sample(z0, steps[i], Q[i]) + (1 - m) * x.
Gates as test_models_gpu.py: free-running loops 1.3e-5 (f32) / 8e-2 (bf16) relative L2.
"""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

REL = {torch.float32: 5e-5, torch.bfloat16: 4e-2}
LOOP_REL = {torch.float32: 1.3e-5, torch.bfloat16: 8e-2}
DT = [torch.float32, torch.bfloat16]
UNET_CFG = dict(model_channels=64, out_channels=4, num_blocks=2, channel_mult=(1, 2, 4, 4), num_heads=8)
CTX_DIM = 128
TXT_CFG = dict(vocab_size=1000, encoder_stack_size=2, hidden_size=CTX_DIM, num_heads=4,
               size_per_head=32, max_seq_len=77, filter_size=256)
KL_CFG = dict(latent_channels=4, channels=64, num_blocks=2, multipliers=(1, 2, 4, 4))
VQ_CFG = dict(latent_channels=4, channels=64, num_blocks=2, multipliers=(1, 2, 2, 4),
              attention_resolutions=(8,), vocab_size=512)
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012, v_posterior=0., scale_factor=0.18215,
           eta=0., num_ddim_steps=10)
B, HW, N = 2, 16, 10


def rel_err(got, ref):
  got = got.detach().float().cpu().double()
  ref = torch.as_tensor(ref).detach().double()
  return ((got - ref).norm() / ref.norm()).item(), (got - ref).abs().max().item()


def check(got, ref, dtype, what, gate=None):
  r, m = rel_err(got, ref)
  gate = REL[dtype] if gate is None else gate
  print(f"{what} [{dtype}]: rel={r:.3e} maxabs={m:.3e}")
  assert r < gate, f"{what}: rel err {r:.3e} >= {gate:.1e} (max abs {m:.3e})"


def q_sample_ref(sched_ac, x0, t, eps):
  """model_runners.py:580-600 in float32: the f64 tables cast to float32, then gathered (_extract, :41-44)."""
  sa = torch.from_numpy(np.sqrt(sched_ac).astype(np.float32)[np.asarray(t)]).reshape(-1, 1, 1, 1)
  sb = torch.from_numpy(np.sqrt(1. - sched_ac).astype(np.float32)[np.asarray(t)]).reshape(-1, 1, 1, 1)
  return sa * torch.as_tensor(x0, dtype=torch.float32) + sb * torch.as_tensor(eps, dtype=torch.float32)


def blend_ref(m, q, x):
  """semantics 5: m * q + (1 - m) * x, m [B,h,w] broadcast over channels."""
  m = torch.as_tensor(m, dtype=torch.float32)[..., None]
  return m * q + (1 - m) * x


@pytest.fixture(scope="module")
def unet_w():
  return Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **UNET_CFG), seed=2, mode="random", scope="unet")


@pytest.fixture(scope="module")
def txt_w():
  return Wt.init_weights(Wt.transformer_manifest(**TXT_CFG), seed=2, mode="random", scope="cond_stage_model")


@pytest.fixture(scope="module")
def kl_w():
  m = Wt.decoder_manifest(**KL_CFG)
  m.update(Wt.encoder_manifest(**KL_CFG, image_size=8 * HW, double_z=True))
  return Wt.init_weights(m, seed=2, mode="random", scope="autoencoder")


def _sampler(dev, dtype, unet_w, txt_w, kl_w, ldm=LDM, use_graph=True):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=CTX_DIM)
  ae = AutoencoderKL(**KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, **ldm)


def _ids():
  g = np.random.default_rng(1)
  cond = g.integers(0, 1000, size=(1, 77))
  uncond = np.array([[101, 102] + [0] * 75])
  return np.concatenate([np.tile(uncond, (B, 1)), np.tile(cond, (B, 1))], 0)


def _inputs(eta):
  g = np.random.default_rng(21)
  img = (g.random((B, 8 * HW, 8 * HW, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
  E = g.standard_normal((B, HW, HW, 4), dtype=np.float32)
  Q = g.standard_normal((N, B, HW, HW, 4), dtype=np.float32)
  noises = g.standard_normal((N, B, HW, HW, 4), dtype=np.float32) if eta else None
  mask = np.zeros((B, HW, HW), np.float32)
  mask[:, :, : HW // 2] = 1.                                 # keep the left half
  return img, E, Q, noises, mask


_ORACLE = {}


def oracle_img2img(ids, img, w, ldm, k, E, Q, noises, mask, gs=5.):
  """The oracle composition: encoder -> posterior sample -> q_sample start -> k DDIM steps (blend before each
  but the first) -> decode.  Returns (images, z0, record of x after each step)."""
  key = (k, ldm["eta"], mask is not None)
  if key in _ORACLE:
    return _ORACLE[key]
  sched = O.make_schedule(ldm["num_steps"], ldm["beta_start"], ldm["beta_end"], ldm["eta"], ldm["num_ddim_steps"])
  steps, ac = sched["ddim_steps"], sched["alphas_cumprod"]
  context = O.text_encoder(ids, w["cond_stage_model"], torch.float32)
  _, _, sample = O.diagonal_gaussian(O.encoder_forward(torch.from_numpy(img), w["autoencoder"]), E)
  z0 = np.float32(ldm["scale_factor"]) * sample
  x = q_sample_ref(ac, z0, [steps[k - 1]] * B, Q[k - 1])
  rec = []
  for i in range(k - 1, -1, -1):
    noise = None if noises is None else noises[i]
    x, _, _ = O.ddim_sample(x, context, i, sched, w["unet"], gs, noise, clip_denoised=False)
    if mask is not None and i >= 1:
      x = blend_ref(mask, q_sample_ref(ac, z0, [steps[i - 1]] * B, Q[i - 1]), x)
    rec.append(x.clone())
  images = O.decoder_forward(x / ldm["scale_factor"], w["autoencoder"])
  _ORACLE[key] = (images, z0, rec)
  return _ORACLE[key]


# ---- 1. ldm_q_sample --------------------------------------------------------------------------------
def test_q_sample_kernel(dev):
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  m = LatentDiffusionModel(None, None, None, **LDM)
  sa, sb, per_index = m._device_q_tables()
  assert torch.equal(sa.cpu(), torch.from_numpy(m._sqrt_alphas_cumprod.astype(np.float32)))
  assert torch.equal(per_index[:, 1].cpu(),
                     torch.from_numpy(m._sqrt_one_minus_alphas_cumprod.astype(np.float32)[m._ddim_steps]))
  g = torch.Generator().manual_seed(3)
  x0 = torch.randn(4, 8, 8, 4, generator=g)
  eps = torch.randn(3, 4, 8, 8, 4, generator=g)
  t = np.array([0, 999, 500, 37], dtype=np.int32)
  ref = q_sample_ref(m._alphas_cumprod, x0, t, eps[1])
  xt = torch.empty(4, 8, 8, 4, device=dev)
  xu = torch.empty(8, 8, 8, 4, device=dev, dtype=torch.bfloat16)
  td = torch.from_numpy(t).to(dev)
  ops.q_sample(x0.to(dev), eps[1].contiguous().to(dev), td, sa, sb, xt, x_unet_out=xu)
  r, mx = rel_err(xt, ref)
  print(f"q_sample: rel={r:.3e} maxabs={mx:.3e}")
  assert r < 1e-6 and torch.allclose(xt.cpu(), ref, rtol=1e-6, atol=1e-6)
  assert torch.equal(xu[:4].cpu(), xt.cpu().to(torch.bfloat16))
  assert torch.equal(xu[4:].cpu(), xt.cpu().to(torch.bfloat16))
  # a noise table row selected by a device index; f32 x_unet copy
  xt2 = torch.empty_like(xt)
  xu2 = torch.empty(8, 8, 8, 4, device=dev)
  idx = torch.tensor([1], dtype=torch.int32, device=dev)
  ops.q_sample(x0.to(dev), eps.to(dev), td, sa, sb, xt2, x_unet_out=xu2, index=idx, noise_index_stride=eps[0].numel())
  assert torch.equal(xt2, xt) and torch.equal(xu2[:4], xt) and torch.equal(xu2[4:], xt)
  # the public method with the reference's signature
  assert torch.equal(m.q_sample(x0, t, eps[1]), xt)


# ---- 2. ldm_cfg_ddim_update_masked --------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_masked_update_kernel(dev, eta):
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  m = LatentDiffusionModel(None, None, None, **dict(LDM, eta=eta))
  sched = O.make_schedule(1000, 0.00085, 0.012, eta, N)
  coef = m._coef_dev
  _, _, qcoef = m._device_q_tables()
  g = torch.Generator().manual_seed(4)
  eps_all = torch.randn(2 * B, 8, 8, 4, generator=g)
  xt = torch.randn(B, 8, 8, 4, generator=g)
  z0 = torch.randn(B, 8, 8, 4, generator=g)
  noise = torch.randn(N, B, 8, 8, 4, generator=g)
  Q = torch.randn(N, B, 8, 8, 4, generator=g)
  soft = torch.rand(B, 8, 8, generator=g)
  soft[:, 0, :] = 1.
  soft[:, 1, :] = 0.
  d = lambda a: a.to(dev).contiguous()
  stride = noise[0].numel()

  def run(masked, mask, idx):
    out = torch.empty(B, 8, 8, 4, device=dev)
    xu = torch.empty(2 * B, 8, 8, 4, device=dev)
    px = torch.empty(B, 8, 8, 4, device=dev)
    index = torch.tensor([idx], dtype=torch.int32, device=dev)
    kw = dict(noise=d(noise), x_unet_out=xu, noise_index_stride=stride, pred_x0_out=px)
    if masked:
      ops.cfg_ddim_update_masked(d(eps_all), d(xt), out, coef, index, 5., d(z0), d(mask), d(Q), qcoef,
                                 q_index_stride=Q[0].numel(), **kw)
    else:
      ops.cfg_ddim_update(d(eps_all), d(xt), out, coef, index, 5., **kw)
    assert index.item() == idx
    return out.cpu(), xu.cpu(), px.cpu()

  for idx in (0, 1, 5, N - 1):
    upd, _ = O.ddim_update(xt, eps_all[:B], eps_all[B:], sched, idx, 5., noise[idx], torch.float32, False)
    want = upd if idx == 0 else blend_ref(soft, q_sample_ref(sched["alphas_cumprod"], z0,
                                                               [sched["ddim_steps"][idx - 1]] * B, Q[idx - 1]), upd)
    got, xu, px = run(True, soft, idx)
    r, mx = rel_err(got, want)
    print(f"masked update idx={idx} eta={eta}: rel={r:.3e} maxabs={mx:.3e}")
    assert r < 1e-5
    assert torch.equal(xu[:B], got) and torch.equal(xu[B:], got)
    plain, plain_xu, plain_px = run(False, soft, idx)
    assert torch.equal(px, plain_px)                        # pred_x0 is the unblended step's
    if idx == 0:
      assert torch.equal(got, plain) and torch.equal(xu, plain_xu)
    else:                                                   # kept rows are the q_sample of the next index
      kept = q_sample_ref(sched["alphas_cumprod"], z0, [sched["ddim_steps"][idx - 1]] * B, Q[idx - 1])
      assert torch.allclose(got[:, 0], kept[:, 0], rtol=1e-6, atol=1e-6)
      assert torch.equal(got[:, 1], plain[:, 1])
    zero, zero_xu, _ = run(True, torch.zeros(B, 8, 8), idx)
    assert torch.equal(zero, plain) and torch.equal(zero_xu, plain_xu)


# ---- 3. get_latents ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
def test_get_latents_kl(dev, dtype, kl_w):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  img, E, _, _, _ = _inputs(0.)
  m = LatentDiffusionModel(None, AutoencoderKL(**KL_CFG, weights=kl_w, dtype=dtype, device=dev), None, **LDM)
  got = m.get_latents(img, noise=E)
  _, _, sample = O.diagonal_gaussian(O.encoder_forward(torch.from_numpy(img), kl_w), E)
  check(got, np.float32(0.18215) * sample, dtype, "KL get_latents", gate=2 * REL[dtype])
  # default noise: the seed's ENCODE_STREAM, per global sample index
  from ldm_tf2_amd.model_runners import ENCODE_STREAM, normal_latents
  a = m.get_latents(img, seed=5, first_sample_index=3)
  b = m.get_latents(img, noise=normal_latents(5, 3, B, (HW, HW, 4), stream=ENCODE_STREAM))
  assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
def test_get_latents_vq(dev, dtype):
  from ldm_tf2_amd.autoencoder import AutoencoderVQ
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  man = Wt.decoder_manifest(**VQ_CFG, latent_size=8)
  man.update(Wt.encoder_manifest(**VQ_CFG, image_size=64, double_z=False))
  w = Wt.init_weights(man, seed=2, mode="random", scope="autoencoder")
  img = (np.random.default_rng(8).random((2, 64, 64, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
  ae = AutoencoderVQ(**VQ_CFG, latent_size=8, weights=w, dtype=dtype, device=dev)
  m = LatentDiffusionModel(None, ae, None, **LDM)
  got = m.get_latents(img)
  z, _, _, _ = O.vq_encode(torch.from_numpy(img), w, attention_resolutions=(8,))
  check(got, np.float32(0.18215) * z, dtype, "VQ get_latents")


# ---- 4. img2img end to end ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("strength", [0.3, 1.0])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_img2img_end_to_end(dev, dtype, strength, eta, unet_w, txt_w, kl_w):
  ldm = dict(LDM, eta=eta)
  k = int(strength * N)
  ids = _ids()
  img, E, Q, noises, _ = _inputs(eta)
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  ref, z0_ref, rec_ref = oracle_img2img(ids, img, w, ldm, k, E, Q, noises, None)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w, ldm=ldm, use_graph=True)
  kw = dict(strength=strength, encode_noise=E, q_noises=Q, noises=noises)
  got = s.ddim_p_sample_loop_img2img(ids, img, 5., **kw)
  assert tuple(got.shape) == (B, 8 * HW, 8 * HW, 3)
  check(s._z0_buf, z0_ref, dtype, "z0", gate=2 * REL[dtype])
  check(s._xt, rec_ref[-1], dtype, f"x_0 latents (k={k})", gate=LOOP_REL[dtype])
  check(got, ref, dtype, f"images (k={k})", gate=LOOP_REL[dtype])
  s2 = _sampler(dev, dtype, unet_w, txt_w, kl_w, ldm=ldm, use_graph=False)
  rec = []
  got2 = s2.ddim_p_sample_loop_img2img(ids, img, 5., record=rec, **kw)
  assert len(rec) == k
  assert torch.equal(got, got2)                              # eager == graph replay
  got3 = s.ddim_p_sample_loop_img2img(ids, img, 5., **kw)
  assert torch.equal(got, got3)                              # a second replay reproduces the run


# ---- 5. inpainting end to end ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
def test_inpainting_end_to_end(dev, dtype, unet_w, txt_w, kl_w):
  strength, k = 0.8, 8
  ids = _ids()
  img, E, Q, _, mask = _inputs(0.)
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  ref, _, rec_ref = oracle_img2img(ids, img, w, LDM, k, E, Q, None, mask)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w, use_graph=True)
  kw = dict(strength=strength, encode_noise=E, q_noises=Q)
  got = s.ddim_p_sample_loop_img2img(ids, img, 5., mask=mask, **kw)
  check(s._xt, rec_ref[-1], dtype, "inpainting x_0 latents", gate=LOOP_REL[dtype])
  check(got, ref, dtype, "inpainting images", gate=LOOP_REL[dtype])
  s2 = _sampler(dev, dtype, unet_w, txt_w, kl_w, use_graph=False)
  rec = []
  got2 = s2.ddim_p_sample_loop_img2img(ids, img, 5., mask=mask[0], record=rec, **kw)   # [h,w] is tiled
  assert len(rec) == k and torch.equal(got, got2)
  z0 = s2._z0_buf.cpu()
  steps, ac = s2._ddim_steps, s2._alphas_cumprod
  keep = torch.from_numpy(mask).bool()
  for j in range(k - 1):                       # after the step at index k-1-j, the cells kept for index k-2-j
    i = k - 2 - j
    want = q_sample_ref(ac, z0, [steps[i]] * B, Q[i])
    r = rel_err(rec[j].cpu()[keep], want[keep])[0]
    assert r < 1e-6, (j, r)
  assert not torch.equal(rec[-1].cpu()[keep], q_sample_ref(ac, z0, [steps[0]] * B, Q[0])[keep])
  # an all-zero mask is plain img2img, bit for bit
  zero = s.ddim_p_sample_loop_img2img(ids, img, 5., mask=np.zeros_like(mask), **kw)
  plain = s.ddim_p_sample_loop_img2img(ids, img, 5., **kw)
  assert torch.equal(zero, plain)


# ---- 6. the blend adds no launch ---------------------------------------------------------------------
class _CountingLib:
  def __init__(self, lib):
    self._lib, self.calls = lib, []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)

    def call(*args):
      self.calls.append(name)
      return fn(*args)
    return call


@pytest.mark.parametrize("temb_table", [True, False])
def test_mask_adds_no_launch(dev, unet_w, txt_w, kl_w, monkeypatch, temb_table):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  s = LatentDiffusionModelSampler(UNet(**UNET_CFG, weights=unet_w, device=dev, context_dim=CTX_DIM),
                                  AutoencoderKL(**KL_CFG, weights=kl_w, device=dev),
                                  TransformerModel(**TXT_CFG, weights=txt_w, device=dev),
                                  use_graph=False, verbose=False, temb_table=temb_table, **LDM)
  img, E, Q, _, mask = _inputs(0.)
  s.ddim_p_sample_loop_img2img(_ids(), img, 5., strength=0.5, mask=mask, encode_noise=E, q_noises=Q, record=[])
  counts = {}
  for masked in (False, True):
    s._index_dev.fill_(s._loop_start_index(4))
    proxy = _CountingLib(ops.lib)
    monkeypatch.setattr(ops, "lib", proxy)
    s._step(5., False, None, dec_index=True, masked=masked)
    monkeypatch.setattr(ops, "lib", proxy._lib)
    torch.cuda.synchronize()
    counts[masked] = proxy.calls
  print({k: len(v) for k, v in counts.items()})
  assert len(counts[True]) == len(counts[False]) > 1
  assert counts[True].count("ldm_cfg_ddim_update_masked") == 1 and "ldm_cfg_ddim_update" not in counts[True]
  assert counts[False].count("ldm_cfg_ddim_update") == 1


# ---- 7. txt2img after img2img ------------------------------------------------------------------------
def test_txt2img_after_img2img(dev, unet_w, txt_w, kl_w):
  ids = _ids()
  img, E, Q, _, mask = _inputs(0.)
  x_T = np.random.default_rng(9).standard_normal((B, HW, HW, 4)).astype(np.float32)
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  s.ddim_p_sample_loop_img2img(ids, img, 5., strength=0.5, mask=mask, encode_noise=E, q_noises=Q)
  after_masked = s.ddim_p_sample_loop(ids, [B, HW, HW, 4], 5., x_T=x_T)
  s.ddim_p_sample_loop_img2img(ids, img, 5., strength=0.5, encode_noise=E, q_noises=Q)
  after_plain = s.ddim_p_sample_loop(ids, [B, HW, HW, 4], 5., x_T=x_T)
  fresh = _sampler(dev, torch.float32, unet_w, txt_w, kl_w).ddim_p_sample_loop(ids, [B, HW, HW, 4], 5., x_T=x_T)
  assert torch.equal(after_masked, fresh) and torch.equal(after_plain, fresh)
  assert s.last_loop_ms_per_step() > 0


# ---- 8. errors ---------------------------------------------------------------------------------------
def test_errors(dev, unet_w, txt_w, kl_w):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  ids = _ids()
  img, E, Q, _, mask = _inputs(0.)
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  for strength in (0., 1.5):
    with pytest.raises(ValueError, match="strength"):
      s.ddim_p_sample_loop_img2img(ids, img, 5., strength=strength)
  with pytest.raises(ValueError, match="mask"):
    s.ddim_p_sample_loop_img2img(ids, img, 5., mask=np.ones((B, HW // 2, HW // 2), np.float32))
  with pytest.raises(ValueError, match="init_images"):
    s.ddim_p_sample_loop_img2img(ids, img[:, :, :, :2], 5.)
  dec_only = {k: v for k, v in kl_w.items() if not k.startswith(("encoder/", "quant_conv/"))}
  s._autoencoder = AutoencoderKL(**KL_CFG, weights=dec_only, device=dev)
  with pytest.raises(RuntimeError, match="without its encoder"):
    s.ddim_p_sample_loop_img2img(ids, img, 5.)


# ---- 9. CLI ------------------------------------------------------------------------------------------
def test_cli_img2img_inpainting(dev, tmp_path):
  from ldm_tf2_amd import run_ldm_sampler as R
  from ldm_tf2_amd.model_runners import ENCODE_STREAM, Q_STREAM, latent_mask, normal_latents
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
  g = np.random.default_rng(5)
  img = g.integers(0, 256, size=(128, 128, 3)).astype(np.uint8)
  pm = np.ones((128, 128), np.uint8)
  pm[40:100, 20:90] = 0                                       # regenerate this box
  np.save(tmp_path / "init.npy", img)
  np.save(tmp_path / "mask.npy", pm)
  cfg = {
      "ldm_sampling": {"autoencoder_type": "kl", "latent_shape": [2, 16, 16, 4], "guidance_scale": 5.0,
                       "text_prompt": prompt, "vocab_dir": str(tmp_path), "sample_save_progress": False,
                       "init_image": str(tmp_path / "init.npy"), "strength": 0.5,
                       "mask": str(tmp_path / "mask.npy")},
      "pre_ckpt_paths": {"cond_stage_model": None, "unet": None, "autoencoder": None},
      "cond_stage_model": txt, "autoencoder_kl": kl, "unet": unet, "ldm": LDM,
  }
  path = tmp_path / "config.yaml"
  path.write_text(yaml.safe_dump(cfg))
  out = tmp_path / "images.npy"
  R.main(["--config_path", str(path), "--dtype", "f32", "--seed", "7", "--out", str(out)])
  got = np.load(out)
  assert got.dtype == np.uint8 and got.shape == (2, 128, 128, 3)
  # the oracle pipeline on the same seeded (keras-init) weights and the same seeded draws
  ids = get_token_ids(prompt, 2, str(tmp_path), 77)
  am = Wt.decoder_manifest(**kl)
  am.update(Wt.encoder_manifest(**kl, image_size=256, double_z=True))
  w = {"unet": Wt.init_weights(Wt.unet_manifest(context_dim=128, **unet), seed=2, scope="unet"),
       "cond_stage_model": Wt.init_weights(Wt.transformer_manifest(**txt), seed=2, scope="cond_stage_model"),
       "autoencoder": Wt.init_weights(am, seed=2, scope="autoencoder")}
  k = 5
  E = normal_latents(7, 0, 2, (16, 16, 4), stream=ENCODE_STREAM)
  Q = np.zeros((N, 2, 16, 16, 4), np.float32)
  for i in range(k):
    Q[i] = normal_latents(7, 0, 2, (16, 16, 4), stream=Q_STREAM + i)
  images = np.tile(img[None].astype(np.float32) / np.float32(127.5) - np.float32(1.0), (2, 1, 1, 1))
  m = latent_mask(pm, 8)[0]
  assert m.sum() > 0 and (m == 0).sum() > 0
  _ORACLE.clear()
  ref, _, _ = oracle_img2img(ids, images, w, LDM, k, E, Q, None, np.tile(m[None], (2, 1, 1)))
  _ORACLE.clear()
  ref = np.asarray(O.tensor_to_image(ref))
  diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
  print("uint8 images: equal %.4f, max diff %d" % ((diff == 0).mean(), diff.max()))
  assert diff.max() <= 1 and (diff == 0).mean() > 0.99
