"""Model-level parity: HIP U-Net / text encoder / decoders / DDIM loop (through the
C ABI) against the CPU oracle on small configurations the oracle finishes in
seconds.  Same seeded weights (ldm_tf2_amd.weights.init_weights, mode="random" so
that biases and affine parameters are exercised), same x_T, same token ids.

Tolerances (relative L2 error ||got-ref|| / ||ref||, and max-abs):
  float32 : 5e-5 rel  -- summation order only (the f32 MFMA is an exact fma chain).  Calibrated
            (tools/calibrate_tolerance.py, profiles/r01_tolerance_calibration.txt): the oracle's
            own float32-vs-float64 drift is 2e-6 .. 4e-6 for one U-Net evaluation (tiny and
            full-size), a decoder pass and the free-running 10/50-step loops; the gate is ~12x
            that noise floor, and the HIP path measures 2e-6 .. 7e-6.
  bfloat16: 4e-2 rel  -- bf16 storage of weights and activations, f32 accumulation
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ldm_tf2_amd import weights as Wt  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

REL = {torch.float32: 5e-5, torch.bfloat16: 4e-2}
# free-running 10-step loops (x_0 latents, images, progressive frames): 2x the error measured on
# MI355X (f32: 5.0e-6 / 6.2e-6 / 6.3e-6 for eta = 0 / 1 / progressive -- no larger than ONE U-Net
# evaluation's, the trajectory does not amplify; bf16: 3.0e-2 / 4.0e-2), no free factor
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


def rel_err(got, ref):
  got = got.detach().float().cpu().double()
  ref = ref.detach().double()
  return ((got - ref).norm() / ref.norm()).item(), (got - ref).abs().max().item()


def check(got, ref, dtype, what, gate=None):
  r, m = rel_err(got, ref)
  print(f"{what} [{dtype}]: rel={r:.3e} maxabs={m:.3e}")
  gate = REL[dtype] if gate is None else gate
  assert r < gate, f"{what}: rel err {r:.3e} >= {gate:.1e} (max abs {m:.3e})"


@pytest.fixture(scope="module")
def unet_w():
  return Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **UNET_CFG), seed=2, mode="random", scope="unet")


@pytest.fixture(scope="module")
def txt_w():
  return Wt.init_weights(Wt.transformer_manifest(**TXT_CFG), seed=2, mode="random", scope="cond_stage_model")


@pytest.fixture(scope="module")
def kl_w():
  return Wt.init_weights(Wt.decoder_manifest(**KL_CFG), seed=2, mode="random", scope="autoencoder")


def _inputs(R=4, hw=16):
  g = np.random.default_rng(0)
  x = g.standard_normal((R, hw, hw, 4)).astype(np.float32)
  ctx = g.standard_normal((R, 77, CTX_DIM)).astype(np.float32)
  return x, ctx


@pytest.mark.parametrize("dtype", DT)
def test_unet_forward(dev, dtype, unet_w):
  from ldm_tf2_amd.unet import UNet
  x, ctx = _inputs()
  t = np.array([981, 981, 21, 500], dtype=np.int32)       # per-row timesteps (unet.py:118 contract)
  taps = {}
  ref = O.unet_forward(x, t, ctx, unet_w, taps=taps)
  unet = UNet(**UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=CTX_DIM)
  got = unet(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(ctx))
  assert got.dtype == torch.float32 and tuple(got.shape) == (4, 16, 16, 4)
  check(got, ref, dtype, "unet")
  # second call with the same context object re-uses the cached K/V and is deterministic
  got2 = unet(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(ctx))
  assert torch.equal(got, got2)
  # the oracle's per-block taps against the model's own (free-running, the same gate; the stage-local comparison is
  # tests/test_zz_block_parity_gpu.py): a block's tap is its last stage's
  mine = {}
  got3 = unet.forward(torch.from_numpy(x).to(dev), t_rows=torch.from_numpy(t).to(dev), taps=mine)
  assert torch.equal(got, got3)
  for blk, want in taps.items():
    last = [n for n in mine if n.startswith(blk + "/")][-1]
    assert last.rsplit("/", 1)[1] in ("residual", "spatial_transformer", "downsample", "upsample", "residual2")
    check(mine[last], want, dtype, f"unet tap {last}")


@pytest.mark.parametrize("dtype", DT)
def test_text_encoder(dev, dtype, txt_w):
  from ldm_tf2_amd.transformer import TransformerModel
  g = np.random.default_rng(1)
  cond = g.integers(0, 1000, size=(1, 77))
  uncond = np.array([[101, 102] + [0] * 75])
  ids = np.concatenate([np.tile(uncond, (3, 1)), np.tile(cond, (3, 1))], 0)    # run_ldm_sampler.py:42-45
  ref = O.text_encoder(ids, txt_w, num_heads=4, size_per_head=32)
  model = TransformerModel(**TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  got = model(ids)
  assert tuple(got.shape) == (6, 77, CTX_DIM)
  check(got, ref, dtype, "text_encoder")
  nodedup = TransformerModel(**TXT_CFG, weights=txt_w, dtype=dtype, device=dev, dedup_rows=False)
  assert torch.equal(nodedup(ids), got)


@pytest.mark.parametrize("dtype", DT)
def test_decoder_kl(dev, dtype, kl_w):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  g = np.random.default_rng(2)
  z = g.standard_normal((2, 8, 8, 4)).astype(np.float32)
  ref = O.decoder_forward(torch.from_numpy(z) / 0.18215, kl_w)
  ae = AutoencoderKL(**KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  got = ae.decode(torch.from_numpy(z), scale_factor=0.18215)
  assert tuple(got.shape) == (2, 64, 64, 3) and got.dtype == torch.float32
  check(got, ref, dtype, "decoder_kl")


@pytest.mark.parametrize("dtype", DT)
def test_decoder_vq(dev, dtype):
  from ldm_tf2_amd.autoencoder import AutoencoderVQ
  man = Wt.decoder_manifest(latent_size=8, **VQ_CFG)
  w = Wt.init_weights(man, seed=3, mode="random", scope="autoencoder")
  g = np.random.default_rng(3)
  z = (g.standard_normal((2, 8, 8, 4)) * 0.02).astype(np.float32)
  ref = O.decoder_forward(torch.from_numpy(z) / 0.18215, w, attention_resolutions=(8,), force_quantize=True)
  ae = AutoencoderVQ(**VQ_CFG, latent_size=8, weights=w, dtype=dtype, device=dev)
  got = ae.decode(torch.from_numpy(z), force_quantize=True, scale_factor=0.18215)
  assert tuple(got.shape) == (2, 64, 64, 3)
  check(got, ref, dtype, "decoder_vq")


def _build_sampler(dev, dtype, unet_w, txt_w, kl_w, ldm=LDM, use_graph=True):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=CTX_DIM)
  ae = AutoencoderKL(**KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, **ldm)


def _ids(B):
  g = np.random.default_rng(1)
  cond = g.integers(0, 1000, size=(1, 77))
  uncond = np.array([[101, 102] + [0] * 75])
  return np.concatenate([np.tile(uncond, (B, 1)), np.tile(cond, (B, 1))], 0)


def test_schedule_tables_match_oracle(dev, unet_w, txt_w, kl_w):
  """bit-exact integer step table; float tables equal the oracle's to the last bit."""
  s = _build_sampler(dev, torch.float32, unet_w, txt_w, kl_w, ldm=dict(LDM, num_ddim_steps=50, eta=0.3))
  o = O.make_schedule(1000, 0.00085, 0.012, 0.3, 50)
  assert s._ddim_steps.dtype == np.int32 and np.array_equal(s._ddim_steps, o["ddim_steps"])
  assert s._ddim_steps[-1] == 981
  for a, b in [(s._ddim_alphas_cumprod_prev, o["ddim_alphas_cumprod_prev"]), (s._ddim_sigmas, o["ddim_sigmas"]),
               (s._ddim_sqrt_recip_alphas_cumprod, o["ddim_sqrt_recip_alphas_cumprod"]),
               (s._ddim_sqrt_recipm1_alphas_cumprod, o["ddim_sqrt_recipm1_alphas_cumprod"])]:
    assert np.array_equal(a, b)
  with pytest.raises(IndexError):
    _build_sampler(dev, torch.float32, unet_w, txt_w, kl_w, ldm=dict(LDM, num_ddim_steps=300))


@pytest.mark.parametrize("dtype", DT)
def test_ddim_sample_single_step(dev, dtype, unet_w, txt_w, kl_w):
  """teacher-forced: one ddim_sample call at a given index (model_runners.py:438-472)."""
  s = _build_sampler(dev, dtype, unet_w, txt_w, kl_w, ldm=dict(LDM, eta=0.5))
  B = 2
  x, ctx = _inputs(R=2 * B)
  xt = x[:B]
  noise = np.random.default_rng(5).standard_normal(xt.shape).astype(np.float32)
  sched = O.make_schedule(1000, 0.00085, 0.012, 0.5, 10)
  ref, ref_x0, eps_ref = O.ddim_sample(xt, torch.from_numpy(ctx), 7, sched, unet_w, guidance_scale=5.,
                                       noise=noise, clip_denoised=False)
  got, got_x0 = s.ddim_sample(torch.from_numpy(xt), torch.from_numpy(ctx), 7, guidance_scale=5.,
                              clip_denoised=False, return_pred_x0=True, noise=noise)
  # (1) the U-Net evaluation inside the step meets the U-Net gate itself (no extra factor)
  eps_got = s._eps.detach().float().cpu()
  check(eps_got, eps_ref, dtype, "eps_all inside ddim_sample")
  # (2) the CFG + DDIM update is float32 arithmetic in both storage modes: fed the GPU's own eps it
  #     must reproduce the oracle's update to float32 rounding
  upd, upd_x0 = O.ddim_update(torch.from_numpy(xt), eps_got[:B], eps_got[B:], sched, 7, 5.,
                              torch.from_numpy(noise), torch.float32, False)
  assert rel_err(got, upd)[0] < 1e-5 and rel_err(got_x0, upd_x0)[0] < 1e-5
  # (3) hence the error of pred_x0 is the eps error amplified by exactly the modelled factor
  #     (model_runners.py:453,455-459): |d x0| <= c2 * ((s - 1) |d eps_u| + s |d eps_c|); no free factor
  c2 = float(np.float32(sched["ddim_sqrt_recipm1_alphas_cumprod"][7]))
  d = (eps_got - eps_ref).double()
  bound = c2 * (4.0 * d[:B].norm() + 5.0 * d[B:].norm()).item()
  err = (got_x0.detach().cpu().double() - ref_x0.double()).norm().item()
  print(f"pred_x0 [{dtype}]: |err| = {err:.3e} <= modelled bound {bound:.3e} (c2 = {c2:.3f})")
  assert err <= bound * 1.001 + 1e-6
  # the clipped variant (clip_denoised=True, the method's default) only contracts the error
  ref_c, ref_x0c, _ = O.ddim_sample(xt, torch.from_numpy(ctx), 7, sched, unet_w, guidance_scale=5.,
                                    noise=noise, clip_denoised=True)
  got_c, got_x0c = s.ddim_sample(torch.from_numpy(xt), torch.from_numpy(ctx), 7, guidance_scale=5.,
                                 clip_denoised=True, return_pred_x0=True, noise=noise)
  assert (got_x0c.detach().cpu().double() - ref_x0c.double()).norm().item() <= bound * 1.001 + 1e-6
  assert float(got_x0c.abs().max()) <= 1.0


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_loop_end_to_end(dev, dtype, eta, unet_w, txt_w, kl_w):
  """free-running: text encode -> 10 DDIM steps (HIP graph replay) -> KL decode."""
  B, n = 2, 10
  ldm = dict(LDM, eta=eta)
  ids = _ids(B)
  g = np.random.default_rng(7)
  x_T = g.standard_normal((B, 16, 16, 4)).astype(np.float32)
  noises = g.standard_normal((n, B, 16, 16, 4)).astype(np.float32) if eta else None
  rec = []
  ref = O.ddim_p_sample_loop(ids, x_T, dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w), ldm,
                             guidance_scale=5., noises=noises, record=rec, num_heads=8)
  # note: the oracle's text encoder needs this config's head layout
  s = _build_sampler(dev, dtype, unet_w, txt_w, kl_w, ldm=ldm, use_graph=True)
  got = s.ddim_p_sample_loop(ids, [B, 16, 16, 4], guidance_scale=5., x_T=x_T, noises=noises)
  assert tuple(got.shape) == (B, 128, 128, 3)
  check(s._xt, rec[-1], dtype, "x_0 latents", gate=LOOP_REL[dtype])
  check(got, ref, dtype, "images", gate=LOOP_REL[dtype])
  # eager (no graph) path gives bit-identical results to graph replay
  s2 = _build_sampler(dev, dtype, unet_w, txt_w, kl_w, ldm=ldm, use_graph=False)
  rec2 = []
  got2 = s2.ddim_p_sample_loop(ids, [B, 16, 16, 4], guidance_scale=5., x_T=x_T, noises=noises, record=rec2)
  assert len(rec2) == n
  assert torch.equal(got, got2)
  # replaying the captured graph a second time reproduces the run
  got3 = s.ddim_p_sample_loop(ids, [B, 16, 16, 4], guidance_scale=5., x_T=x_T, noises=noises)
  assert torch.equal(got, got3)


def test_progressive_sampling(dev, unet_w, txt_w, kl_w):
  """intended semantics of ddim_p_sample_loop_progressive (float32, eta=1)."""
  B, n, freq = 2, 10, 5
  ldm = dict(LDM, eta=1.0)
  ids = _ids(B)
  g = np.random.default_rng(11)
  x_T = g.standard_normal((B, 16, 16, 4)).astype(np.float32)
  noises = g.standard_normal((n, B, 16, 16, 4)).astype(np.float32)
  ri, rs, rx = O.ddim_p_sample_loop_progressive(ids, x_T, dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w),
                                                ldm, guidance_scale=5., record_freq=freq, noises=noises)
  s = _build_sampler(dev, torch.float32, unet_w, txt_w, kl_w, ldm=ldm)
  gi, gs, gx = s.ddim_p_sample_loop_progressive(ids, [B, 16, 16, 4], 5., record_freq=freq, x_T=x_T, noises=noises)
  assert tuple(gs.shape) == (B, n // freq, 128, 128, 3) and tuple(gx.shape) == tuple(gs.shape)
  check(gi, ri, torch.float32, "progressive: images", gate=LOOP_REL[torch.float32])
  check(gs, rs, torch.float32, "progressive: samples", gate=LOOP_REL[torch.float32])
  check(gx, rx, torch.float32, "progressive: pred_x0", gate=LOOP_REL[torch.float32])
  # the final images equal the plain loop's
  plain = s.ddim_p_sample_loop(ids, [B, 16, 16, 4], 5., x_T=x_T, noises=noises)
  assert rel_err(plain, gi.cpu())[0] < 1e-5


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
def test_unet_forward_fused_layernorm(dev, dtype):
  """LayerNorms emitted by the producing GEMM's epilogue (opt-in; C = 320 blocks) give the same U-Net."""
  from ldm_tf2_amd.unet import UNet
  cfg = dict(model_channels=320, out_channels=4, num_blocks=1, channel_mult=(1, 2), num_heads=8)
  w = Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **cfg), seed=3, mode="random", scope="unet")
  g = np.random.default_rng(5)
  x = g.standard_normal((2, 16, 16, 4)).astype(np.float32)
  ctx = g.standard_normal((2, 77, CTX_DIM)).astype(np.float32)
  t = np.array([981, 21], dtype=np.int32)
  ref = O.unet_forward(x, t, ctx, w)
  outs = []
  for fuse in (True, False):
    unet = UNet(**cfg, weights=w, dtype=dtype, device=dev, context_dim=CTX_DIM, fuse_layernorm=fuse)
    assert unet._fuse_ln == fuse
    got = unet(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(ctx))
    check(got, ref, dtype, f"unet (fused LayerNorm={fuse})")
    outs.append(got.float().cpu())
  if dtype == torch.float32:
    assert (outs[0] - outs[1]).abs().max().item() < 1e-4
