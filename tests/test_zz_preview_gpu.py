"""Latent previews: ldm_latent_preview against its restatement (tests/preview_ref.py), and the
txt2img / img2img loops with preview_freq against the same loops without it and against eager runs.

Gate of the kernel tests, the project's "twice the float32 emulation's error" rule: with t64 = preview64 and t32 =
preview32 of the same float32 inputs, e32 = max |t32 - t64| and delta = max(2 e32, 255 * 2^-23); every byte is within 1
of quantise(t64), and equal to it wherever t64 is farther than delta from every rounding threshold k + 0.5 and from
the clamp points 0 and 255.  The models, ids and LDM section are those of tests/test_img2img_gpu.py.

The module's name puts it behind the older GPU modules in the collection order, as tests/test_zz_norm_accounting_gpu.py
does: it extends the suite's run at its end and moves no earlier test."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import preview_ref as P  # noqa: E402
from ldm_tf2_amd import _lib, ops  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402

UNET_CFG = dict(model_channels=64, out_channels=4, num_blocks=2, channel_mult=(1, 2, 4, 4), num_heads=8)
CTX_DIM = 128
TXT_CFG = dict(vocab_size=1000, encoder_stack_size=2, hidden_size=CTX_DIM, num_heads=4,
               size_per_head=32, max_seq_len=77, filter_size=256)
KL_CFG = dict(latent_channels=4, channels=64, num_blocks=2, multipliers=(1, 2, 4, 4))
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012, v_posterior=0., scale_factor=0.18215,
           eta=0., num_ddim_steps=10)
B, HW, N = 2, 16, 10
Q, SCALE = 3, 2                                   # preview_freq and scale of the loop tests: R = 4 slots
CANARY, PAD = 0xA5, 64


# ---- the kernel through a canary-filled byte buffer ------------------------------------------------------
def _frames(dev, R, Bn, sh, sw, offset):
  """(whole byte buffer, the [R,Bn,sh,sw,3] view that starts PAD + offset bytes into it)."""
  n = R * Bn * sh * sw * 3
  buf = torch.full((PAD + offset + n + PAD,), CANARY, dtype=torch.uint8, device=dev)
  return buf, buf[PAD + offset:PAD + offset + n].view(R, Bn, sh, sw, 3)


def _run(dev, lat, proj, scale, mode, R=3, freq=2, index=1, bias=1, offset=0, lat_b=None, use_index=True):
  """One launch; returns (frames_a [R,..] NumPy, the pads' bytes, frames_b or None)."""
  lat_d = torch.from_numpy(np.ascontiguousarray(lat, dtype=np.float32)).to(dev)
  proj_d = torch.from_numpy(np.ascontiguousarray(proj, dtype=np.float32)).to(dev)
  Bn, h, w, _ = lat.shape
  buf, fr = _frames(dev, R, Bn, scale * h, scale * w, offset)
  kw = {}
  bufb = None
  if lat_b is not None:
    bufb, frb = _frames(dev, R, Bn, scale * h, scale * w, offset)
    kw = dict(lat_b=torch.from_numpy(np.ascontiguousarray(lat_b, dtype=np.float32)).to(dev), frames_b=frb)
  idx = torch.tensor([index], dtype=torch.int32, device=dev) if use_index else None
  ops.latent_preview(lat_d, proj_d, fr, freq, index=idx, index_bias=bias, scale=scale, mode=mode, **kw)
  torch.cuda.synchronize()
  assert idx is None or idx.item() == index                    # the launch does not move the counter
  pads = lambda b: np.concatenate([b[:PAD + offset].cpu().numpy(), b[-PAD:].cpu().numpy()])
  out_b = None
  if bufb is not None:
    assert (pads(bufb) == CANARY).all()
    out_b = frb.cpu().numpy()
  return fr.cpu().numpy(), pads(buf), out_b


def _gate(got, lat, proj, scale, mode, what):
  """The docstring's gate on one slot's bytes; returns the band share."""
  lat32, proj32 = np.asarray(lat, np.float32), np.asarray(proj, np.float32)
  t64 = P.preview64(lat32, proj32, scale, mode)
  e32 = np.abs(P.preview32(lat32, proj32, scale, mode).astype(np.float64) - t64).max()
  delta = max(2. * e32, 255. * 2. ** -23)
  thresholds = (t64 > -1.) & (t64 < 256.) & (np.abs(t64 - np.floor(t64) - 0.5) <= delta)
  band = thresholds | (np.abs(t64) <= delta) | (np.abs(t64 - 255.) <= delta)
  share = band.mean()
  # a condition on the test's own inputs, checked on the host before any byte is compared
  assert share <= 0.01, f"{what}: {share:.2%} of the bytes lie within delta={delta:.2e} of a threshold: choose another seed"
  want = P.quantise(t64)
  diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
  print(f"{what}: e32={e32:.3e} delta={delta:.3e} band={share:.2e} unequal={int((diff != 0).sum())} max diff={diff.max()}")
  assert diff.max() <= 1, f"{what}: a byte is {diff.max()} off"
  assert (diff[~band] == 0).all(), f"{what}: {int((diff[~band] != 0).sum())} bytes outside the band differ"
  return share


SHAPES = [(4, 5, 7, 3), (4, 16, 16, 2), (4, 1, 1, 8), (3, 3, 5, 1), (4, 16, 16, 8)]      # (c, h, w, scale)


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("c,h,w,scale", SHAPES)
def test_kernel_against_restatement(dev, c, h, w, scale, mode):
  g = np.random.default_rng(100 * c + 10 * h + scale)
  lat = g.standard_normal((B, h, w, c)).astype(np.float32)
  proj = (0.3 * g.standard_normal((c + 1, 3))).astype(np.float32)
  runs = {}
  # byte offsets 0 and 1 (and 2: with an odd slot size it is the offset at which slot 1 is dword-aligned)
  for offset in (0, 1, 2):
    fr, pads, _ = _run(dev, lat, proj, scale, mode, R=3, freq=2, index=1, bias=1, offset=offset)     # idx 2: slot 1
    assert (pads == CANARY).all(), f"offset {offset}: a pad byte was written"
    assert (fr[0] == CANARY).all() and (fr[2] == CANARY).all(), f"offset {offset}: another slot was written"
    runs[offset] = fr[1]
  assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])      # dword and byte paths agree
  again, _, _ = _run(dev, lat, proj, scale, mode, R=3, freq=2, index=1, bias=1, offset=0)
  assert np.array_equal(again[1], runs[0])                                           # deterministic
  assert (runs[0] != CANARY).any()
  _gate(runs[0], lat, proj, scale, mode, f"c={c} {h}x{w} s={scale} {mode}")


def test_kernel_generic_channel_count(dev):
  """c = 4 and c = 3 keep the matrix in registers; any other c reads it in the channel loop: the same gate at the
  ends of the range."""
  for c in (1, 5, 16):
    g = np.random.default_rng(c)
    lat = g.standard_normal((B, 3, 5, c)).astype(np.float32)
    proj = (0.3 / np.sqrt(c) * g.standard_normal((c + 1, 3))).astype(np.float32)
    for mode in P.MODES:
      fr, pads, _ = _run(dev, lat, proj, 3, mode)
      assert (pads == CANARY).all() and (fr[0] == CANARY).all() and (fr[2] == CANARY).all()
      _gate(fr[1], lat, proj, 3, mode, f"c={c} {mode}")


@pytest.mark.parametrize("mode,scale", [("nearest", 1), ("nearest", 3), ("nearest", 8), ("bilinear", 2), ("bilinear", 4)])
def test_exact_grids(dev, mode, scale):
  """Latents k/2 in [-2, 2], matrix and bias entries k/4 in [-1, 1]: every intermediate of either evaluation order is
  exact in float32, so the bytes equal quantise(preview64) everywhere, ties included.  Bit count: the bilinear
  fractions at scales 2 and 4 are multiples of 1/8, so wy wx is a multiple of 2^-6, wy wx lat one of 2^-7 and the
  upscaled latent, at most 2 in size, needs 9 bits; times a matrix entry it is a multiple of 2^-9, and v, the bias
  plus c = 4 such terms, at most 9 in size, needs 13 bits; 127.5 v = 255 v / 2 is a multiple of 2^-10 below 1148, and
  t = 127.5 v + 127.5 below 1276 needs 21 bits (projecting first: p a multiple of 2^-3 below 9, wy wx p a multiple of
  2^-9, the same t).  All are below float32's 24.  A tie inside the range is t = 127.5 exactly, v = 0."""
  g = np.random.default_rng(7 + scale)
  lat = (g.integers(-4, 5, size=(B, 6, 9, 4)) / 2.).astype(np.float32)
  lat[:, 0, :3] = 0.                                       # v = bias = 0 there: ties also in the clamped corner taps
  proj = (g.integers(-4, 5, size=(5, 3)) / 4.).astype(np.float32)
  proj[4] = [0., 0.25, -0.5]
  t64 = P.preview64(lat, proj, scale, mode)
  assert np.array_equal(P.preview32(lat, proj, scale, mode).astype(np.float64), t64)      # exact, as claimed
  ties = (t64 >= 0.) & (t64 <= 255.) & (t64 - np.floor(t64) == 0.5)
  assert ties.sum() > 0
  for offset in (0, 1):
    fr, pads, _ = _run(dev, lat, proj, scale, mode, offset=offset)
    assert (pads == CANARY).all()
    assert np.array_equal(fr[1], P.quantise(t64)), f"{mode} s={scale} offset {offset}"
  assert (fr[1][ties] == np.floor(t64[ties]) + 1).all()    # a tie rounds up


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("h,w,scale", [(5, 7, 3), (2, 2, 2)])
def test_one_hot_probes(dev, h, w, scale, mode):
  """Image p of the batch is 1 at cell p, channel 0; bias -1 makes the background byte 0 and a weight 2 saturates a
  unit latent, so a byte is nonzero exactly where a tap with a nonzero weight reads cell p: every tap of every output
  pixel is accounted for, the clamped borders included (the smallest nonzero weight, 1/36 at scale 3, gives byte 7)."""
  n = h * w
  lat = np.zeros((n, h, w, 4), np.float32)
  lat.reshape(n, n, 4)[np.arange(n), np.arange(n), 0] = 1.
  proj = np.array([[2., 2., 2.], [0.7, -0.3, 0.2], [-0.4, 0.6, 0.1], [0.3, 0.3, -0.9], [-1., -1., -1.]], np.float32)
  want = P.quantise(P.preview64(lat, proj, scale, mode))
  assert (want != 0).any(axis=(1, 2, 3)).all() and (want == 0).any()
  fr, pads, _ = _run(dev, lat, proj, scale, mode)
  assert (pads == CANARY).all()
  assert np.array_equal(fr[1] != 0, want != 0)
  assert np.abs(fr[1].astype(np.int16) - want.astype(np.int16)).max() <= 1
  if mode == "nearest":
    assert np.array_equal(fr[1], want) and (fr[1] != 0).sum() == n * scale * scale * 3


def test_launches_that_write_nothing(dev):
  g = np.random.default_rng(3)
  lat = g.standard_normal((B, 5, 7, 4)).astype(np.float32)
  lat_b = g.standard_normal((B, 5, 7, 4)).astype(np.float32)
  proj = (0.3 * g.standard_normal((5, 3))).astype(np.float32)
  # R = 3, freq = 2: idx 3 is no multiple, idx 6 is slot 3 >= R, idx -2 and -1 are negative
  for index, bias in ((2, 1), (3, 0), (6, 0), (5, 1), (-2, 0), (0, -1), (-3, 1)):
    fr, pads, frb = _run(dev, lat, proj, 3, "bilinear", index=index, bias=bias, lat_b=lat_b)
    assert (fr == CANARY).all() and (frb == CANARY).all() and (pads == CANARY).all(), (index, bias)
  # no index pointer: idx = index_bias
  fr, _, _ = _run(dev, lat, proj, 3, "bilinear", bias=4, use_index=False)
  assert (fr[0] == CANARY).all() and (fr[1] == CANARY).all() and (fr[2] != CANARY).any()
  fr, _, _ = _run(dev, lat, proj, 3, "bilinear", bias=3, use_index=False)
  assert (fr == CANARY).all()


@pytest.mark.parametrize("mode", P.MODES)
def test_second_source_and_nan(dev, mode):
  g = np.random.default_rng(4)
  lat = g.standard_normal((B, 5, 7, 4)).astype(np.float32)
  lat_b = g.standard_normal((B, 5, 7, 4)).astype(np.float32)
  proj = (0.3 * g.standard_normal((5, 3))).astype(np.float32)
  for offset in (0, 2):
    fa, pads, fb = _run(dev, lat, proj, 3, mode, lat_b=lat_b, offset=offset)
    one_a, _, _ = _run(dev, lat, proj, 3, mode, offset=offset)
    one_b, _, _ = _run(dev, lat_b, proj, 3, mode, offset=offset)
    assert (pads == CANARY).all()
    assert np.array_equal(fa, one_a) and np.array_equal(fb, one_b)            # untouched slots included
    assert not np.array_equal(fa[1], fb[1])
  # a NaN latent: bytes 0 wherever it projects, no error
  bad = lat.copy()
  bad[1, 2, 3, 1] = np.nan
  t64 = P.preview64(bad, proj, 3, mode)
  fr, pads, _ = _run(dev, bad, proj, 3, mode)
  hit = np.isnan(t64)
  assert hit.any() and not hit.all() and (pads == CANARY).all()
  assert (fr[1][hit] == 0).all()
  assert hit[1, 6:9, 9:12].all()                                               # the cell's own pixels, all three bytes
  clean, _, _ = _run(dev, lat, proj, 3, mode)
  assert np.array_equal(fr[1][~hit], clean[1][~hit])


def test_argument_errors(dev):
  lat = torch.zeros(B, 4, 4, 4, device=dev)
  proj = torch.zeros(5, 3, device=dev)
  fr = torch.zeros(2 * B * 8 * 8 * 3, dtype=torch.uint8, device=dev)
  frb = torch.zeros_like(fr)
  idx = torch.zeros(1, dtype=torch.int32, device=dev)
  good = dict(lat_a=lat.data_ptr(), lat_b=lat.data_ptr(), proj=proj.data_ptr(), frames_a=fr.data_ptr(),
              frames_b=frb.data_ptr(), index=idx.data_ptr(), index_bias=0, freq=1, R=2, B=B, h=4, w=4, c=4, scale=2,
              mode=1)
  names = list(good)

  def call(**change):
    a = dict(good, **change)
    return ops.lib.ldm_latent_preview(*[a[n] for n in names], None)

  assert call() == _lib.OK and call(lat_b=None, frames_b=None) == _lib.OK and call(index=None) == _lib.OK
  torch.cuda.synchronize()
  cases = [dict(lat_a=None), dict(proj=None), dict(frames_a=None), dict(lat_b=None), dict(frames_b=None),
           dict(c=0), dict(c=17), dict(scale=0), dict(scale=17), dict(freq=0), dict(R=0), dict(mode=2), dict(mode=-1),
           dict(B=0), dict(h=0), dict(w=-1)]
  for change in cases:
    assert call(**change) == _lib.ERR_ARG, change
    msg = _lib.last_error()
    assert msg.startswith("ldm_latent_preview"), (change, msg)
  torch.cuda.synchronize()
  with pytest.raises(ValueError, match="preview mode"):
    ops.latent_preview(lat, proj, fr.view(2, B, 8, 8, 3), 1, scale=2, mode="bicubic")
  assert "latent_preview" in ops.__all__ and _lib.PREVIEW_MODES == {"nearest": 0, "bilinear": 1}
  assert ctypes.c_void_p in _lib.SIGNATURES["ldm_latent_preview"][1]


# ---- the loops -----------------------------------------------------------------------------------------
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


PROJ = (0.3 * np.random.default_rng(17).standard_normal((5, 3))).astype(np.float32)


def _sampler(dev, unet_w, txt_w, kl_w, use_graph=True, preview=True, **kw):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  s = LatentDiffusionModelSampler(UNet(**UNET_CFG, weights=unet_w, device=dev, context_dim=CTX_DIM),
                                  AutoencoderKL(**KL_CFG, weights=kl_w, device=dev),
                                  TransformerModel(**TXT_CFG, weights=txt_w, device=dev), use_graph=use_graph,
                                  verbose=False, **dict(LDM, **kw))
  if preview:
    s.set_preview(PROJ, scale=SCALE, mode="bilinear")
  return s


def _ids():
  g = np.random.default_rng(1)
  cond = g.integers(0, 1000, size=(1, 77))
  uncond = np.array([[101, 102] + [0] * 75])
  return np.concatenate([np.tile(uncond, (B, 1)), np.tile(cond, (B, 1))], 0)


def _img_inputs():
  g = np.random.default_rng(21)
  img = (g.random((B, 8 * HW, 8 * HW, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
  E = g.standard_normal((B, HW, HW, 4), dtype=np.float32)
  mask = np.zeros((B, HW, HW), np.float32)
  mask[:, :, : HW // 2] = 1.
  return img, E, mask


def _op_preview(dev, lat):
  """ops.latent_preview of one latent tensor with the loop tests' matrix, scale and mode: uint8 [B,H,W,3]."""
  fr = torch.zeros(1, B, SCALE * HW, SCALE * HW, 3, dtype=torch.uint8, device=dev)
  ops.latent_preview(lat.contiguous(), torch.from_numpy(PROJ).to(dev), fr, 1, scale=SCALE, mode="bilinear")
  return fr[0].cpu().numpy()


def _call(s, kind, ids, seed=3, **kw):
  """(images, final latents) of one call of the loop under test."""
  if kind == "img2img":
    img, E, mask = _img_inputs()
    images = s.ddim_p_sample_loop_img2img(ids, img, 5., strength=0.5, mask=mask, encode_noise=E, seed=seed, **kw)
  elif kind == "interval":
    images = s.ddim_p_sample_loop(ids, [B, HW, HW, 4], 5., seed=seed, guidance_interval=(300, 700), **kw)
  else:
    images = s.ddim_p_sample_loop(ids, [B, HW, HW, 4], 5., seed=seed, **kw)
  return images.clone(), s._xt.clone()


CASES = [("txt2img", solver, noise) for solver in ("ddim", "plms", "deis") for noise in ("host", "device")]
CASES += [("interval", "ddim", "host"), ("interval", "plms", "device"), ("interval", "deis", "host")]
CASES += [("img2img", "ddim", "host"), ("img2img", "plms", "device"), ("img2img", "deis", "host")]


@pytest.mark.parametrize("kind,solver,noise", CASES)
def test_loop_previews(dev, unet_w, txt_w, kl_w, kind, solver, noise):
  ids = _ids()
  k = 5 if kind == "img2img" else N
  R = (N - 1) // Q + 1
  s = _sampler(dev, unet_w, txt_w, kl_w, sampler=solver, noise_source=noise)
  images, latents = _call(s, kind, ids, preview_freq=Q)
  pv = s.last_previews()
  if kind == "interval":
    assert set(s._pv_sched_graphs) == {True, False}            # both captured forms carry the launch
  plain_images, plain_latents = _call(s, kind, ids)
  assert torch.equal(images, plain_images) and torch.equal(latents, plain_latents)
  # shapes, indices, written
  assert pv["sample"].dtype == np.uint8 and pv["sample"].shape == pv["pred_x0"].shape == (B, R, SCALE * HW, SCALE * HW, 3)
  assert np.array_equal(pv["indices"], [0, 3, 6, 9])
  assert np.array_equal(pv["written"], [r * Q <= k - 1 for r in range(R)])
  for r in range(R):
    if not pv["written"][r]:                                   # the slots the loop never reaches stay 0
      assert (pv["sample"][:, r] == 0).all() and (pv["pred_x0"][:, r] == 0).all()
  # an eager run of the same call: record for the samples, its own strips for pred_x0
  e = _sampler(dev, unet_w, txt_w, kl_w, use_graph=False, sampler=solver, noise_source=noise)
  rec = []
  e_images, _ = _call(e, kind, ids, preview_freq=Q, record=rec)
  assert len(rec) == k and torch.equal(e_images, images)
  epv = e.last_previews()
  for r in range(R):
    if pv["written"][r]:
      want = _op_preview(dev, rec[k - 1 - Q * r])
      assert np.array_equal(pv["sample"][:, r], want), f"sample slot {r}"
      assert (pv["pred_x0"][:, r] != 0).any()
  assert np.array_equal(pv["pred_x0"], epv["pred_x0"]) and np.array_equal(pv["sample"], epv["sample"])
  assert not np.array_equal(pv["pred_x0"][:, 1], pv["sample"][:, 1])


def test_loop_pred_x0_counter_bias_and_graph_reuse(dev, unet_w, txt_w, kl_w):
  ids = _ids()
  shape = [B, HW, HW, 4]
  s = _sampler(dev, unet_w, txt_w, kl_w)
  plain = s.ddim_p_sample_loop(ids, shape, 5., seed=3).clone()
  g_plain, key_plain = s._graph, s._graph_key
  assert g_plain is not None and s._pv_graph is None
  images = s.ddim_p_sample_loop(ids, shape, 5., seed=3, preview_freq=Q)
  assert torch.equal(images, plain)
  pv = s.last_previews()
  g_pv = s._pv_graph
  assert g_pv is not None and s._graph is g_plain and s._graph_key == key_plain
  assert s._pv_graph_key[:-1] == key_plain and s._pv_graph_key[-1] == ("preview", Q, SCALE, "bilinear")
  # another seed: nothing new is captured, the strips change
  s.ddim_p_sample_loop(ids, shape, 5., seed=4, preview_freq=Q)
  assert s._pv_graph is g_pv and s._graph is g_plain
  assert not np.array_equal(s.last_previews()["sample"], pv["sample"])
  # without the keyword afterwards: the graph it had before
  again = s.ddim_p_sample_loop(ids, shape, 5., seed=3)
  assert s._graph is g_plain and s._pv_graph is g_pv and torch.equal(again, plain)
  # set_preview: the same three change nothing; another scale drops the preview graphs and no others
  s.set_preview(PROJ, scale=SCALE, mode="bilinear")
  assert s._pv_graph is g_pv
  s.set_preview(PROJ, scale=SCALE, mode="nearest")
  assert s._pv_graph is None and s._graph is g_plain
  s.ddim_p_sample_loop(ids, shape, 5., seed=3, preview_freq=Q)
  near = s.last_previews()
  assert s._pv_graph_key[-1] == ("preview", Q, SCALE, "nearest") and not np.array_equal(near["sample"], pv["sample"])
  assert np.array_equal(near["sample"][:, :, ::2, ::2], near["sample"][:, :, 1::2, 1::2])
  # temb_table=False: the update moves the counter at its end (index_bias 1); the strips are the same
  t = _sampler(dev, unet_w, txt_w, kl_w, temb_table=False)
  t_images = t.ddim_p_sample_loop(ids, shape, 5., seed=3, preview_freq=Q)
  tpv = t.last_previews()
  assert t._pre_dec is False and s._pre_dec is True
  assert torch.equal(t_images, plain)
  assert np.array_equal(tpv["sample"], pv["sample"]) and np.array_equal(tpv["pred_x0"], pv["pred_x0"])
  # slot 0's pred_x0 is the DDIM step's at index 0 from the latents before it
  e = _sampler(dev, unet_w, txt_w, kl_w, use_graph=False)
  rec = []
  e.ddim_p_sample_loop(ids, shape, 5., seed=3, record=rec)
  context = e._cond_stage_model(ids)
  _, x0 = e.ddim_sample(rec[N - 2], context, 0, guidance_scale=5., clip_denoised=False, return_pred_x0=True)
  assert np.array_equal(pv["pred_x0"][:, 0], _op_preview(dev, x0))
  with pytest.raises(ValueError, match="on_preview needs preview_freq"):
    s.ddim_p_sample_loop(ids, shape, 5., on_preview=lambda *a: None)
  with pytest.raises(ValueError, match="preview matrix"):
    _sampler(dev, unet_w, txt_w, kl_w, preview=False).ddim_p_sample_loop(ids, shape, 5., preview_freq=Q)


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
def test_preview_adds_one_launch(dev, unet_w, txt_w, kl_w, monkeypatch, temb_table):
  """Eager loops of N steps, every C-ABI call counted: with previews there are exactly N more, all of them
  ldm_latent_preview; without, none."""
  s = _sampler(dev, unet_w, txt_w, kl_w, use_graph=False, temb_table=temb_table)
  ids = _ids()
  s.ddim_p_sample_loop(ids, [B, HW, HW, 4], 5., seed=3, preview_freq=Q)          # (every buffer and table exists)
  counts = {}
  for q in (None, Q, 1):
    proxy = _CountingLib(ops.lib)
    monkeypatch.setattr(ops, "lib", proxy)
    s.ddim_p_sample_loop(ids, [B, HW, HW, 4], 5., seed=3, preview_freq=q)
    monkeypatch.setattr(ops, "lib", proxy._lib)
    torch.cuda.synchronize()
    counts[q] = proxy.calls
  print({q: len(v) for q, v in counts.items()})
  assert "ldm_latent_preview" not in counts[None]
  for q in (Q, 1):                                             # one launch per step, whatever the frequency
    assert counts[q].count("ldm_latent_preview") == N
    assert len(counts[q]) == len(counts[None]) + N
    assert [c for c in counts[q] if c != "ldm_latent_preview"] == counts[None]
    # the launch follows the step's update directly
    where = [i for i, c in enumerate(counts[q]) if c == "ldm_latent_preview"]
    assert all(counts[q][i - 1] == "ldm_cfg_ddim_update" for i in where)


def test_on_preview(dev, unet_w, txt_w, kl_w):
  s = _sampler(dev, unet_w, txt_w, kl_w)
  seen = []
  s.ddim_p_sample_loop(_ids(), [B, HW, HW, 4], 5., seed=3, preview_freq=Q,
                       on_preview=lambda i, a, b: seen.append((i, a, b, a.clone(), b.clone())))
  pv = s.last_previews()
  assert [v[0] for v in seen] == [9, 6, 3, 0]
  for i, a, b, a_then, b_then in seen:
    assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == tuple(b.shape) == (B, SCALE * HW, SCALE * HW, 3)
    for got in (a, a_then):
      assert np.array_equal(got.cpu().numpy(), pv["sample"][:, i // Q])
    for got in (b, b_then):
      assert np.array_equal(got.cpu().numpy(), pv["pred_x0"][:, i // Q])
  # the img2img loop from index 4: the callback sees 3 and 0
  img, E, _ = _img_inputs()
  seen = []
  s.ddim_p_sample_loop_img2img(_ids(), img, 5., strength=0.5, encode_noise=E, seed=3, preview_freq=Q,
                               on_preview=lambda i, a, b: seen.append(i))
  assert seen == [3, 0]


def test_fit_preview(dev, unet_w, txt_w, kl_w):
  s = _sampler(dev, unet_w, txt_w, kl_w, preview=False)
  proj = s.fit_preview(n=4, shape=(HW, HW, 4))
  assert proj.dtype == np.float32 and proj.shape == (5, 3) and np.isfinite(proj).all()
  assert s._pv_scale == 8 and np.array_equal(s._pv_host, proj)      # the autoencoder's factor by default
  assert not np.array_equal(proj, s.fit_preview(n=4, seed=1, shape=(HW, HW, 4)))
  s.set_preview(proj)
  images = s.ddim_p_sample_loop(_ids(), [B, HW, HW, 4], 5., seed=3, preview_freq=5)
  pv = s.last_previews()
  assert pv["sample"].shape == (B, 2, 8 * HW, 8 * HW, 3) == (B, 2) + tuple(images.shape[1:])
  assert np.array_equal(pv["indices"], [0, 5]) and pv["written"].all()
  # with no shape given: the last loop's
  assert s.fit_preview(n=2).shape == (5, 3)
  # given latents: the decoder's images of them are what the fit sees
  from ldm_tf2_amd.model_runners import fit_latent_preview
  lat = s._xt.clone()
  want = fit_latent_preview(lat, s.decode_first_stage(lat))
  assert np.array_equal(s.fit_preview(latents=lat), want)


# ---- CLI -----------------------------------------------------------------------------------------------
def test_cli_writes_previews(dev, tmp_path):
  import yaml
  from ldm_tf2_amd import run_ldm_sampler as R
  unet = dict(model_channels=64, out_channels=4, num_blocks=2, attention_resolutions=[4, 2, 1], dropout_rate=0.1,
              channel_mult=[1, 2, 4, 4], num_heads=8)
  txt = dict(vocab_size=200, encoder_stack_size=2, hidden_size=128, num_heads=4, size_per_head=32,
             max_seq_len=77, filter_size=256, dropout_rate=0.1)
  kl = dict(latent_channels=4, channels=64, num_blocks=2, attention_resolutions=[], dropout_rate=0.,
            multipliers=[1, 2, 4, 4], resample_with_conv=True)
  words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "painting", "of", "virus", "monster", "play", "##ing", "guitar"]
  words += [f"tok{i}" for i in range(200 - len(words))]
  (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n", encoding="utf-8")
  samp = {"autoencoder_type": "kl", "latent_shape": [2, 16, 16, 4], "guidance_scale": 5.0,
          "text_prompt": "a painting of a virus monster playing guitar", "vocab_dir": str(tmp_path),
          "sample_save_progress": False}
  cfg = {"ldm_sampling": samp, "pre_ckpt_paths": {"cond_stage_model": None, "unet": None, "autoencoder": None},
         "cond_stage_model": txt, "autoencoder_kl": kl, "unet": unet, "ldm": LDM}

  def run(name, **keys):
    out = tmp_path / name
    out.mkdir()
    path = out / "config.yaml"
    path.write_text(yaml.safe_dump(dict(cfg, ldm_sampling=dict(samp, **keys))))
    R.main(["--config_path", str(path), "--dtype", "f32", "--seed", "7", "--out", str(out / "images.npy")])
    return out

  plain = run("plain")
  assert not (plain / "preview_sample.npy").exists() and not (plain / "preview_x0.npy").exists()
  np.save(tmp_path / "m.npy", PROJ)
  given = run("given", preview_freq=4, preview_scale=2, preview_mode="nearest", preview_matrix=str(tmp_path / "m.npy"))
  assert np.array_equal(np.load(given / "images.npy"), np.load(plain / "images.npy"))
  a, b = np.load(given / "preview_sample.npy"), np.load(given / "preview_x0.npy")
  assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == (2, 3, 32, 32, 3)          # R = 9 // 4 + 1
  assert (a != 0).any(axis=(0, 2, 3, 4)).all() and not np.array_equal(a, b)
  assert np.array_equal(a[:, :, ::2, ::2], a[:, :, 1::2, 1::2])                              # nearest, scale 2
  fitted = run("fitted", preview_freq=5)                                                     # fit_preview, scale 8
  assert np.array_equal(np.load(fitted / "images.npy"), np.load(plain / "images.npy"))
  assert np.load(fitted / "preview_sample.npy").shape == (2, 2, 128, 128, 3)
