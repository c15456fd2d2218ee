"""Init images and masks of any size, and pixel-space upscaling in the two-pass loop, on the GPU (DESIGN.md section
15).  Every check composes the same launches by hand on the same sampler -- crop, ops.resample_nhwc, then the loop of
today on the host copy of the result -- so both sides see identical inputs and are compared exactly, as
tests/test_hires_gpu.py compares its repeated calls.  The kernel itself is gated in tests/test_varsize_resample_gpu.py.
Tiny models, ids and LDM are those of tests/test_img2img_gpu.py: B = 2, N = 10, 128 x 128 images, 16 x 16 latents."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd.model_runners import hires_seed, img2img_start, latent_mask_fit  # noqa: E402
from ldm_tf2_amd.resample import crop_box  # noqa: E402

B, N, HW = T.B, T.N, T.HW
SIZE = (8 * HW, 8 * HW)                          # what the tiny autoencoder and U-Net were built for
SRC = (40, 56)
GS, STRENGTH = 5., 0.5
LO, HI = [B, 16, 16, 4], [B, 32, 32, 4]


@pytest.fixture(scope="module")
def sampler(dev, unet_w, txt_w, kl_w):
  return T._sampler(dev, torch.float32, unet_w, txt_w, kl_w)


def _inputs():
  g = np.random.default_rng(41)
  mask = np.ones((B,) + SRC, dtype=np.float32)
  mask[:, 10:30, 20:44] = 0.                      # regenerate a box that straddles latent cells
  return dict(img=(g.random((B,) + SRC + (3,), dtype=np.float32) * 2 - 1).astype(np.float32),
              E=g.standard_normal((B, HW, HW, 4)).astype(np.float32),
              Q=g.standard_normal((N, B, HW, HW, 4)).astype(np.float32), mask=mask,
              x_T=g.standard_normal(tuple(LO)).astype(np.float32),
              E_hi=g.standard_normal(tuple(HI)).astype(np.float32),
              Q_hi=g.standard_normal((N,) + tuple(HI)).astype(np.float32))


def _fitted(dev, img, fit, name):
  """crop (when asked) and ops.resample_nhwc by hand -> the host copy."""
  x = torch.from_numpy(img).to(dev)
  if fit == "crop":
    y0, x0, hc, wc = crop_box(SRC, SIZE)
    assert (y0, x0, hc, wc) == (0, 8, 40, 40)
    x = x[:, y0:y0 + hc, x0:x0 + wc].contiguous()
  return ops.resample_nhwc(x, SIZE, name).cpu()


@pytest.mark.parametrize("fit", ["stretch", "crop"])
def test_img2img_resamples_its_init_images(dev, sampler, fit):
  t, ids, s = _inputs(), T._ids(), sampler
  kw = dict(strength=STRENGTH, encode_noise=t["E"], q_noises=t["Q"])
  got = s.ddim_p_sample_loop_img2img(ids, t["img"], GS, image_size=SIZE, fit=fit, resample="lanczos3", **kw)
  lat = s._xt.clone()
  pre = _fitted(dev, t["img"], fit, "lanczos3")
  assert tuple(pre.shape) == (B,) + SIZE + (3,)
  want = s.ddim_p_sample_loop_img2img(ids, pre, GS, **kw)
  assert torch.equal(got, want) and torch.equal(lat, s._xt)
  assert tuple(got.shape) == (B,) + SIZE + (3,) and torch.isfinite(got).all()
  if fit == "stretch":                            # one image [H,W,3] is tiled
    one = s.ddim_p_sample_loop_img2img(ids, t["img"][0], GS, image_size=SIZE, fit=fit, **kw)
    assert torch.equal(one[0], got[0])


@pytest.mark.parametrize("fit", ["stretch", "crop"])
def test_pixel_mask_at_the_source_size(dev, sampler, fit):
  t, ids, s = _inputs(), T._ids(), sampler
  kw = dict(strength=STRENGTH, encode_noise=t["E"], q_noises=t["Q"])
  got = s.ddim_p_sample_loop_img2img(ids, t["img"], GS, mask=t["mask"], image_size=SIZE, fit=fit, **kw)
  m = t["mask"]
  if fit == "crop":
    y0, x0, hc, wc = crop_box(SRC, SIZE)
    m = m[:, y0:y0 + hc, x0:x0 + wc]
  lm = latent_mask_fit(m, (HW, HW))
  assert 0 < lm.sum() < lm.size
  pre = _fitted(dev, t["img"], fit, "lanczos3")
  assert torch.equal(got, s.ddim_p_sample_loop_img2img(ids, pre, GS, mask=lm, **kw))
  if fit == "stretch":                            # a mask at latent resolution keeps working next to image_size
    assert torch.equal(got, s.ddim_p_sample_loop_img2img(ids, t["img"], GS, mask=lm, image_size=SIZE, fit=fit, **kw))
  else:                                           # one [Hs,Ws] mask is tiled
    assert torch.equal(got, s.ddim_p_sample_loop_img2img(ids, t["img"], GS, mask=t["mask"][0], image_size=SIZE,
                                                         fit=fit, **kw))
    with pytest.raises(ValueError, match="neither a latent mask"):
      s.ddim_p_sample_loop_img2img(ids, t["img"], GS, mask=np.ones((B, 40, 40)), image_size=SIZE, fit=fit, **kw)


def test_invert_and_edit_resample_their_init_images(dev, sampler):
  t, ids, s = _inputs(), T._ids(), sampler
  k = img2img_start(STRENGTH, N)
  pre = _fitted(dev, t["img"], "crop", "cubic")
  got = s.ddim_invert_loop(ids, init_images=t["img"], strength=STRENGTH, encode_noise=t["E"], image_size=SIZE,
                           fit="crop", resample="cubic")
  want = s.ddim_invert_loop(ids, init_images=pre, strength=STRENGTH, encode_noise=t["E"])
  assert torch.equal(got, want) and tuple(got.shape) == tuple(LO) and torch.isfinite(got).all()
  tgt = ids.copy()
  tgt[B:, 1:5] = (tgt[B:, 1:5] + 7) % 1000
  kw = dict(guidance_scale=GS, strength=STRENGTH, encode_noise=t["E"])
  got = s.ddim_p_sample_loop_edit(ids, tgt, t["img"], image_size=SIZE, fit="stretch", resample="cubic", **kw)
  want = s.ddim_p_sample_loop_edit(ids, tgt, _fitted(dev, t["img"], "stretch", "cubic"), **kw)
  assert torch.equal(got, want) and tuple(got.shape) == (B,) + SIZE + (3,) and k == 5


def test_an_image_already_at_image_size_takes_todays_path(dev, sampler, monkeypatch):
  ids, s = T._ids(), sampler
  img, E, Q, _, mask = T._inputs(0.)
  kw = dict(strength=STRENGTH, encode_noise=E, q_noises=Q)
  want = s.ddim_p_sample_loop_img2img(ids, img, GS, **kw)
  want_masked = s.ddim_p_sample_loop_img2img(ids, img, GS, mask=mask, **kw)
  calls = []
  monkeypatch.setattr(ops, "resample_nhwc", lambda *a, **k_: calls.append(a) or pytest.fail("resampled"))
  assert torch.equal(s.ddim_p_sample_loop_img2img(ids, img, GS, image_size=SIZE, fit="stretch", **kw), want)
  assert torch.equal(s.ddim_p_sample_loop_img2img(ids, img, GS, mask=mask, image_size=SIZE, fit="crop", **kw),
                     want_masked)
  pixel = np.repeat(np.repeat(mask, 8, axis=1), 8, axis=2)      # the same mask at 128 x 128: latent_mask's rule
  assert torch.equal(s.ddim_p_sample_loop_img2img(ids, img, GS, mask=pixel, image_size=SIZE, **kw), want_masked)
  assert not calls


def test_hires_in_pixel_space_is_the_hand_chained_sequence(dev, sampler):
  """16 x 16 -> 32 x 32 latents through 128 x 128 -> 256 x 256 pixels: ddim_p_sample_loop without the decode, decode,
  ops.resample_nhwc, get_latents(encode_noise), the img2img tail.  A second call captures no new graph."""
  t, ids, s = _inputs(), T._ids(), sampler
  k = img2img_start(STRENGTH, N)
  kw = dict(strength=STRENGTH, guidance_scale=GS, x_T=t["x_T"], q_noises=t["Q_hi"], pixel_filter="cubic")
  got = s.ddim_p_sample_loop_hires(ids, LO, HI, encode_noise=t["E_hi"], **kw)
  lat, first = s._xt.clone(), s.hires_first_latents.clone()
  assert tuple(got.shape) == (B, 256, 256, 3) and torch.isfinite(got).all() and s._state_key == tuple(HI)
  g_hi, g_lo = s._graph, s._states[tuple(LO)]["_graph"]
  assert g_hi is not None and g_lo is not None and g_hi is not g_lo
  # the hand-chained sequence, on the same sampler with the same tables
  s.ddim_p_sample_loop(ids, LO, GS, x_T=t["x_T"])
  assert torch.equal(s._xt, first)
  image = s.decode_first_stage(s._xt.clone())
  assert tuple(image.shape) == (B,) + SIZE + (3,) and image.dtype == torch.float32
  big = ops.resample_nhwc(image, (256, 256), "cubic")
  z0 = s.get_latents(big, noise=t["E_hi"])
  assert tuple(z0.shape) == tuple(HI)
  want = s._sdedit(s._cond_stage_model(ids), z0, k, GS, None, None, t["Q_hi"], None, hires_seed(0), 0, None)
  assert torch.equal(want, got) and torch.equal(s._xt, lat)
  assert s._graph is g_hi and s._states[tuple(LO)]["_graph"] is g_lo
  # a second call captures nothing; without encode_noise the encode draws under hires_seed(seed)
  drawn = s.ddim_p_sample_loop_hires(ids, LO, HI, seed=3, **kw)
  assert s._graph is g_hi and s._states[tuple(LO)]["_graph"] is g_lo and not torch.equal(drawn, got)
  z0 = s.get_latents(big, seed=hires_seed(3))
  assert torch.equal(drawn, s._sdedit(s._cond_stage_model(ids), z0, k, GS, None, None, t["Q_hi"], None, hires_seed(3),
                                      0, None))
  assert s._graph is g_hi
