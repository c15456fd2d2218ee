"""Restatement of two-pass high-resolution sampling, NumPy, no GPU.

Resize of an NHWC array, per axis with source extent L, output extent Lo and output index i (align_corners=False, no
antialiasing):
  nearest:  the source index min((i * L) // Lo, L - 1);
  bilinear: s = max((i + 0.5) L / Lo - 0.5, 0), i0 = floor(s), f = s - i0; taps min(i0, L-1), min(i0+1, L-1), weights
            1 - f, f;
  bicubic:  s = (i + 0.5) L / Lo - 0.5, i0 = floor(s), f = s - i0; taps clamp(i0-1 .. i0+2, 0, L-1), weights Keys'
            kernel (a = -0.75) at the distances f + 1, f, 1 - f, 2 - f;
the 2-D result the sum over the tap grid of wy * wx * x.  `resize64` is that in float64, from the rules as written.
`resize32` is a float32 emulation of the same formula in the order the device kernel documents (include/ldm_hip.h):
its error against `resize64` is what float32 costs, the tests' gate.

The two-pass loop, composed from the oracle as tests/test_img2img_gpu.py composes img2img: N DDIM steps at the first
shape, the resize of the latents, q_sample to the level of steps[k-1], DDIM indices k-1 .. 0 at the second shape,
decode."""
import numpy as np
import torch

MODES = ("nearest", "bilinear", "bicubic")
A = -0.75


def keys(d):
  """Keys' cubic convolution kernel with a = -0.75 at the distance d >= 0 (float64)."""
  d = np.abs(np.asarray(d, dtype=np.float64))
  near = (A + 2.) * d ** 3 - (A + 3.) * d ** 2 + 1.
  far = A * d ** 3 - 5. * A * d ** 2 + 8. * A * d - 4. * A
  return np.where(d <= 1., near, np.where(d < 2., far, 0.))


def axis_taps(L, Lo, mode):
  """(idx int [Lo, n], w float64 [Lo, n]) of one axis; n = 1, 2, 4."""
  i = np.arange(Lo)
  if mode == "nearest":
    return np.minimum((i * L) // Lo, L - 1)[:, None], np.ones((Lo, 1))
  s = (i + 0.5) * L / Lo - 0.5
  if mode == "bilinear":
    s = np.maximum(s, 0.)
    i0 = np.floor(s).astype(np.int64)
    f = s - i0
    return np.stack([np.minimum(i0, L - 1), np.minimum(i0 + 1, L - 1)], 1), np.stack([1. - f, f], 1)
  if mode == "bicubic":
    i0 = np.floor(s).astype(np.int64)
    f = s - i0
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None], 0, L - 1)
    return idx, np.stack([keys(f + 1.), keys(f), keys(1. - f), keys(2. - f)], 1)
  raise ValueError(mode)


def resize64(x, size, mode):
  """x [B,H,W,c] -> float64 [B,Ho,Wo,c]."""
  x = np.asarray(x, dtype=np.float64)
  _, H, W, _ = x.shape
  if mode == "nearest" or (H, W) == tuple(size):
    # a copy of the source values, the sign of a zero included (at the same size every mode's source coordinate is
    # the output index and its weights are 1, 0 ..)
    return x[:, axis_taps(H, size[0], "nearest")[0][:, 0]][:, :, axis_taps(W, size[1], "nearest")[0][:, 0]]
  (iy, wy), (ix, wx) = axis_taps(H, size[0], mode), axis_taps(W, size[1], mode)
  out = np.zeros((x.shape[0], size[0], size[1], x.shape[3]))
  for a in range(iy.shape[1]):
    for b in range(ix.shape[1]):
      out += (wy[:, a, None] * wx[None, :, b])[None, :, :, None] * x[:, iy[:, a]][:, :, ix[:, b]]
  return out


def _axis_taps32(L, Lo, mode):
  """float32 weights as the kernel forms them: s = ((2i+1) L - Lo) / (2 Lo) with an integer floor and ONE rounded
  division for the fraction; Keys' inner polynomial in Horner form, the outer one in its factors a (d-1) (d-2)^2."""
  f32 = np.float32
  i = np.arange(Lo, dtype=np.int64)
  num, den = (2 * i + 1) * L - Lo, 2 * Lo
  i0 = num // den
  f = ((num - i0 * den).astype(f32) / f32(den)).astype(f32)
  if mode == "bilinear":
    f = np.where(num < 0, f32(0), f)
    i0 = np.where(num < 0, 0, i0)
    return np.stack([np.minimum(i0, L - 1), np.minimum(i0 + 1, L - 1)], 1), np.stack([f32(1) - f, f], 1)
  near = lambda d: (f32(1.25) * d - f32(2.25)) * d * d + f32(1)
  far = lambda dm1, dm2: f32(-0.75) * dm1 * (dm2 * dm2)            # a (d - 1) (d - 2)^2
  g = f32(1) - f
  idx = np.clip(i0[:, None] + np.arange(-1, 3)[None], 0, L - 1)
  return idx, np.stack([far(f, g), near(f), near(g), far(g, f)], 1).astype(f32)


def resize32(x, size, mode):
  """The float32 emulation (bilinear, bicubic): every product and sum rounded to float32, rows outermost."""
  x = np.asarray(x, dtype=np.float32)
  _, H, W, _ = x.shape
  (iy, wy), (ix, wx) = _axis_taps32(H, size[0], mode), _axis_taps32(W, size[1], mode)
  out = np.zeros((x.shape[0], size[0], size[1], x.shape[3]), dtype=np.float32)
  for a in range(iy.shape[1]):
    for b in range(ix.shape[1]):
      w = (wy[:, a, None] * wx[None, :, b]).astype(np.float32)
      out = (out + (w[None, :, :, None] * x[:, iy[:, a]][:, :, ix[:, b]]).astype(np.float32)).astype(np.float32)
  return out


def q_sample(ac, x0, t, eps, dtype=torch.float32):
  """model_runners.py:580-600: the float64 tables cast to float32, gathered, then widened to `dtype`."""
  sa = torch.from_numpy(np.sqrt(ac).astype(np.float32)[np.asarray(t)]).reshape(-1, 1, 1, 1).to(dtype)
  sb = torch.from_numpy(np.sqrt(1. - ac).astype(np.float32)[np.asarray(t)]).reshape(-1, 1, 1, 1).to(dtype)
  return sa * torch.as_tensor(x0).to(dtype) + sb * torch.as_tensor(eps).to(dtype)


def sdedit_loop(O, context, z0, w, ldm, k, Q, gs=5., dtype=torch.float32, record=None):
  """The unmasked img2img loop from the latents z0: q_sample to steps[k-1] with Q[k-1], DDIM indices k-1 .. 0."""
  sched = O.make_schedule(ldm["num_steps"], ldm["beta_start"], ldm["beta_end"], ldm["eta"], ldm["num_ddim_steps"])
  x = q_sample(sched["alphas_cumprod"], z0, [sched["ddim_steps"][k - 1]] * z0.shape[0], Q[k - 1], dtype)
  for i in range(k - 1, -1, -1):
    x, _, _ = O.ddim_sample(x, context, i, sched, w["unet"], gs, None, dtype, clip_denoised=False)
    if record is not None:
      record.append(x.clone())
  return x


def hires_loop(O, ids, x_T, w, ldm, k, size, mode, Q, gs=5., dtype=torch.float32):
  """-> (images, latents of pass 1, z0, latents of pass 2), eta = 0."""
  sched = O.make_schedule(ldm["num_steps"], ldm["beta_start"], ldm["beta_end"], ldm["eta"], ldm["num_ddim_steps"])
  context = O.text_encoder(ids, w["cond_stage_model"], dtype)
  x = torch.as_tensor(x_T).to(dtype)
  for i in range(len(sched["ddim_steps"]) - 1, -1, -1):
    x, _, _ = O.ddim_sample(x, context, i, sched, w["unet"], gs, None, dtype, clip_denoised=False)
  z0 = torch.from_numpy(resize64(x.numpy(), size, mode)).to(dtype)
  x2 = sdedit_loop(O, context, z0, w, ldm, k, Q, gs, dtype)
  images = O.decoder_forward(x2 / ldm["scale_factor"], w["autoencoder"], dtype)
  return images, x, z0, x2
