"""DDIM sampler with classifier-free guidance on the HIP path -- host side.

Mirrors `LatentDiffusionModel` / `LatentDiffusionModelSampler`
(model_runners.py:352-509): same constructor kwargs (the YAML `ldm` section), the
same three public methods, the three models treated as opaque callables with the
contracts of SURVEY.md section 8b.  The reference draws x_T and the per-step noise
from an unseeded tf.random.normal (:466,:478); here they are explicit inputs (or
derived from `seed`), which is what makes parity checkable.

Host (this file, float64/float32 NumPy): the schedule tables -- built once, exactly
as model_runners.py:379-423 builds them.  Device (HIP kernels via ops): everything
inside the loop.  One DDIM step = one U-Net forward on [xt; xt] + one fused
CFG/DDIM-update kernel that reads its coefficients from a device table at a
device-resident index and decrements it, so a step has no host-side scalars and
the whole step can be captured once in a HIP graph and replayed N times.

img2img / inpainting run the same step from an intermediate DDIM
index: the start latent is the forward diffusion (q_sample, the reference trainer's
:580-600) of the encoded init image, and a mask pins kept latent cells to it inside the
step's one update launch.

sampler="plms"  swaps that update for the PLMS one: the same launch count, a ring of the last
four guided eps and the loop's start index on the device, the same captured graph for any start index.

noise_source="device"  draws every random number of the loops on the device: Philox4x32-10 keyed
by the seed, counted by (element, global sample index, stream), formed in registers inside the step's update launch.
No noise table is built or uploaded, and one captured graph serves any seed.

step_spacing= / ddim_steps= choose the integer timesteps the loops walk: the reference's uniform
table (default), N timesteps evenly spaced in lambda = half the log signal-to-noise ratio ("logsnr"), Karras et al.'s
rho = 7 spacing in sigma ("karras"), or a table handed in.  Every derived table is built from the chosen one.
sampler="deis" is the PLMS step with its weights computed for the table actually walked: a float32 device table
[N][4][4] read by the one update launch.

guidance_scale=[g_0 .. g_{N-1}] / guidance_interval=(t_lo, t_hi) give every DDIM index its own
guidance scale: a float32 device table read by the one update launch (ldm_cfg_sched_update), so no scale is frozen
into a captured graph.  A step whose scale is exactly 1 is unguided: its eps is the conditional one by definition,
and the U-Net runs on the conditional rows alone against the resident context.  A loop replays one of two captured
graphs per step.  eta must be 0 there; a float scale without an interval takes the path above unchanged.

ddim_p_sample_loop_panorama samples a canvas wider than the U-Net's training size: every step
crops the canvas into overlapping training-size windows (ldm_window_gather), runs the U-Net on the window rows,
averages the windows' eps back onto the canvas (ldm_window_fold) and runs the configured solver's one update launch
on the canvas.  The updates are affine in eps, so that equals averaging the windows' step outputs (MultiDiffusion).
With `wrap` the windows of an axis cross the edge and come back on the other side, with `window_weights` the average
is weighted by a window profile (ldm_window_gather_ex, ldm_window_fold_ex), and `wrap_decode_margin` decodes the canvas
behind a circular margin (ldm_wrap_pad_nhwc) that is cropped from the images.

ddim_invert_loop runs the deterministic DDIM step upwards from the latents of an image: a U-Net
evaluation at the level the input is on and one update launch (ldm_cfg_ddim_invert_update) per step, replayed from a
captured graph of its own.  ddim_p_sample_loop(x_T=, start_index=k) samples from the level it reached, and
ddim_p_sample_loop_edit chains the two: inversion under a source prompt, sampling under a target prompt.

ddim_p_sample_loop_hires samples at the U-Net's training size, resizes the latents on the device
(ldm_resize_nhwc) and re-runs the last int(strength * N) DDIM indices at the larger size, the unmasked img2img loop
without an encoder.  The sampler keeps the device state and the captured graphs of every latent shape it has run
(_alloc_state), so the two passes of a call, and later calls, replay two graphs captured once.

image_size= / fit= / resample= on the image-driven loops, and pixel_filter= on the two-pass loop
bring init images, pixel masks and pass 1's decoded image to the size the models need with the antialiased resample
(ldm_resample_nhwc, tables from resample.py) on the device, next to the encoder.

preview_freq= / on_preview= on ddim_p_sample_loop and ddim_p_sample_loop_img2img record small
RGB pictures of x_t and of the predicted x_0 every q DDIM indices: the step's update also writes pred_x0 and one
ldm_latent_preview launch inside the captured step maps both through the matrix of set_preview / fit_preview, enlarges
and quantises them into the slot the device-resident index selects.  Those steps are captured in graph slots of their
own; without the keyword every key, launch and graph is the one it was.

ddim_p_sample_loop_diffedit keeps the prompt edit inside a mask: diffedit_mask replays one
captured contrast step per noise draw (ldm_q_sample by table row, the paired U-Net call against the two prompts'
conditional contexts, ldm_eps_contrast_accum) and thresholds the map on the device (ldm_contrast_mask);
ddim_invert_loop(trajectory=True) stores every inversion level with one ldm_store_row launch inside its captured step;
the sampling loop's masked blend then reads that trajectory where the img2img loop reads q_sample(z0, Q).  Three graph
slots of their own; without the keywords every key, launch and graph is the one it was.

ddim_p_sample_loop_outpaint and masked_content="fill" on ddim_p_sample_loop_img2img choose what
a regenerated region starts from: the image the encoder sees gets that region -- the new border of an outpainted
canvas, or the mask's hole -- filled with a smooth continuation of the kept pixels by a push-pull image pyramid
(ldm_pushpull_fill), one eager call in front of the encoder.  The loop behind it is the masked img2img loop as it is:
no new graph, slot or state.

paste_back= / mask_feather= / color_match= on ddim_p_sample_loop_img2img and ddim_p_sample_loop_outpaint (DESIGN.md
section 22) put the init images' own pixels back after the decode wherever the mask keeps them: a feathered weight map
(ldm_mask_feather), optionally the gain and offset that match the decoded image to the originals on the kept pixels
(ldm_keep_stats), and the blend (ldm_paste_back) -- three eager calls after decode_first_stage, nothing inside the
captured step; without the keywords every call and bit is the one it was.
"""
from __future__ import annotations

import itertools
import sys

import numpy as np
import torch

from . import ops
from ._lib import LdmHipError
from .autoencoder import AutoencoderKL, AutoencoderVQ
from .resample import check_filter, crop_box


def _tf_linspace_f32(start, stop, num):
  """tf.linspace on float32 operands [TF-mem]: exact endpoints, interior
  start + delta*i with float32 delta = (stop-start)/(num-1)."""
  start, stop = np.float32(start), np.float32(stop)
  delta = np.float32((stop - start) / np.float32(num - 1))
  inner = (start + delta * np.arange(1, num - 1, dtype=np.float32)).astype(np.float32)
  return np.concatenate([[start], inner, [stop]]).astype(np.float32)


def _extract(data, t):
  """model_runners.py:28-45: cast to float32 THEN gather; shape [-1,1,1,1]."""
  return np.asarray(data).astype(np.float32)[np.asarray(t)].reshape(-1, 1, 1, 1)


def _as_tensor(x, dtype=torch.float32):
  """A caller's array (a tensor, a NumPy array or nested numbers) as a tensor of `dtype` (None: its own), where it is."""
  return torch.as_tensor(x if isinstance(x, torch.Tensor) else np.asarray(x), dtype=dtype)


def normal_latents(seed, first_index, count, shape_hwc, stream=None):
  """x_T ~ N(0,1): sample i of a run is drawn from its own generator keyed by
  (seed, global sample index), so a sample's trajectory does not depend on how
  samples are spread over GPUs.  `stream` (an int) keys a third entropy word: the
  img2img draws (ENCODE_STREAM, Q_STREAM + i) never share a generator with the x_T
  stream (seed) or the eta-noise streams (seed + 1 + i), which have two words."""
  out = np.empty((count,) + tuple(shape_hwc), dtype=np.float32)
  for i in range(count):
    key = [int(seed), int(first_index) + i] + ([] if stream is None else [int(stream)])
    g = np.random.default_rng(key)
    out[i] = g.standard_normal(shape_hwc, dtype=np.float32)
  return out


ENCODE_STREAM = 1 << 30          # posterior noise E of get_latents
Q_STREAM = (1 << 30) + 1         # + i: forward-diffusion noise Q[i] of DDIM index i
PREVIEW_FIT_STREAM = 1 << 31     # the stand-in latents of fit_preview (above Q_STREAM + i for every i < 2^30)
MAP_STREAM = 3 << 29             # + r: draw r of DiffEdit's contrast map (above Q_STREAM + i for i < 2^29 - 1, below 2^31)
# noise_source="device" only (the host draws key x_T and the eta noise by the seed word, see normal_latents): the
# stream word is the third counter word of the device generator; the four ranges are disjoint for i < 2^29.
XT_STREAM = 0                    # x_T
ETA_STREAM = 1 << 29             # + i: eta noise of the step at DDIM index i
NOISE_SOURCES = ("host", "device")
RESIZE_MODES = ("nearest", "bilinear", "bicubic")
FITS = ("stretch", "crop")       # image_size=: the whole source, or its centred box of the target's aspect ratio


def hires_seed(seed):
  """The seed of everything the second pass of ddim_p_sample_loop_hires draws: `seed` mod 2^64
  with bit 63 flipped.  It is a 64-bit value that differs from `seed` by at least 2^63, so on the host no generator key
  of the second pass ((s', index, Q_STREAM + i) and (s' + 1 + i, index), i < N) equals one of the first ((seed, index)
  and (seed + 1 + i, index)), and on the device the two passes run under different Philox keys."""
  return (int(seed) % (1 << 64)) ^ (1 << 63)
STEP_SPACINGS = ("uniform", "logsnr", "karras")
KARRAS_RHO = 7.


def log_snr_half(alphas_cumprod):
  """lambda(t) = 0.5 * ln(abar[t] / (1 - abar[t])), float64: it falls as t rises."""
  ac = np.asarray(alphas_cumprod, dtype=np.float64)
  return 0.5 * np.log(ac / (1. - ac))


def spaced_steps(alphas_cumprod, num_ddim_steps, top, spacing):
  """The "logsnr" / "karras" step table: num_ddim_steps targets evenly spaced in lambda, or in
  sigma^(1/rho) with sigma = sqrt((1 - abar) / abar), between timestep 0 (exclusive) and `top` (inclusive); each
  target becomes the integer timestep with the nearest lambda, at least 1 and above its predecessor; the last one
  is `top`.  int32, ascending."""
  ac = np.asarray(alphas_cumprod, dtype=np.float64)
  lam = log_snr_half(ac)
  n = int(num_ddim_steps)
  if spacing == "logsnr":
    targets = np.linspace(lam[0], lam[top], n + 1)[1:]
  elif spacing == "karras":
    sigma = np.sqrt((1. - ac) / ac)
    targets = -np.log(np.linspace(sigma[0] ** (1. / KARRAS_RHO), sigma[top] ** (1. / KARRAS_RHO), n + 1)[1:]
                      ** KARRAS_RHO)
  else:
    raise ValueError(f"step_spacing must be one of {STEP_SPACINGS}, got {spacing!r}")
  steps = np.empty(n, dtype=np.int32)
  for j, target in enumerate(targets):
    t = max(int(np.argmin(np.abs(lam - target))), 1)
    steps[j] = t if j == 0 else max(t, steps[j - 1] + 1)
  steps[-1] = top
  return steps


def check_steps(steps, num_steps, num_ddim_steps):
  """A step table as int32: strictly ascending timesteps in [1, num_steps - 1], num_ddim_steps of them."""
  arr = np.asarray(steps)
  if arr.ndim != 1 or arr.size == 0 or not np.issubdtype(arr.dtype, np.integer):
    raise ValueError(f"ddim_steps must be a non-empty 1-D sequence of ints, got {steps!r}")
  if arr.size != num_ddim_steps:
    raise ValueError(f"ddim_steps has {arr.size} entries, num_ddim_steps is {num_ddim_steps}")
  if arr.min() < 1 or arr.max() > num_steps - 1:
    raise ValueError(f"ddim_steps must lie in [1, {num_steps - 1}], got [{int(arr.min())}, {int(arr.max())}]")
  if np.any(np.diff(arr.astype(np.int64)) <= 0):
    raise ValueError("ddim_steps must be strictly ascending")
  return arr.astype(np.int32)


def img2img_start(strength, num_ddim_steps):
  """k = int(strength * N) (CompVis's t_enc): the loop runs DDIM indices k-1 .. 0."""
  strength = float(strength)
  if not 0. < strength <= 1.:
    raise ValueError(f"strength must be in (0, 1], got {strength}")
  k = int(strength * num_ddim_steps)
  if k < 1:
    raise ValueError(f"strength {strength} runs int({strength} * {num_ddim_steps}) = 0 DDIM steps")
  return k


def latent_mask(pixel_mask, f):
  """Pixel mask [B,H,W] (or [H,W]; nonzero = keep) -> float32 [B,H/f,W/f] by a min-pool over
  each f x f cell: a latent cell is kept only if all its pixels are, so every pixel marked for
  regeneration is regenerated."""
  m = np.asarray(pixel_mask.cpu() if isinstance(pixel_mask, torch.Tensor) else pixel_mask)
  if m.ndim == 2:
    m = m[None]
  if m.ndim != 3 or m.shape[1] % f or m.shape[2] % f:
    raise ValueError(f"pixel mask of shape {m.shape} is not [B,H,W] with H, W multiples of {f}")
  B, H, W = m.shape
  keep = (m != 0).reshape(B, H // f, f, W // f, f).all(axis=(2, 4))
  return keep.astype(np.float32)


def latent_mask_fit(pixel_mask, size):
  """Pixel mask [B,Hs,Ws] (or [Hs,Ws]; nonzero = keep) of any extents -> float32 [B,h,w], `size` = (h, w) (DESIGN.md
  section 15).  Latent cell y covers the source rows floor(y Hs / h) .. ceil((y + 1) Hs / h) - 1, every row any part
  of which falls into the cell, in integer arithmetic; columns alike.  A cell is kept only if all the pixels it
  covers are, so every pixel marked for regeneration is regenerated.  At Hs = f h, Ws = f w this is latent_mask."""
  m = np.asarray(pixel_mask.cpu() if isinstance(pixel_mask, torch.Tensor) else pixel_mask)
  if m.ndim == 2:
    m = m[None]
  h, w = (int(v) for v in size)
  if m.ndim != 3 or min(m.shape[1:]) < 1 or h < 1 or w < 1:
    raise ValueError(f"pixel mask of shape {m.shape} is not a non-empty [B,H,W], or the latent size {(h, w)} is empty")
  B, Hs, Ws = m.shape
  keep = m != 0
  rows = np.empty((B, h, Ws), dtype=bool)
  for y in range(h):
    rows[:, y] = keep[:, (y * Hs) // h:-((-(y + 1) * Hs) // h)].all(axis=1)
  out = np.empty((B, h, w), dtype=bool)
  for x in range(w):
    out[:, :, x] = rows[:, :, (x * Ws) // w:-((-(x + 1) * Ws) // w)].all(axis=2)
  return out.astype(np.float32)


MASKED_CONTENTS = ("original", "fill")   # what a regenerated region starts from


def fill_keep_mask(mask, src, size, f, fit="stretch"):
  """The keep weights float32 [B,H,W] (B = 1 for a 2-D mask) that masked_content="fill" hands ops.pushpull_fill with
  the images [B,H,W,3] the encoder sees, `size` = (H, W).  `mask` is the img2img loop's:
    a latent mask [B,H/f,W/f] (or [H/f,W/f]): every cell's value repeated over its f x f pixels;
    a pixel mask at the source images' extents `src` ([B,Hs,Ws] or [Hs,Ws], nonzero = keep): brought to the canvas the
      way the images are -- with `fit` "crop" the same centred box (resample.crop_box) -- and canvas pixel y covers
      the source rows floor(y Hs / H) .. ceil((y + 1) Hs / H) - 1, columns alike (latent_mask_fit's rule at pixel
      resolution): the weight is 1 exactly where every source pixel the canvas pixel covers is kept, else 0.
  Any other shape is a ValueError."""
  H, W = (int(v) for v in size)
  src = tuple(int(v) for v in src)
  if H % f or W % f:
    raise ValueError(f"the filled canvas {(H, W)} must have extents that are multiples of {f}")
  h, w = H // f, W // f
  m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask)
  shape = m.shape
  if m.ndim == 2:
    m = m[None]
  if m.ndim == 3 and m.shape[1:] == (h, w):
    return np.repeat(np.repeat(m.astype(np.float32), f, axis=1), f, axis=2)
  if m.ndim != 3 or m.shape[1:] != src:
    raise ValueError(f"mask of shape {shape} is neither a latent mask [B,{h},{w}] (or [{h},{w}]) nor a pixel mask "
                     f"at the init images' size [B,{src[0]},{src[1]}] (or [{src[0]},{src[1]}])")
  if fit == "crop" and src != (H, W):
    y0, x0, hc, wc = crop_box(src, (H, W))
    m = m[:, y0:y0 + hc, x0:x0 + wc]
  return latent_mask_fit(m, (H, W))


def outpaint_geometry(image_hw, pad, f, div=1):
  """Outpainting's canvas: an image of `image_hw` = (H, W) pixels grows by `pad` = (top,
  bottom, left, right) pixels, each at least 0 and not all 0.  Returns ((Hc, Wc), (y0, x0, H, W)): the canvas size and
  the box the image takes on it.  Both canvas extents must be positive multiples of f * div (`f` the autoencoder's
  pixels per latent cell, `div` = 2^levels for a U-Net that halves its input `levels` times): ValueError otherwise."""
  if np.ndim(image_hw) != 1 or len(image_hw) != 2 or any(int(v) != v or v < 1 for v in image_hw):
    raise ValueError(f"image_hw must be (H, W) in pixels, got {image_hw!r}")
  if np.ndim(pad) != 1 or len(pad) != 4 or any(isinstance(v, bool) or int(v) != v for v in pad):
    raise ValueError(f"pad must be (top, bottom, left, right) in pixels, got {pad!r}")
  H, W = (int(v) for v in image_hw)
  top, bottom, left, right = (int(v) for v in pad)
  if min(top, bottom, left, right) < 0 or max(top, bottom, left, right) == 0:
    raise ValueError(f"pad {(top, bottom, left, right)}: every side must be at least 0 and one of them positive")
  Hc, Wc = H + top + bottom, W + left + right
  f, div = int(f), int(div)
  if Hc % (f * div) or Wc % (f * div):
    raise ValueError(f"outpaint canvas {(Hc, Wc)}: the autoencoder maps {f} pixels to a latent cell and the U-Net halves "
                     f"its input {div.bit_length() - 1} times, the extents must be positive multiples of {f * div}")
  return (Hc, Wc), (top, left, H, W)


def window_origins(L, l, s):
  """Origins of the windows of extent l at stride s covering an axis of extent L:
  n = ceil((L - l) / s) + 1 windows, origin_i = min(i * s, L - l); the last one is clamped to the edge.  Needs
  1 <= l <= L and 1 <= s <= l (no gaps); strictly increasing."""
  L, l, s = int(L), int(l), int(s)
  if not 1 <= l <= L:
    raise ValueError(f"window extent {l} must lie in [1, {L}] (the canvas extent)")
  if not 1 <= s <= l:
    raise ValueError(f"window stride {s} must lie in [1, {l}] (the window extent): windows leave no gaps")
  n = -((l - L) // s) + 1
  return [min(i * s, L - l) for i in range(n)]


def wrap_origins(L, l, s):
  """Origins of the windows along a wrapped axis: n = ceil(L / s) windows at origin_i = i * s,
  no clamp; window i covers the cells (origin_i + j) mod L, j = 0 .. l - 1.  Needs 1 <= l <= L and 1 <= s <= l, as
  window_origins; the origins are distinct and below L, every cell is covered, and a window covers a cell once."""
  L, l, s = int(L), int(l), int(s)
  if not 1 <= l <= L:
    raise ValueError(f"window extent {l} must lie in [1, {L}] (the canvas extent)")
  if not 1 <= s <= l:
    raise ValueError(f"window stride {s} must lie in [1, {l}] (the window extent): windows leave no gaps")
  return [i * s for i in range(-(-L // s))]


WINDOW_WEIGHTS = ("uniform", "tent", "gaussian")


def window_profile(kind, l):
  """float32 [l]: the window profile `kind` along an axis of window extent l.  "uniform": ones;
  "tent": min(j + 1, l - j); "gaussian": exp(-(j - (l - 1) / 2)^2 / (2 (l / 4)^2)), computed in float64 and rounded.
  All positive and symmetric."""
  l = int(l)
  if l < 1:
    raise ValueError(f"window extent {l} must be at least 1")
  j = np.arange(l, dtype=np.float64)
  if kind == "uniform":
    p = np.ones(l)
  elif kind == "tent":
    p = np.minimum(j + 1, l - j)
  elif kind == "gaussian":
    p = np.exp(-(j - (l - 1) / 2.) ** 2 / (2. * (l / 4.) ** 2))
  else:
    raise ValueError(f"window_weights must be one of {WINDOW_WEIGHTS} or a pair of arrays (wy, wx), got {kind!r}")
  return p.astype(np.float32)


def window_weight_tables(window_weights, window):
  """(identity, tables) of the panorama loop's `window_weights` for `window` = (h, w): ("uniform", None) -- no
  tables, the plain mean -- or (name or "tables", (wy float32 [h], wx float32 [w])) for "tent", "gaussian" or a pair
  of positive finite arrays."""
  h, w = window
  if isinstance(window_weights, str):
    if window_weights == "uniform":
      return "uniform", None
    return window_weights, (window_profile(window_weights, h), window_profile(window_weights, w))
  if isinstance(window_weights, torch.Tensor) or not hasattr(window_weights, "__len__") or len(window_weights) != 2:
    raise ValueError(f"window_weights must be one of {WINDOW_WEIGHTS} or a pair of arrays (wy, wx)")
  tables = []
  for t, n, what in zip(window_weights, (h, w), ("wy", "wx")):
    t = np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64)
    if t.shape != (n,):
      raise ValueError(f"window_weights: {what} has shape {t.shape}, expected {(n,)}")
    with np.errstate(over="ignore"):
      t = t.astype(np.float32)
    if not (np.isfinite(t).all() and (t > 0).all()):
      raise ValueError(f"window_weights: {what} must be positive and finite in float32")
    tables.append(t)
  return "tables", tuple(tables)


def wrap_pair(wrap):
  """`wrap` = (wrap_y, wrap_x) of a panorama call as a pair of bools."""
  if np.ndim(wrap) != 1 or len(wrap) != 2 or any(not isinstance(v, (bool, np.bool_)) for v in wrap):
    raise ValueError(f"wrap must be a pair of bools (wrap_y, wrap_x), got {wrap!r}")
  return bool(wrap[0]), bool(wrap[1])


def window_and_stride(window, stride=None):
  """((h, w), (sy, sx)) of a panorama call: each argument one int (both axes) or a pair; `stride` None = half the
  window, rounded down, at least 1."""
  def pair(v, what):
    if np.ndim(v) == 0:
      v = (v, v)
    if np.ndim(v) != 1 or len(v) != 2 or any(int(x) != x for x in v):
      raise ValueError(f"{what} must be an int or a pair of ints, got {v!r}")
    return tuple(int(x) for x in v)
  h, w = pair(window, "window")
  if stride is None:
    stride = (max(h // 2, 1), max(w // 2, 1))
  return (h, w), pair(stride, "stride")


def guidance_table(steps, guidance_scale, guidance_interval=None):
  """The per-step guidance scales g[N] (float32, indexed by DDIM index like the coefficient table; DESIGN.md section
  11).  `guidance_scale` a float: g[i] = it where t_lo <= steps[i] <= t_hi (`guidance_interval`, bounds in training
  timesteps, inclusive; None = everywhere) and 1 elsewhere.  A sequence of N finite floats: g itself (no interval).
  A step with g[i] == 1 is unguided."""
  steps = np.asarray(steps)
  n = steps.size
  if np.ndim(guidance_scale) > 0:
    if guidance_interval is not None:
      raise ValueError("guidance_interval cannot be given with a sequence guidance_scale: the sequence is the schedule")
    g = np.asarray(guidance_scale, dtype=np.float64)
    if g.ndim != 1 or g.size != n:
      raise ValueError(f"guidance_scale has shape {g.shape}, expected one float or {n} floats (one per DDIM index)")
  else:
    g = np.full(n, float(guidance_scale), dtype=np.float64)
    if guidance_interval is not None:
      if np.ndim(guidance_interval) != 1 or len(guidance_interval) != 2:
        raise ValueError(f"guidance_interval must be (t_lo, t_hi), got {guidance_interval!r}")
      t_lo, t_hi = (float(v) for v in guidance_interval)
      if not t_lo <= t_hi:
        raise ValueError(f"guidance_interval: t_lo={t_lo} must not exceed t_hi={t_hi}")
      g = np.where((steps >= t_lo) & (steps <= t_hi), g, 1.)
  with np.errstate(over="ignore"):                # (a float64 beyond float32's range becomes inf and is rejected)
    g = g.astype(np.float32)
  if not np.all(np.isfinite(g)):
    raise ValueError("guidance_scale must be finite (as float32)")
  return g


PREVIEW_MODES = ("nearest", "bilinear")


def fit_latent_preview(latents, images):
  """The latent-to-RGB matrix of the previews, float32 [c+1,3]: c weight rows, then the bias
  row.  `latents` [n,h,w,c] and `images` [n,f*h,f*w,3] (the decoder's, in [-1, 1]): the f x f block mean of the
  images is regressed on [latents, 1] by least squares, in float64.  ValueError: image extents that are not one
  integer multiple f of the latents', or a design matrix of rank below c + 1 (fewer than c + 1 cells, or channels
  that are affinely dependent)."""
  lat = np.asarray(latents.detach().float().cpu() if isinstance(latents, torch.Tensor) else latents, dtype=np.float64)
  img = np.asarray(images.detach().float().cpu() if isinstance(images, torch.Tensor) else images, dtype=np.float64)
  if lat.ndim != 4 or img.ndim != 4 or img.shape[0] != lat.shape[0] or img.shape[3] != 3:
    raise ValueError(f"fit_latent_preview: latents {lat.shape} must be [n,h,w,c] and images {img.shape} [n,f*h,f*w,3]")
  n, h, w, c = lat.shape
  if min(n, h, w, c) < 1:
    raise ValueError(f"fit_latent_preview: empty latents {lat.shape}")
  f = img.shape[1] // h
  if f < 1 or img.shape[1] != f * h or img.shape[2] != f * w:
    raise ValueError(f"fit_latent_preview: image extents {img.shape[1:3]} are not one integer multiple of the "
                     f"latent extents {(h, w)}")
  target = img.reshape(n, h, f, w, f, 3).mean(axis=(2, 4)).reshape(-1, 3)
  design = np.concatenate([lat.reshape(-1, c), np.ones((n * h * w, 1))], axis=1)
  sol, _, rank, _ = np.linalg.lstsq(design, target, rcond=None)
  if rank < c + 1:
    raise ValueError(f"fit_latent_preview: the design matrix [latents, 1] of shape {design.shape} has rank {rank}, "
                     f"below {c + 1}: the fit is not determined")
  return sol.astype(np.float32)


def attention_step_weights(n, attn_maps):
  """The checked `attn_maps` keyword of the loops: None (no heat maps) or the float32 [n] table
  of weights by DDIM index -- True: every step counts once; else n finite weights >= 0, not all zero."""
  if attn_maps is None:
    return None
  if isinstance(attn_maps, (bool, np.bool_)):
    if not attn_maps:
      raise ValueError("attn_maps must be None, True or a sequence of weights by DDIM index, got False")
    return np.ones(int(n), dtype=np.float32)
  if isinstance(attn_maps, (str, bytes)) or np.ndim(attn_maps) != 1:
    raise ValueError(f"attn_maps must be None, True or {n} weights by DDIM index, got {attn_maps!r}")
  if any(isinstance(v, (bool, np.bool_)) for v in attn_maps):
    raise ValueError("attn_maps weights must be numbers, not bools")
  w = np.asarray(attn_maps, dtype=np.float64)
  if w.shape != (int(n),):
    raise ValueError(f"attn_maps must hold one weight per DDIM index ({n}), got {w.shape[0]}")
  if not np.isfinite(w).all() or (w < 0).any():
    raise ValueError("attn_maps weights must be finite and >= 0")
  with np.errstate(over="ignore"):
    w = w.astype(np.float32)
  if not np.isfinite(w).all() or not (w > 0).any():
    raise ValueError("attn_maps weights must be finite in float32 and not all zero")
  return w


def word_heatmaps(heat, spans):
  """heat [B,Tk,H,W] (last_attention_maps) and spans [(word, [token positions])] (Tokenizer.word_spans) ->
  [B,n_words,H,W]: the sum of each word's token maps."""
  heat = np.asarray(heat)
  if heat.ndim != 4:
    raise ValueError(f"heat must be [B,Tk,H,W], got {heat.shape}")
  out = np.zeros((heat.shape[0], len(spans)) + heat.shape[2:], dtype=heat.dtype)
  for i, (_, pos) in enumerate(spans):
    pos = [int(p) for p in pos]
    if any(not 0 <= p < heat.shape[1] for p in pos):
      raise ValueError(f"token positions {pos} outside the {heat.shape[1]} maps")
    if pos:
      out[:, i] = heat[:, pos].sum(axis=1)
  return out


def combine_attention_maps(raw, weight_sum, size=None, resize=None):
  """The aggregation of last_attention_maps on host arrays: raw = per-layer [B,h_l,w_l,Tk] accumulators ->
  heat [B,Tk,H,W] = (1 / (weight_sum L)) sum_l resize(raw_l -> (H, W)); `resize(a, (H, W))` maps [B,h,w,Tk] to
  [B,H,W,Tk] and is needed only when a layer's size differs from `size` (default: the first layer's)."""
  if not raw:
    raise ValueError("no layers to combine")
  if not weight_sum > 0:
    raise ValueError(f"weight_sum must be positive, got {weight_sum!r}")
  H, W = (int(v) for v in (size if size is not None else raw[0].shape[1:3]))
  total = None
  for a in raw:
    a = np.asarray(a, dtype=np.float32)
    if tuple(a.shape[1:3]) != (H, W):
      if resize is None:
        raise ValueError(f"a layer of size {a.shape[1:3]} needs `resize` to reach {(H, W)}")
      a = np.asarray(resize(a, (H, W)), dtype=np.float32)
    total = a.copy() if total is None else total + a
  heat = total * np.float32(1.0 / (float(weight_sum) * len(raw)))
  return np.ascontiguousarray(heat.transpose(0, 3, 1, 2))


def preview_slots(num_ddim_steps, freq):
  """R = (N - 1) // q + 1: the slots of a preview strip; slot r holds the step at DDIM index r * q."""
  return (int(num_ddim_steps) - 1) // int(freq) + 1


class LatentDiffusionModel(object):

  def __init__(self, unet, autoencoder, cond_stage_model, num_steps=1000, beta_start=1e-4,
               beta_end=2e-2, v_posterior=0., scale_factor=0.18215, eta=0., num_ddim_steps=50, step_spacing="uniform",
               ddim_steps=None):
    if step_spacing not in STEP_SPACINGS:
      raise ValueError(f"step_spacing must be one of {STEP_SPACINGS}, got {step_spacing!r}")
    if ddim_steps is not None and step_spacing != "uniform":
      raise ValueError(f"ddim_steps is a step table of its own: step_spacing={step_spacing!r} cannot be given with it")
    self._unet = unet
    self._autoencoder = autoencoder
    self._cond_stage_model = cond_stage_model
    self._num_steps = num_steps
    self._beta_start = beta_start
    self._beta_end = beta_end
    self._v_posterior = v_posterior
    self._scale_factor = scale_factor
    self._eta = eta
    self._num_ddim_steps = num_ddim_steps
    self._step_spacing = step_spacing if ddim_steps is None else "custom"

    # model_runners.py:379-384 (linspace and square in float32, then float64)
    ls = _tf_linspace_f32(beta_start ** 0.5, beta_end ** 0.5, num_steps)
    self._betas = (ls * ls).astype(np.float32).astype(np.float64)
    self._alphas = 1. - self._betas
    self._alphas_cumprod = np.cumprod(self._alphas, axis=0)
    self._sqrt_recip_alphas_cumprod = np.sqrt(1. / self._alphas_cumprod)
    self._sqrt_recipm1_alphas_cumprod = np.sqrt(1. / self._alphas_cumprod - 1)
    if ddim_steps is not None:
      # a table handed in (the N-divides-num_steps rule belongs to the uniform table)
      self._ddim_steps = check_steps(ddim_steps, num_steps, num_ddim_steps)
    else:
      # :406-409
      self._ddim_steps = np.arange(0, num_steps, num_steps // num_ddim_steps, dtype=np.int32)
      if self._num_ddim_steps < self._num_steps:
        self._ddim_steps = self._ddim_steps + 1
      if self._ddim_steps.max() >= num_steps:
        # tf.gather on CPU raises for an out-of-range index; N must divide num_steps
        raise IndexError(f"ddim step {int(self._ddim_steps.max())} out of range: num_ddim_steps="
                         f"{num_ddim_steps} must divide num_steps={num_steps}")
      if step_spacing != "uniform":
        # another table on the same interval (the uniform table's last entry stays the last)
        self._ddim_steps = check_steps(
            spaced_steps(self._alphas_cumprod, num_ddim_steps, int(self._ddim_steps[-1]), step_spacing), num_steps,
            num_ddim_steps)
    alphas_cumprod = self._alphas_cumprod[self._ddim_steps]
    # :412-415 -- a_prev at index 0 is abar[0], not 1
    self._ddim_alphas_cumprod_prev = np.concatenate(
        [[self._alphas_cumprod[0]], self._alphas_cumprod[self._ddim_steps[:-1]]], axis=0)
    # :416-419
    self._ddim_sigmas = eta * np.sqrt(
        (1 - self._ddim_alphas_cumprod_prev) / (1 - alphas_cumprod) *
        (1 - alphas_cumprod / self._ddim_alphas_cumprod_prev))
    # :420-423
    self._ddim_sqrt_recip_alphas_cumprod = self._sqrt_recip_alphas_cumprod[self._ddim_steps]
    self._ddim_sqrt_recipm1_alphas_cumprod = self._sqrt_recipm1_alphas_cumprod[self._ddim_steps]
    # :389-390 (LatentDiffusionModelTrainer.q_sample's tables)
    self._sqrt_alphas_cumprod = np.sqrt(self._alphas_cumprod)
    self._sqrt_one_minus_alphas_cumprod = np.sqrt(1. - self._alphas_cumprod)

    self.device = getattr(unet, "device", torch.device("cuda:0"))
    self._tables = None
    self._q_tables = None
    self._noise_source = "host"
    self._rng = None
    self._ms_weights = None

  def multistep_weights(self):
    """float64 [N][4][4]: row [i][j] = the weights of (e_i, .., e_{i+j}) at DDIM index i with j
    earlier steps in the loop (j + 1 entries, the rest zero; rows whose history would lie beyond index N - 1 stay
    zero and are never read)."""
    lam = log_snr_half(self._alphas_cumprod[self._ddim_steps])
    lam_prev = log_snr_half(self._ddim_alphas_cumprod_prev)
    n = len(self._ddim_steps)
    w = np.zeros((n, 4, 4), dtype=np.float64)
    for i in range(n):
      for j in range(min(3, n - 1 - i) + 1):
        w[i, j, :j + 1] = deis_weights(lam[i:i + j + 1], lam_prev[i])
    return w

  def _device_ms_weights(self):
    """The float32 cast of multistep_weights() on the device, made on first use; the sampler owns it (a captured
    graph reads it at a fixed address)."""
    if self._ms_weights is None:
      self._ms_weights = torch.from_numpy(self.multistep_weights().astype(np.float32)).to(self.device).contiguous()
    return self._ms_weights

  def _set_rng(self, seed, first_sample_index):
    """The device generator's state uint32[4] = {seed_lo, seed_hi, first_sample_index, 0} (seed mod 2^64; int32
    storage), allocated on first use and rewritten in place: the kernels read it through a fixed pointer."""
    seed = int(seed) % (1 << 64)
    words = np.array([seed & 0xffffffff, seed >> 32, int(first_sample_index) % (1 << 32), 0], dtype=np.uint32)
    if self._rng is None:
      self._rng = torch.zeros(4, dtype=torch.int32, device=self.device)
    self._rng.copy_(torch.from_numpy(words.view(np.int32)))
    return self._rng

  def _device_tables(self):
    """Device copies of the schedule, made on first use: per DDIM index the row
    (c1, c2, a_prev, sigma) after the float32 cast of `_extract`, the int32 step table
    and the device-resident loop index."""
    if self._tables is None:
      coef = np.stack([self._ddim_sqrt_recip_alphas_cumprod, self._ddim_sqrt_recipm1_alphas_cumprod,
                       self._ddim_alphas_cumprod_prev, self._ddim_sigmas], axis=1).astype(np.float32)
      self._tables = (torch.from_numpy(coef).to(self.device),
                      torch.from_numpy(self._ddim_steps.copy()).to(self.device),
                      torch.zeros(1, dtype=torch.int32, device=self.device))
    return self._tables

  def _device_q_tables(self):
    """Device copies of the forward-diffusion tables after the float32 cast of `_extract`: sqrt(abar) and
    sqrt(1 - abar) [num_steps], and per DDIM index the pair gathered at its step [N,2]."""
    if self._q_tables is None:
      sa = self._sqrt_alphas_cumprod.astype(np.float32)
      sb = self._sqrt_one_minus_alphas_cumprod.astype(np.float32)
      per_index = np.stack([sa[self._ddim_steps], sb[self._ddim_steps]], axis=1)
      self._q_tables = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (sa, sb, per_index))
    return self._q_tables

  def q_sample(self, x0, t, eps):
    """model_runners.py:580-600 (LatentDiffusionModelTrainer.q_sample): _extract(sqrt_ac, t) * x0 +
    _extract(sqrt_1m_ac, t) * eps.  x0, eps [B,h,w,c]; t int [B] DDPM timesteps.  float32, on the device."""
    x0 = torch.as_tensor(x0, dtype=torch.float32).to(self.device).contiguous()
    eps = torch.as_tensor(eps, dtype=torch.float32).to(self.device).contiguous()
    t = _as_tensor(t, dtype=None).to(self.device, torch.int32)
    t = t.reshape(-1).contiguous()
    if tuple(eps.shape) != tuple(x0.shape) or t.numel() != x0.shape[0]:
      raise ValueError(f"q_sample: x0 {tuple(x0.shape)}, eps {tuple(eps.shape)}, t {tuple(t.shape)}")
    sa, sb, _ = self._device_q_tables()
    return ops.q_sample(x0, eps, t, sa, sb, torch.empty_like(x0))

  def get_latents(self, inputs, noise=None, seed=0, first_sample_index=0):
    """model_runners.py:602-625: images [B,H,W,3] in [-1, 1] -> scale_factor * latents.  KL: a posterior
    sample (`noise` [B,h,w,c], else drawn from `seed`'s ENCODE_STREAM per global sample index -- by
    ldm_normal_fill when the noise source is "device" -- where the reference draws an unseeded tf.random.normal); VQ: encode(only_encode=True)."""
    # noise source "device": sample i must not depend on how samples are spread over launches or GPUs, so every
    # image is encoded on its own (a pass's launch plans depend on its batch); "host": one pass, as before
    enc = dict(per_sample=True) if self._noise_source == "device" else {}
    if isinstance(self._autoencoder, AutoencoderKL):
      posterior = self._autoencoder.encode(inputs, **enc)
      moments = posterior._moments
      B, h, w, c2 = moments.shape
      if noise is None and self._noise_source == "device":
        noise = ops.normal_fill(torch.empty(B, h, w, c2 // 2, dtype=torch.float32, device=moments.device),
                                self._set_rng(seed, first_sample_index), ENCODE_STREAM)
      elif noise is None:
        noise = normal_latents(seed, first_sample_index, B, (h, w, c2 // 2), stream=ENCODE_STREAM)
      noise = _as_tensor(noise).to(self.device).contiguous()
      if tuple(noise.shape) != (B, h, w, c2 // 2):
        raise ValueError(f"encode noise {tuple(noise.shape)} != latents {(B, h, w, c2 // 2)}")
      out = torch.empty(B, h, w, c2 // 2, dtype=torch.float32, device=moments.device)
      # (mean + std * noise) * scale_factor: the sample, then the float32 scale (:624)
      return ops.gaussian_sample(moments, out, noise=noise, out_scale=np.float32(self._scale_factor))
    elif isinstance(self._autoencoder, AutoencoderVQ):
      latents = self._autoencoder.encode(inputs, only_encode=True, **enc)
      return latents * np.float32(self._scale_factor)
    raise NotImplementedError("Invalid autoencoder")

  @property
  def _coef_dev(self):
    return self._device_tables()[0]

  @property
  def _steps_dev(self):
    return self._device_tables()[1]

  @property
  def _index_dev(self):
    return self._device_tables()[2]

  def decode_first_stage(self, latents):
    """model_runners.py:425-434: latents / scale_factor, then the autoencoder's decode
    (the division is fused into the decoder's first kernel)."""
    if isinstance(self._autoencoder, AutoencoderKL):
      outputs = self._autoencoder.decode(latents, training=False, scale_factor=self._scale_factor)
    elif isinstance(self._autoencoder, AutoencoderVQ):
      outputs = self._autoencoder.decode(latents, force_quantize=True, training=False,
                                         scale_factor=self._scale_factor)
    else:
      raise NotImplementedError("autoencoder not implemented")
    return outputs


# PLMS: row j = Adams-Bashforth weights of (e_i, e_{i+1}, .., e_{i+j}), the guided eps of the
# step at DDIM index i and of the j steps before it in the loop.  cfg_update4_kernel<.., kAdamsBashforth, ..>
# (csrc/sampler.hip) carries the same numbers as (numerators) / denominator.
PLMS_WEIGHTS = (
    (1.,),
    (3. / 2., -1. / 2.),
    (23. / 12., -16. / 12., 5. / 12.),
    (55. / 24., -59. / 24., 37. / 24., -9. / 24.),
)
SAMPLERS = ("ddim", "plms", "deis")
MULTISTEP = ("plms", "deis")     # samplers with a ring of guided eps and a loop start index; deterministic
_GL_X, _GL_W = np.polynomial.legendre.leggauss(16)


def deis_weights(lams, lam_target):
  """DEIS (Zhang & Chen 2022), the exponential-integrator Adams-Bashforth weights in lambda: nodes lams = (l_0, .., l_j)
  (this step's lambda, then the j earlier steps'), the step lands on lam_target > l_0.
    w[m] = int_{l_0}^{l'} e^{-l} L_m(l) dl / int_{l_0}^{l'} e^{-l} dl,  L_m = the Lagrange basis on the nodes.
  With l = l_0 + h s both integrals run over s in [0, 1] with the weight e^{-h s}: 16-point Gauss-Legendre in float64
  (the integrand is e^{-h s} times a polynomial of degree <= 3 and h is a few units at most; the closed form in
  tests/deis_ref.py agrees to 1e-12).  Sum_m w[m] = 1; j = 0 gives (1,), the DDIM step."""
  lams = np.asarray(lams, dtype=np.float64)
  h = float(lam_target) - lams[0]
  if not h > 0.:
    raise ValueError(f"the step must raise lambda: {lams[0]} -> {lam_target}")
  nodes = (lams - lams[0]) / h
  s = 0.5 * (_GL_X + 1.)
  ex = _GL_W * np.exp(-h * s)
  den = ex.sum()
  w = np.empty(len(nodes), dtype=np.float64)
  for m in range(len(nodes)):
    basis = np.ones_like(s)
    for k in range(len(nodes)):
      if k != m:
        basis = basis * ((s - nodes[k]) / (nodes[m] - nodes[k]))
    w[m] = (ex * basis).sum() / den
  return w


class LatentDiffusionModelSampler(LatentDiffusionModel):

  def __init__(self, *args, use_graph=True, verbose=True, temb_table=True, sampler="ddim", noise_source="host",
               skip_unguided=True, **kwargs):
    super().__init__(*args, **kwargs)
    if sampler not in SAMPLERS:
      raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if noise_source not in NOISE_SOURCES:
      raise ValueError(f"noise_source must be one of {NOISE_SOURCES}, got {noise_source!r}")
    self._noise_source = noise_source
    if sampler in MULTISTEP and self._eta != 0:
      raise ValueError(f"sampler={sampler!r} is deterministic: eta must be 0, got {self._eta}")
    self._sampler = sampler
    self._use_graph = use_graph
    self._use_temb_table = bool(temb_table)      # A/B: False = four temb launches + a decrement launch per step
    self._temb_tbl = None
    self._pre_dec = False
    self._verbose = verbose
    self._skip_unguided = bool(skip_unguided)    # A/B: False = an unguided step still evaluates all 2B rows
    self._states = {}                            # (B,h,w,c) -> the device state and captured graphs of a shape
    self._state_key = None                       # that is not the current one (_alloc_state)
    for slot, (key, by_form) in self._GRAPH_SLOTS.items():
      setattr(self, slot, {} if by_form else None)
      setattr(self, key, None)
    self._gtab = None
    self._plms_tbl = None
    self._form_events = None
    self._inv_tbl = None
    self._inv_temb = None
    self._pv_proj = None                         # set_preview: the matrix on the device, the scale and the mode
    self._pv_host = None
    self._pv_scale = None
    self._pv_mode = "bilinear"
    self._pv_last = None
    self._am_tab = None                          # the weights by DDIM index on the device (values change in place)
    self._am_last = None
    self._dm_counters = None                     # two device ints: the contrast step's DDIM index, its draw counter
    self._de_qcoef = None                        # the blend's constant coefficients (0, 1): q_sample(z0, Q) = Q
    self._blend_traj = False                     # whether _blend_kwargs hands the blend the trajectory for Q
    self._dm_last = None
    self._traj_last = None
    self.last_step_ms = None

  # ---- the steps' temb projections, once per sampler ---------------------------------
  def _temb_kwargs(self, dec_index):
    """kwargs of UNet.forward for one step: the table of every DDIM step's temb projections (built on first use: it
    depends on the step table and the weights only) and whether the step's first launch moves the loop counter.
    A U-Net without `temb_table` (any callable with the forward contract) gets neither."""
    if self._temb_tbl is None and hasattr(self._unet, "temb_table") and self._use_temb_table:
      self._temb_tbl = self._unet.temb_table(self._steps_dev).clone()     # (the U-Net's scratch may serve another sampler)
    self._pre_dec = self._temb_tbl is not None
    if self._temb_tbl is None:
      return {}
    return dict(temb_table=self._temb_tbl, pre_decrement=bool(dec_index))

  def _loop_start_index(self, n):
    """Value of the device-side counter before the first step: steps that pre-decrement start one above."""
    self._temb_kwargs(True)
    return n if self._pre_dec else n - 1

  # ---- one step on device state -----------------------------------------------------
  # What belongs to one latent shape (B,h,w,c): the step's state, the buffers the sampler owns and the window batch
  # (all sized by the shape), and the graphs captured over them.  The attributes hold the CURRENT shape's; the others'
  # wait in _states, so a sampler that alternates between two shapes allocates and captures each
  # once.  What the graphs of every shape read alike (_rng, _gtab, the tables, the device counter) is not listed.
  _SHAPE_BUFFERS = ("_xt", "_x2", "_eps", "_ring", "_start", "_noise_buf", "_q_buf", "_z0_buf", "_mask_buf", "_t_buf",
                    "_x_win", "_eps_win", "_win_key", "_win_wy", "_win_wx", "_pv_x0", "_pv_a", "_pv_b", "_am_accs",
                    "_traj", "_dm_acc", "_dm_out", "_dm_noise", "_dm_t")
  # The captured-graph slots, declared once: attribute -> (the attribute of its key, by_form).  A slot holds one
  # captured step (_sample_loop), or with by_form a dict form (guided?) -> captured step (_sample_loop_sched), and the
  # key says what it was captured for.  A loop with a slot of its own (`slot=`) finds the others' graphs as it left
  # them.  The defaults of a fresh sampler, what travels with a shape (_SHAPE_GRAPHS), the keys a fresh shape resets
  # and what _drop_graphs / _clear_slots empty all derive from this table: a new slot is one entry here.
  _GRAPH_SLOTS = {
      "_graph": ("_graph_key", False),               # the sampling loops without a slot of their own
      "_sched_graphs": ("_sched_key", True),         # guidance schedules
      "_inv_graph": ("_inv_graph_key", False),       # the inversion's step (section 13)
      "_pv_graph": ("_pv_graph_key", False),         # the steps captured with previews (section 17)
      "_pv_sched_graphs": ("_pv_sched_key", True),
      "_am_graph": ("_am_graph_key", False),         # the steps captured with heat maps (section 18)
      "_dm_graph": ("_dm_graph_key", False),         # DiffEdit (section 19): the contrast step,
      "_invt_graph": ("_invt_graph_key", False),     # the inversion that keeps its trajectory
      "_de_graph": ("_de_graph_key", False),         # and the sampling whose blend reads it
  }
  _SHAPE_GRAPHS = tuple(_GRAPH_SLOTS) + tuple(key for key, _ in _GRAPH_SLOTS.values())

  def _alloc_state(self, B, h, w, c):
    key = (B, h, w, c)
    if self._state_key != key:
      names = self._SHAPE_BUFFERS + self._SHAPE_GRAPHS
      if self._state_key is not None:
        self._states[self._state_key] = {n: getattr(self, n) for n in names if hasattr(self, n)}
      saved = self._states.pop(key, None)
      for n in self._SHAPE_BUFFERS:
        if hasattr(self, n):
          delattr(self, n)
      if saved is not None:                      # a shape seen before: its buffers and graphs as they were left
        for n, v in saved.items():
          setattr(self, n, v)
        self._state_key = key
        return
      for slot_key, _ in self._GRAPH_SLOTS.values():
        setattr(self, slot_key, None)
      dev, f32 = self.device, torch.float32
      self._xt = torch.empty(B, h, w, c, dtype=f32, device=dev)
      self._x2 = torch.empty(2 * B, h, w, c, dtype=f32, device=dev)
      self._eps = torch.empty(2 * B, h, w, c, dtype=f32, device=dev)
      if self._sampler in MULTISTEP:
        # the last four guided eps by DDIM index & 3 (never initialised: a step reads only slots its own loop wrote)
        # and the DDIM index of the loop's first step
        self._ring = torch.empty(4, B, h, w, c, dtype=f32, device=dev)
        self._start = torch.zeros(1, dtype=torch.int32, device=dev)
      if self._sampler == "deis":
        self._device_ms_weights()                # (made before any capture: the graph reads it at a fixed address)
      if self._noise_source == "device" and self._rng is None:
        self._rng = torch.zeros(4, dtype=torch.int32, device=dev)    # (written by each loop's reset)
      self._state_key = key
      self._drop_graphs()

  def release_shapes(self):
    """Frees the state and graphs kept for every latent shape but the current one."""
    self._states = {}

  def _drop_graphs(self):
    """A buffer the captured steps of the current shape read has a new address."""
    self._clear_slots(*self._GRAPH_SLOTS)

  def _clear_slots(self, *slots, all_shapes=False):
    """Empties the named slots of the current shape and, with `all_shapes`, of every shape parked in _states: what
    their captured steps read is gone.  The keys stay (a key without its graph matches nothing)."""
    for slot in slots:
      by_form = self._GRAPH_SLOTS[slot][1]
      setattr(self, slot, {} if by_form else None)
      for saved in self._states.values() if all_shapes else ():
        saved[slot] = {} if by_form else None

  # ---- latent previews --------------------------------------------------
  def set_preview(self, proj, scale=None, mode="bilinear"):
    """The previews' latent-to-RGB matrix `proj` [c+1,3] (c weight rows, then the bias; fit_latent_preview's result),
    the integer upscale `scale` (None: the autoencoder's pixels per latent cell, so a preview has the image's size) and
    the upscale `mode`, "nearest" or "bilinear".  Changing any of the three drops the steps captured with previews, of
    every latent shape, and no other graph; the same three again change nothing."""
    if mode not in PREVIEW_MODES:
      raise ValueError(f"preview mode must be one of {PREVIEW_MODES}, got {mode!r}")
    scale = self._pixel_factor() if scale is None else scale
    if isinstance(scale, bool) or int(scale) != scale or not 1 <= int(scale) <= 16:
      raise ValueError(f"preview scale must be an int in [1, 16], got {scale!r}")
    proj = np.asarray(proj.detach().cpu() if isinstance(proj, torch.Tensor) else proj, dtype=np.float32)
    if proj.ndim != 2 or proj.shape[1] != 3 or not 2 <= proj.shape[0] <= 17:
      raise ValueError(f"preview matrix must be [c+1,3] with c in [1, 16], got {proj.shape}")
    if not np.isfinite(proj).all():
      raise ValueError("preview matrix must be finite")
    same = (self._pv_proj is not None and (int(scale), mode) == (self._pv_scale, self._pv_mode) and
            np.array_equal(self._pv_host, proj))
    if same:
      return
    # (a new tensor: the graphs that read the old one go with it)
    self._pv_host = proj.copy()
    self._pv_proj = torch.from_numpy(self._pv_host).to(self.device).contiguous()
    self._pv_scale, self._pv_mode = int(scale), mode
    self._clear_slots("_pv_graph", "_pv_sched_graphs", all_shapes=True)

  def fit_preview(self, latents=None, n=8, seed=0, shape=None):
    """Fits the previews' matrix on this sampler's own decoder and stores it (set_preview, keeping the scale and mode
    already set): `latents` [n,h,w,c], scaled as the loops' latents are, are decoded with decode_first_stage and
    handed to fit_latent_preview.  Without `latents`, `n` draws of N(0,1) (normal_latents under a key derived from
    `seed`: its stream PREVIEW_FIT_STREAM) at `shape` = (h, w, c) stand in for them -- default: the latent shape of
    the last loop, else the size the autoencoder is bound to, else 32 x 32, with the autoencoder's latent channels
    (the U-Net itself carries no size).  That default is rough: white noise
    is not what the loops' latents look like, and a matrix fitted on a run's final latents (tools/fit_preview.py)
    gives truer colours.  Returns the float32 [c+1,3] matrix."""
    if latents is None:
      if shape is None:
        if self._state_key is not None:
          shape = self._state_key[1:]
        else:
          side = getattr(self._autoencoder, "_latent_size", None) or 32
          shape = (side, side, getattr(self._autoencoder, "_latent_channels", 4))
      latents = normal_latents(seed, 0, int(n), tuple(int(v) for v in shape), stream=PREVIEW_FIT_STREAM)
    lat = _as_tensor(latents).to(self.device).contiguous()
    images = self.decode_first_stage(lat)
    proj = fit_latent_preview(lat, images)
    self.set_preview(proj, scale=self._pv_scale, mode=self._pv_mode)
    return proj

  def _preview_on(self, preview_freq, on_preview, N):
    """The checked `preview_freq` of a loop call: None (no previews; `on_preview` needs them) or q >= 1, with the
    current shape's pred_x0 buffer and the two strips [R,B,s*h,s*w,3] allocated (after _alloc_state)."""
    if preview_freq is None:
      if on_preview is not None:
        raise ValueError("on_preview needs preview_freq")
      return None
    q = int(preview_freq)
    if isinstance(preview_freq, bool) or q != preview_freq or q < 1:
      raise ValueError(f"preview_freq must be an int of at least 1, got {preview_freq!r}")
    if self._pv_proj is None:
      raise ValueError("preview_freq needs a preview matrix: call set_preview or fit_preview first")
    B, h, w, c = self._xt.shape
    if self._pv_proj.shape[0] != c + 1:
      raise ValueError(f"the preview matrix is {tuple(self._pv_proj.shape)}, latents with {c} channels need {(c + 1, 3)}")
    s = self._pv_scale
    shape = (preview_slots(N, q), B, s * h, s * w, 3)
    if getattr(self, "_pv_a", None) is None or tuple(self._pv_a.shape) != shape:
      self._pv_x0 = torch.empty(B, h, w, c, dtype=torch.float32, device=self.device)
      self._pv_a = torch.zeros(shape, dtype=torch.uint8, device=self.device)
      self._pv_b = torch.zeros(shape, dtype=torch.uint8, device=self.device)
      self._clear_slots("_pv_graph", "_pv_sched_graphs")         # (the captured launches wrote the old strips)
    return q

  def _preview_step(self, q, dec_index):
    """The step's one extra launch: _xt and the step's pred_x0 into the slot of the step's DDIM index.  After the
    update the counter holds that index when the U-Net's first launch pre-decremented it, and one less when the
    update itself moved it (temb_table=False); the uncounted warm-up step moves nothing."""
    ops.latent_preview(self._xt, self._pv_proj, self._pv_a, q, index=self._index_dev,
                       index_bias=1 if dec_index and not self._pre_dec else 0, lat_b=self._pv_x0,
                       frames_b=self._pv_b, scale=self._pv_scale, mode=self._pv_mode)

  def last_previews(self):
    """The strips of the last loop run with preview_freq = q: dict(sample=, pred_x0=) uint8 NumPy [B,R,H,W,3] (x_t
    after, and the predicted x_0 of, the step at DDIM index r * q), indices= int [R] (r * q) and written= bool [R]
    (False: a slot above the loop's first index, left at 0).  Synchronises."""
    if self._pv_last is None:
      raise ValueError("no loop has run with preview_freq")
    q, k, a, b = self._pv_last
    R = a.shape[0]
    indices = np.arange(R) * q
    return dict(sample=np.ascontiguousarray(a.cpu().numpy().swapaxes(0, 1)),
                pred_x0=np.ascontiguousarray(b.cpu().numpy().swapaxes(0, 1)), indices=indices,
                written=indices <= k - 1)

  # ---- cross-attention heat maps ------------------------------------------
  @staticmethod
  def _no_attn_maps(attn_maps, what):
    if attn_maps is not None:
      raise ValueError(f"attn_maps and {what} do not combine")

  def _attn_maps_on(self, attn_maps, attn_layers, gsched, preview_freq, record):
    """The checked heat-map keywords of a loop call: None, or (weights float32 [N] on the host, the layers as a sorted
    tuple) with the weights copied into the device table the captured steps read."""
    if attn_maps is None:
      if attn_layers is not None:
        raise ValueError("attn_layers needs attn_maps")
      return None
    w = attention_step_weights(len(self._ddim_steps), attn_maps)
    if gsched is not None:
      raise ValueError("attn_maps and a guidance schedule (a sequence guidance_scale or guidance_interval) do not combine")
    self._no_attn_maps(None if preview_freq is None else attn_maps, "preview_freq")
    self._no_attn_maps(None if record is None else attn_maps, "record=")
    unet = self._unet
    if not all(hasattr(unet, a) for a in ("capture_attention", "attention_layers", "reset_attention_maps", "sts")):
      raise ValueError("attn_maps needs a U-Net with capture_attention")
    n_st = len(unet.sts)
    layers = tuple(range(n_st)) if attn_layers is None else tuple(sorted(int(n) for n in attn_layers))
    if not layers or len(set(layers)) != len(layers) or not all(0 <= n < n_st for n in layers):
      raise ValueError(f"attn_layers must be distinct indices below {n_st}, got {attn_layers!r}")
    if self._am_tab is None or self._am_tab.numel() != len(w):
      self._am_tab = torch.empty(len(w), dtype=torch.float32, device=self.device)
      self._clear_slots("_am_graph", all_shapes=True)
    self._am_tab.copy_(torch.from_numpy(w))
    return w, layers

  def last_attention_maps(self, size=None, layers=None, mode="bilinear", raw=False):
    """The heat maps of the last loop run with attn_maps: dict(heat= float32 NumPy [B,Tk,H,W], layers= the transformer
    blocks summed, weight_sum= the weights of the DDIM indices the loop ran); heat[b, j] = (1 / (weight_sum L)) sum
    over the L layers of their accumulators [B,h,w,Tk] resized to `size` = (H, W) (default: the latent size) with
    ops.resize_nhwc in `mode`.  `layers`: a subset of the captured ones.  raw=True adds raw=, the per-layer NumPy
    accumulators [B,h_l,w_l,Tk].  Synchronises."""
    if self._am_last is None:
      raise ValueError("no loop has run with attn_maps")
    wsum, shape, accs = self._am_last
    if not wsum > 0:
      raise ValueError("the last loop with attn_maps ran no DDIM index with a positive weight")
    have = [n for n, _, _, _ in accs]
    sel = have if layers is None else [int(n) for n in layers]
    if not sel or len(set(sel)) != len(sel) or any(n not in have for n in sel):
      raise ValueError(f"layers must be distinct members of the captured layers {have}, got {layers!r}")
    H, W = (int(v) for v in (shape if size is None else size))
    if H < 1 or W < 1:
      raise ValueError(f"size must be positive, got {size!r}")
    total, raws = None, []
    for n, h, w, acc in accs:
      if n not in sel:
        continue
      a = acc if (h, w) == (H, W) else ops.resize_nhwc(acc, (H, W), mode)
      total = a.clone() if total is None else total + a
      if raw:
        raws.append(acc.cpu().numpy())
    heat = total * (1.0 / (wsum * len(sel)))
    out = dict(heat=np.ascontiguousarray(heat.permute(0, 3, 1, 2).cpu().numpy()), layers=sorted(sel), weight_sum=wsum)
    if raw:
      out["raw"] = raws
    return out

  def _set_loop_start(self, start_index):
    """PLMS / DEIS: the loop's first step is the one at DDIM index `start_index` (it has no history)."""
    if self._sampler in MULTISTEP:
      self._start.fill_(int(start_index))

  def _start_counters(self, k):
    """The device counters of a sampling loop whose first step is the one at DDIM index k - 1."""
    self._index_dev.fill_(self._loop_start_index(k))                      # :476 (index = k - 1 in the first step)
    self._set_loop_start(k - 1)

  def _copy_start(self, src):
    """A loop's start state from latents on the device: _xt and both halves of the first U-Net input."""
    B = self._xt.shape[0]
    self._xt.copy_(src)
    self._x2[:B].copy_(src)
    self._x2[B:].copy_(src)

  def _owned(self, name, src, shape, dtype=torch.float32):
    """`src` copied into a buffer the sampler owns (one per name and shape): a captured graph reads it at a
    fixed address, whatever tensor the caller passed.  A new buffer drops the captured graph."""
    src = _as_tensor(src, dtype)
    if tuple(src.shape) != tuple(shape):
      raise ValueError(f"{name}: shape {tuple(src.shape)}, expected {tuple(shape)}")
    buf = getattr(self, name, None)
    if buf is None or tuple(buf.shape) != tuple(shape):
      buf = torch.empty(shape, dtype=dtype, device=self.device)
      setattr(self, name, buf)
      self._drop_graphs()
    buf.copy_(src)
    return buf

  def _noise_table(self, noises, shape):
    """Per-step noise in a buffer the sampler owns (one per shape)."""
    return self._owned("_noise_buf", noises, shape)

  def _step(self, guidance_scale, clip_denoised, noise_table, dec_index, pred_x0_out=None, masked=False, rng=False):
    """unet([xt; xt], t=steps[index]) -> CFG -> DDIM update, all on device.  `masked`: the update also pins the
    kept cells for the next step (img2img inpainting: _z0_buf, _mask_buf, _q_buf; still one launch).  `rng`: the
    update draws the eta noise and the blend's Q itself from _rng (no noise_table, no _q_buf; still one launch)."""
    # (paired_rows: x2 = [xt; xt], one timestep -- rows r and r + B differ only in their context, :449-452)
    # The loop counter moves at the START of a step (`dec_index`: the U-Net's first launch pre-decrements it and
    # selects the step's row of the temb table), so a loop starts from index = N and ends at 0.
    self._unet.forward(self._x2, steps=self._steps_dev, index=self._index_dev, out=self._eps, paired_rows=True,
                       **self._temb_kwargs(dec_index))
    self._update(guidance_scale, clip_denoised, noise_table, dec_index, self._x2, pred_x0_out, masked, rng)

  def _update(self, guidance_scale, clip_denoised, noise_table, dec_index, x_unet_out, pred_x0_out=None, masked=False,
              rng=False):
    """The one update launch of the configured solver on _eps / _xt (`x_unet_out`: where the next U-Net input goes,
    None = nowhere)."""
    rng, multistep = bool(rng), self._sampler in MULTISTEP
    # (device noise: no tables; multistep: eta = 0, so no noise table either, and the loops never clip)
    assert noise_table is None or not (rng or multistep)
    assert not (clip_denoised and multistep)
    update = {("ddim", False): ops.cfg_ddim_update_masked if masked else ops.cfg_ddim_update,
              ("ddim", True): ops.cfg_ddim_update_rng,
              ("plms", False): ops.cfg_plms_update, ("plms", True): ops.cfg_plms_update_rng,
              ("deis", False): ops.cfg_ms_update, ("deis", True): ops.cfg_ms_update_rng}[self._sampler, rng]
    kw = dict(coef=self._coef_dev, index=self._index_dev, guidance_scale=guidance_scale, x_unet_out=x_unet_out,
              dec_index=dec_index and not self._pre_dec, pred_x0_out=pred_x0_out, **self._blend_kwargs(masked, rng))
    if multistep:
      kw.update(ring=self._ring, start=self._start)
      if self._sampler == "deis":
        kw.update(weights=self._device_ms_weights())
    else:
      kw.update(clip_denoised=clip_denoised)
      if not rng:
        kw.update(noise=noise_table, noise_index_stride=0 if noise_table is None else noise_table[0].numel())
    if rng:
      kw.update(rng=self._rng)
    update(self._eps, self._xt, self._xt, **kw)

  def _blend_kwargs(self, masked, rng):
    """The inpainting blend's arguments of an update: none unless `masked`; the Q table unless Q is drawn (`rng`)."""
    if not masked:
      return {}
    if self._blend_traj:
      # DiffEdit: Q = the inversion trajectory under the coefficients (0, 1), so the blend's
      # q_sample(z0, Q[j]) is traj[j] bit for bit; always the table-reading entries
      assert not rng
      return dict(z0=self._z0_buf, mask=self._mask_buf, q_coef=self._de_qcoef, q_noise=self._traj,
                  q_index_stride=self._traj[0].numel())
    blend = dict(z0=self._z0_buf, mask=self._mask_buf, q_coef=self._device_q_tables()[2])
    if not rng:
      blend.update(q_noise=self._q_buf, q_index_stride=self._q_buf[0].numel())
    return blend

  # ---- guidance schedules ---------------------------------------------
  def _guidance(self, guidance_scale, guidance_interval):
    """None for a float scale without an interval (the loops above, untouched); else the schedule's float32 [N] table
    in the device buffer the sampler owns (its values change in place: the captured steps read it by address)."""
    if np.ndim(guidance_scale) == 0 and guidance_interval is None:
      return None
    g = guidance_table(self._ddim_steps, guidance_scale, guidance_interval)
    if self._eta != 0:
      raise ValueError(f"a guidance schedule (a sequence guidance_scale or guidance_interval) needs eta = 0, got "
                       f"{self._eta}: the scheduled update has no eta noise")
    if self._gtab is None:
      self._gtab = torch.empty(len(g), dtype=torch.float32, device=self.device)
    self._gtab.copy_(torch.from_numpy(g))
    return g

  def _sched_weights(self):
    """The weight table of the scheduled update: None (ddim: no history), the Adams-Bashforth constants as a table
    (plms: row [i][j] = PLMS_WEIGHTS[j]) or multistep_weights() (deis); float32 [N,4,4] on the device."""
    if self._sampler == "deis":
      return self._device_ms_weights()
    if self._sampler == "plms":
      if self._plms_tbl is None:
        w = np.zeros((len(self._ddim_steps), 4, 4), dtype=np.float32)
        for j, row in enumerate(PLMS_WEIGHTS):
          w[:, j, :j + 1] = np.array(row, dtype=np.float32)
        self._plms_tbl = torch.from_numpy(w).to(self.device).contiguous()
      return self._plms_tbl
    return None

  def _step_sched(self, guided, dec_index, pred_x0_out=None, masked=False, rng=False):
    """One step of a guidance schedule.  Guided: today's U-Net evaluation on [xt; xt], then the update with the scale
    gtab[index].  Unguided: the U-Net on the conditional rows x2[B:] against the resident context's rows B .. 2B-1,
    writing eps[B:] (skip_unguided=False: all 2B rows, as a guided step), then the update on eps[B:] alone.  Either
    update writes both halves of x2."""
    B = self._xt.shape[0]
    if guided or not self._skip_unguided:
      self._unet.forward(self._x2, steps=self._steps_dev, index=self._index_dev, out=self._eps, paired_rows=True,
                         **self._temb_kwargs(dec_index))
    else:
      self._unet.forward(self._x2[B:], steps=self._steps_dev, index=self._index_dev, out=self._eps[B:],
                         paired_rows=False, context_rows=(B, 2 * B), **self._temb_kwargs(dec_index))
    hist = {}
    weights = self._sched_weights()
    if weights is not None:
      hist = dict(ring=self._ring, start=self._start, weights=weights)
    ops.cfg_sched_update(self._eps, self._xt, self._xt, self._coef_dev, self._gtab, self._index_dev, guided,
                         rng=self._rng if rng else None, x_unet_out=self._x2,
                         dec_index=dec_index and not self._pre_dec, pred_x0_out=pred_x0_out, **hist,
                         **self._blend_kwargs(masked, rng))

  def _sample_loop_sched(self, forms, reset, step, gkey, record, slot="_sched_graphs", after_step=None):
    """_sample_loop for a guidance schedule: forms[s] = whether the s-th step of the loop is guided (host-known when
    the loop starts; the index stays on the device); `step(guided, dec_index)` enqueues one step.  With graphs, one
    step per form in use is captured once per `gkey` (guided first) and the host replays whichever form each step
    takes.  Events around every contiguous run of one form give the per-form times (last_form_ms_per_step).  `slot`:
    a by-form slot of _GRAPH_SLOTS, as in _sample_loop; `after_step(s)` runs on the host after the s-th step is
    enqueued."""
    reset()
    graphs = None
    if self._use_graph and record is None:
      key = self._GRAPH_SLOTS[slot][0]
      if getattr(self, key) != gkey:
        self._clear_slots(slot)
        setattr(self, key, gkey)
      graphs = getattr(self, slot)
      for guided in sorted(set(forms) - set(graphs), reverse=True):
        graphs[guided] = self._capture_step(len(forms), reset, lambda dec: step(guided, dec))
    marks = self._run_steps(forms, graphs, step, record, after_step)
    self._form_events = (marks, list(forms))

  def last_form_ms_per_step(self):
    """{"guided": ms, "unguided": ms} of the last scheduled loop: device time of the contiguous runs of each form
    divided by its step count (None for a form the loop did not take; synchronises)."""
    marks, forms = self._form_events
    marks[-1][0].synchronize()
    total = {True: 0., False: 0.}
    for (e0, _), (e1, guided) in zip(marks[:-1], marks[1:]):
      total[guided] += e0.elapsed_time(e1)
    count = {True: sum(forms), False: len(forms) - sum(forms)}
    return {name: (total[k] / count[k] if count[k] else None) for name, k in (("guided", True), ("unguided", False))}

  def _sched_forms(self, g, first, count):
    """Guided? for the steps at DDIM indices first, first - 1, .. (count of them)."""
    return [bool(g[i] != 1.) for i in range(first, first - count, -1)]

  def _sched_key_of(self, masked, rng):
    return ("sched", self._ctx_shape, masked, self._noise_source, rng, self._step_spacing, self._sampler,
            self._skip_unguided)

  def ddim_sample(self, xt, cond, index, guidance_scale=1., clip_denoised=True,
                  return_pred_x0=False, noise=None):
    """model_runners.py:438-472 for a host-side `index`.  `noise` [B,h,w,c] replaces
    the reference's tf.random.normal draw (zeros when omitted; irrelevant at eta=0).
    Always the DDIM step, also on a sampler="plms" or "deis" sampler: a single step has no history."""
    xt = torch.as_tensor(xt, dtype=torch.float32).to(self.device).contiguous()
    B, h, w, c = xt.shape
    self._alloc_state(B, h, w, c)
    self._set_context(cond)
    self._copy_start(xt)
    self._index_dev.fill_(int(index))
    nz = None
    if noise is not None:
      nz = torch.as_tensor(noise, dtype=torch.float32).to(self.device).contiguous()[None]
    pred_x0 = torch.empty_like(self._xt) if return_pred_x0 else None
    sample = torch.empty_like(self._xt)
    self._unet.forward(self._x2, steps=self._steps_dev, index=self._index_dev, out=self._eps, paired_rows=True,
                       **self._temb_kwargs(False))
    ops.cfg_ddim_update(self._eps, self._xt, sample, self._coef_dev, self._index_dev,
                        guidance_scale, noise=nz, x_unet_out=None, dec_index=False,
                        clip_denoised=clip_denoised, noise_index_stride=0, pred_x0_out=pred_x0)
    if return_pred_x0:
      return sample, pred_x0
    return sample

  def _set_context(self, cond):
    """Always re-projects the context (never cached on the tensor's address: the allocator
    reuses a freed context's address for the next prompt).  The U-Net keeps the projections
    in its own persistent buffers, one set per context shape, so a captured graph only has
    to be rebuilt when that shape changes."""
    cond = torch.as_tensor(cond).to(self.device).contiguous()
    self._unet.set_context(cond)
    self._ctx_shape = tuple(cond.shape)

  def _eta_noise_table(self, noises, seed, first_sample_index, B, h, w, c):
    """[N,B,h,w,c] per-step noise (read only when eta > 0): `noises`, else per DDIM index i the stream seed + 1 + i
    (noise source "device": row i filled on the device from stream ETA_STREAM + i)."""
    if self._eta == 0.:
      return None
    n = len(self._ddim_steps)
    if noises is None and self._noise_source == "device":
      return self._device_table("_noise_buf", (n, B, h, w, c), ETA_STREAM, n, seed, first_sample_index)
    if noises is None:
      noises = np.stack([normal_latents(seed + 1 + i, first_sample_index, B, (h, w, c)) for i in range(n)])
    return self._noise_table(noises, (n, B, h, w, c))

  def _device_table(self, name, shape, stream0, rows, seed, first_sample_index):
    """A per-step table the caller did not give while giving another (the step then runs the table entry): rows
    0 .. rows-1 of the owned buffer `name` filled by ldm_normal_fill from streams stream0 + i, the numbers the fused
    path would draw; later rows are never read."""
    buf = getattr(self, name, None)
    if buf is None or tuple(buf.shape) != tuple(shape):
      buf = torch.zeros(shape, dtype=torch.float32, device=self.device)
      setattr(self, name, buf)
      self._drop_graphs()
    rng = self._set_rng(seed, first_sample_index)
    for i in range(rows):
      ops.normal_fill(buf[i], rng, stream0 + i)
    return buf

  def _draws_on_device(self, noises, q_noises=None):
    """Noise source "device" and no per-step table given: the step's update launch draws what it needs."""
    return self._noise_source == "device" and noises is None and q_noises is None

  def _sample_loop(self, num_steps, reset, step, gkey, record, slot="_graph", after_step=None):
    """Run `num_steps` DDIM steps from the state `reset()` sets (latents, U-Net input and the device counter at
    _loop_start_index(num_steps)); `step(dec_index)` enqueues one step.  With graphs (and no `record`) one step
    is captured once per `gkey` -- after a warm-up step on a side stream has allocated every scratch buffer --
    and replayed num_steps times; the counter lives on the device, so the graph serves any start index.  `slot`: the
    slot of _GRAPH_SLOTS that keeps the graph and its key: a loop with a slot of its own does not evict the others'.
    `after_step(s)` runs on the host after the s-th step is enqueued."""
    reset()
    graphs = None
    if self._use_graph and record is None:
      key = self._GRAPH_SLOTS[slot][0]
      if getattr(self, slot) is None or getattr(self, key) != gkey:
        setattr(self, slot, self._capture_step(num_steps, reset, step))
        setattr(self, key, gkey)
      graphs = {None: getattr(self, slot)}
    self._run_steps([None] * num_steps, graphs, lambda form, dec: step(dec), record, after_step)      # :484-502

  def _capture_step(self, num_steps, reset, step):
    """The graph of one step `step(dec_index)`, captured from the state `reset()` sets after a warm-up step on a side
    stream has allocated every scratch buffer; leaves that state behind.  The one capture sequence of every loop."""
    self._index_dev.fill_(num_steps - 1)             # (the warm-up step does not move the counter)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
      step(False)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    reset()
    g = torch.cuda.CUDAGraph()
    # thread-local capture mode: in a multi-GPU job the RCCL watchdog thread polls events
    # while this thread captures; only this thread's calls belong to the capture
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
      step(True)
    reset()
    return g

  def _run_steps(self, forms, graphs, step, record, after_step):
    """The timed run of every loop: step s takes the form forms[s] -- a replay of graphs[form], or with `graphs` None
    the eager `step(form, True)`, after which `record` receives a copy of x_t -- and `after_step(s)` follows it on the
    host.  An event is recorded right before the first step and after the last step of every contiguous run of one
    form; returns them as [(event, the form of the run it ends)] (None for the first) and sets _loop_events."""
    runs = [(form, len(list(same))) for form, same in itertools.groupby(forms)]
    marks = [(torch.cuda.Event(enable_timing=True), None)]
    done = 0
    marks[0][0].record()
    for form, count in runs:
      replay = None if graphs is None else graphs[form].replay
      for i in range(done, done + count):
        if replay is not None:
          replay()
        else:
          step(form, True)
          if record is not None:
            record.append(self._xt.clone())
        if after_step is not None:
          after_step(i)
      done += count
      ev = torch.cuda.Event(enable_timing=True)
      ev.record()
      marks.append((ev, form))
    self._loop_events = (marks[0][0], marks[-1][0], len(forms))
    return marks

  def _denoise(self, k, set_start, guidance_scale, gsched, noise_table, masked, rng, record, decode=True,
               preview_freq=None, on_preview=None, attn_maps=None, attn_layers=None):
    """DDIM indices k-1 .. 0 of the configured solver from the latents `set_start()` leaves in _xt / _x2 (what
    ddim_p_sample_loop, its start_index= form and the img2img loop share); returns the decoded images, or with
    decode=False the latents (_xt itself: the current shape's state).  `preview_freq` = q:
    every step also writes pred_x0 and ends with the one preview launch, captured with it in a graph slot of the
    previews' own; None leaves the keys, the launches and the graphs as they are without the keyword.  `attn_maps`
    (DESIGN.md section 18): the U-Net evaluations also add their cross-attention maps into its accumulators, again
    in a graph slot of their own."""
    am = self._attn_maps_on(attn_maps, attn_layers, gsched, preview_freq, record)
    q = self._preview_on(preview_freq, on_preview, len(self._ddim_steps))
    B = self._xt.shape[0]
    am_accs = getattr(self, "_am_accs", None) or {}

    def reset():
      set_start()
      self._start_counters(k)
      if q is not None:                       # (outside the graph: what the warm-up and capture steps wrote goes,
        self._pv_a.zero_()                     # and the slots this loop never reaches read 0)
        self._pv_b.zero_()
      if am is not None:                       # (outside the graph too: the warm-up and capture steps added theirs)
        self._unet.reset_attention_maps()

    def after_step(s):
      index = k - 1 - s
      if on_preview is not None and index % q == 0:
        on_preview(index, self._pv_a[index // q], self._pv_b[index // q])

    # previews: the update also writes pred_x0, one launch follows it, the key says so and the graphs have their slots
    pv, pkey, own, own_sched = {}, (), {}, {}
    if self._blend_traj:
      # the blend reads the trajectory: the key says so and the step has a slot of its own, so
      # this loop and the masked img2img loop never share a captured step
      assert masked and not rng and gsched is None and q is None and am is None
      pkey, own = (("traj_blend",),), dict(slot="_de_graph")
    if q is not None:
      pv, pkey = dict(pred_x0_out=self._pv_x0), (("preview", q, self._pv_scale, self._pv_mode),)
      own = dict(slot="_pv_graph", after_step=after_step)
      own_sched = dict(slot="_pv_sched_graphs", after_step=after_step)
      self._pv_last = (q, k, self._pv_a, self._pv_b)

    def step_sched(guided, dec):
      self._step_sched(guided, dec, masked=masked, rng=rng, **pv)
      if q is not None:
        self._preview_step(q, dec)

    def step(dec):
      self._step(guidance_scale, False, noise_table, dec_index=dec, masked=masked, rng=rng, **pv)
      if q is not None:
        self._preview_step(q, dec)

    if gsched is not None:
      self._sample_loop_sched(self._sched_forms(gsched, k - 1, k), reset, step_sched,
                              self._sched_key_of(masked, rng) + pkey, record, **own_sched)
    else:
      gkey = (float(guidance_scale), noise_table is not None, self._ctx_shape, masked, self._noise_source, rng,
              self._step_spacing, self._sampler) + pkey
      if am is None:
        self._sample_loop(k, reset, step, gkey, record, **own)
      else:
        # the conditional half of every evaluation, weighted by the table's entry at the device counter: inside the
        # U-Net the counter holds the step's DDIM index in every mode (the temb launch has pre-decremented it, or the
        # update moves it afterwards; the uncounted warm-up step sits on the loop's first index), so the bias is 0
        self._unet.capture_attention(rows=(B, 2 * B), layers=am[1], step_w=self._am_tab, index_bias=0)
        try:
          self._sample_loop(k, reset, step, gkey + (("attn", am[1]),), record, slot="_am_graph")
          fresh = self._unet.attention_layers()
        finally:
          self._unet.capture_attention(None)
        if fresh:                              # (a replayed graph ran no host code: the accumulators are the ones
          am_accs[am[1]] = fresh               # its capture saw)
          self._am_accs = am_accs
        self._am_last = (float(am[0][:k].astype(np.float64).sum()), tuple(self._xt.shape[1:3]), am_accs[am[1]])
    return self._finish(self._xt) if decode else self._xt

  def ddim_p_sample_loop(self, cond_model_inputs, shape, guidance_scale=5., x_T=None,
                         noises=None, seed=0, first_sample_index=0, record=None, guidance_interval=None,
                         start_index=None, preview_freq=None, on_preview=None, attn_maps=None, attn_layers=None):
    """model_runners.py:474-509.  Extra inputs the reference lacks: `x_T` [B,h,w,4]
    (else N(0,1) from `seed`, keyed per global sample index), `noises` [N,B,h,w,4]
    indexed by DDIM index (only read when eta > 0), `record` (list: receives x_t
    after every step -- disables graph replay).  noise_source="device": what the caller
    does not give is drawn on the device; without `noises` no table exists.
    `guidance_scale` may be N floats indexed by DDIM index, or a float with `guidance_interval` = (t_lo, t_hi) in
    training timesteps (guided where t_lo <= steps[i] <= t_hi); DESIGN.md section 11, eta = 0 only.
    `start_index` = k in [1, N]: `x_T` (required) lies on the level of steps[k-1], what
    ddim_invert_loop returns, and the loop runs DDIM indices k-1 .. 0 only, a multistep solver without history at
    its first step; tables and schedules stay indexed by DDIM index.  None: all N steps.
    `preview_freq` = q (needs set_preview or fit_preview): every step also writes small RGB
    pictures of x_t and of its predicted x_0 into slot index / q of two uint8 strips when its DDIM index is a multiple
    of q, with one extra launch inside the captured step; last_previews() returns the strips, and
    `on_preview(ddim_index, sample_u8, pred_x0_u8)` is called on the host after each such step is enqueued with device
    views [B,H,W,3] of its slot (nothing synchronises unless the callback reads them).  None: nothing changes.
    `attn_maps`: True, or N finite weights >= 0 by DDIM index -- every U-Net evaluation also adds
    the head-averaged cross-attention probabilities of the conditional rows, times its step's weight, into one
    accumulator per transformer block (`attn_layers`: indices into the U-Net's blocks, None = all), one extra launch
    per block inside the captured step; last_attention_maps() returns the per-token heat maps.  Not with guidance
    schedules, preview_freq or record=.  None: nothing changes."""
    gsched = self._guidance(guidance_scale, guidance_interval)
    n = len(self._ddim_steps)
    k = n
    if start_index is not None:
      k = int(start_index)
      if x_T is None:
        raise ValueError("start_index needs x_T: the latents on the level of steps[start_index - 1]")
      if k != start_index or not 1 <= k <= n:
        raise ValueError(f"start_index must be an int in [1, {n}], got {start_index!r}")
    context = self._cond_stage_model(cond_model_inputs)                   # :475
    return self._sample_from(context, shape, k, guidance_scale, gsched, x_T, noises, seed, first_sample_index, record,
                             preview_freq=preview_freq, on_preview=on_preview, attn_maps=attn_maps,
                             attn_layers=attn_layers)

  def _sample_from(self, context, shape, k, guidance_scale, gsched, x_T, noises, seed, first_sample_index, record,
                   decode=True, preview_freq=None, on_preview=None, attn_maps=None, attn_layers=None):
    """ddim_p_sample_loop from the text context on: DDIM indices k-1 .. 0 from x_T."""
    B, h, w, c = (int(s) for s in shape)
    xt = self._x_T(x_T, seed, first_sample_index, B, h, w, c)
    # :480-482 concat(context[:4], context[4:]) == context
    cond_combined = context
    self._alloc_state(B, h, w, c)
    self._set_context(cond_combined)
    rng = self._draws_on_device(noises)
    noise_table = None if rng else self._eta_noise_table(noises, seed, first_sample_index, B, h, w, c)
    return self._denoise(k, lambda: self._set_x_T(xt, seed, first_sample_index, B), guidance_scale, gsched,
                         noise_table, False, rng, record, decode=decode, preview_freq=preview_freq,
                         on_preview=on_preview, attn_maps=attn_maps, attn_layers=attn_layers)

  def _x_T(self, x_T, seed, first_sample_index, B, h, w, c):
    """The caller's x_T on the device; drawn on the host when omitted; None (noise source "device") = drawn on the
    device by _set_x_T."""
    if x_T is None and self._noise_source == "device":
      return None
    if x_T is None:
      x_T = normal_latents(seed, first_sample_index, B, (h, w, c))
    xt = _as_tensor(x_T).to(self.device).contiguous()
    assert tuple(xt.shape) == (B, h, w, c)
    return xt

  def _set_x_T(self, xt, seed, first_sample_index, B):
    """The loop's start state: the latents and both halves of the first U-Net input; with the noise source
    "device" also the generator state (and x_T itself from stream XT_STREAM when the caller gave none)."""
    if self._noise_source == "device":
      self._set_rng(seed, first_sample_index)
    if xt is None:
      ops.normal_fill(self._xt, self._rng, XT_STREAM, x_unet_out=self._x2)
      return
    self._copy_start(xt)

  def _finish(self, latents):
    if self._verbose:                                                     # :503
      print(f"[INFO] Done running denoising for {self._num_ddim_steps} steps with"
            f" eta {self._eta}")
      sys.stdout.flush()
    images = self.decode_first_stage(latents)                             # :506
    if self._verbose:                                                     # :507
      print("[INFO] Done decoding images from the final latent variable.")
      sys.stdout.flush()
    return images

  def ddim_p_sample_loop_img2img(self, cond_model_inputs, init_images, guidance_scale=5., strength=0.75,
                                 mask=None, encode_noise=None, q_noises=None, noises=None, seed=0,
                                 first_sample_index=0, record=None, guidance_interval=None, image_size=None,
                                 fit="stretch", resample="lanczos3", preview_freq=None, on_preview=None,
                                 attn_maps=None, attn_layers=None, masked_content="original", paste_back=False,
                                 mask_feather=0., color_match=False):
    """img2img (SDEdit) and masked inpainting on the DDIM loop.
    cond_model_inputs: token ids [uncond x B; cond x B].  init_images [B,H,W,3] (or [H,W,3], tiled) float32
    in [-1, 1].  z0 = get_latents(init_images, encode_noise); k = int(strength * N); the loop starts from
    x = q_sample(z0, steps[k-1], Q[k-1]) and runs DDIM indices k-1 .. 0.  `mask` [B,h,w] (or [h,w]) at latent
    resolution, 1 = keep: before the step at every index i < k-1, x <- m q_sample(z0, steps[i], Q[i]) + (1-m) x.
    `q_noises` [N,B,h,w,c] (Q, indexed by DDIM index; else seed's Q_STREAM + i per global sample index),
    `noises` as in ddim_p_sample_loop, `record` receives x after each of the k steps (eager, no graph).
    `guidance_scale` / `guidance_interval` as in ddim_p_sample_loop (the table covers all N indices; the loop walks
    its first k).  `image_size` = (H, W) (None: everything above, unchanged): init images of
    any extents are brought to (H, W) on the device before the encoder -- `fit` "stretch" resamples the whole image,
    "crop" its centred box of the target's aspect ratio (resample.crop_box), `resample` names the filter of
    ops.resample_nhwc; images already (H, W) take the path above untouched -- and `mask` may also be a pixel mask at the
    source images' size ([B,Hs,Ws] or [Hs,Ws], nonzero = keep), reduced over the same box by latent_mask_fit; a mask
    whose extents are the latent ones is read as a latent mask.  `preview_freq` / `on_preview` as in
    ddim_p_sample_loop (the strips have a slot for every multiple of q below N; the loop writes those it reaches, up
    to (k-1) // q, and leaves the others 0); `attn_maps` / `attn_layers` too (the weights stay indexed by DDIM index;
    weight_sum covers the k indices run).  `masked_content`: "original" (default: everything
    above, unchanged) starts the regenerated region from the init image's own latents; "fill" (needs `mask`) first
    replaces that region of the image the encoder sees -- after `image_size` fitting -- by a smooth continuation of
    the kept pixels (ops.pushpull_fill, keep weights by fill_keep_mask), one eager call before the encoder.
    `paste_back` (needs `mask`; False: everything above, unchanged): after the decode the init
    images' own pixels -- after `image_size` fitting, before any fill -- are put back bit for bit wherever
    fill_keep_mask keeps them; `mask_feather` = sigma in pixels (0 .. 16) hides the seam with a ramp that lies inside
    the kept region, `color_match` first applies to the decoded image the per-channel gain and offset that bring its
    mean and variance over the kept pixels to the init images' (both need `paste_back`).  Three eager calls after the
    decode, nothing inside the captured step; last_paste_weights() and last_color_match() return what they used.
    Returns the decoded images; the final latents stay in self._xt."""
    size = self._image_size(image_size, fit, resample)
    if masked_content not in MASKED_CONTENTS:
      raise ValueError(f"masked_content must be one of {MASKED_CONTENTS}, got {masked_content!r}")
    if masked_content == "fill" and mask is None:
      raise ValueError("masked_content 'fill' fills the region a mask regenerates: it needs mask")
    paste = self._paste_args(paste_back, mask_feather, color_match, mask is not None)
    gsched = self._guidance(guidance_scale, guidance_interval)
    n = len(self._ddim_steps)
    k = img2img_start(strength, n)
    B = len(cond_model_inputs) // 2
    imgs = self._init_images(init_images, B)
    keep = None
    if masked_content == "fill" or paste is not None:
      src = tuple(int(v) for v in imgs.shape[1:3])
      keep = fill_keep_mask(mask, src, src if size is None else size, self._pixel_factor(), fit)
    if mask is not None and size is not None:
      mask = self._fit_mask(mask, tuple(imgs.shape[1:3]), size, fit)
    if mask is not None:
      mask = self._latent_mask(mask, B)
    if size is not None:
      imgs = self._fit_images(imgs, size, fit, resample)
    originals = imgs
    if masked_content == "fill":
      imgs = self._fill_images(imgs, keep)
    context = self._cond_stage_model(cond_model_inputs)
    z0 = self.get_latents(imgs, noise=encode_noise, seed=seed, first_sample_index=first_sample_index)
    images = self._sdedit(context, z0, k, guidance_scale, gsched, mask, q_noises, noises, seed, first_sample_index,
                          record, preview_freq=preview_freq, on_preview=on_preview, attn_maps=attn_maps,
                          attn_layers=attn_layers)
    return images if paste is None else self._paste_back(images, originals, keep, *paste)

  def _sdedit(self, context, z0, k, guidance_scale, gsched, mask, q_noises, noises, seed, first_sample_index, record,
              preview_freq=None, on_preview=None, attn_maps=None, attn_layers=None):
    """The img2img loop from the latents z0 [B,h,w,c] on: q_sample to the level of steps[k-1], DDIM indices k-1 .. 0
    (with the blend when `mask` is given), decode."""
    n = len(self._ddim_steps)
    B, h, w, c = z0.shape
    if mask is not None:
      mask = self._latent_mask(mask, B, (h, w))
    self._alloc_state(B, h, w, c)
    self._set_context(context)
    rng = self._draws_on_device(noises, q_noises)
    noise_table = None if rng else self._eta_noise_table(noises, seed, first_sample_index, B, h, w, c)
    if rng:
      q_buf = None                             # (Q is drawn where it is used: reset's q_sample and the blend)
    elif q_noises is None and self._noise_source == "device":
      q_buf = self._device_table("_q_buf", (n, B, h, w, c), Q_STREAM, k, seed, first_sample_index)
    else:
      if q_noises is None:
        q_noises = np.zeros((n, B, h, w, c), dtype=np.float32)
        for i in range(k):                     # (rows >= k are never read)
          q_noises[i] = normal_latents(seed, first_sample_index, B, (h, w, c), stream=Q_STREAM + i)
      q_buf = self._owned("_q_buf", q_noises, (n, B, h, w, c))
    z0_buf = self._owned("_z0_buf", z0, (B, h, w, c))
    if mask is not None:
      self._owned("_mask_buf", mask, (B, h, w))
    t_start = self._owned("_t_buf", np.full(B, self._ddim_steps[k - 1]), (B,), dtype=torch.int32)
    sa, sb, _ = self._device_q_tables()
    masked = mask is not None

    def set_start():
      if self._noise_source == "device":
        self._set_rng(seed, first_sample_index)
      if rng:
        ops.q_sample_rng(z0_buf, self._rng, Q_STREAM + k - 1, t_start, sa, sb, self._xt, x_unet_out=self._x2)
      else:
        ops.q_sample(z0_buf, q_buf[k - 1], t_start, sa, sb, self._xt, x_unet_out=self._x2)

    return self._denoise(k, set_start, guidance_scale, gsched, noise_table, masked, rng, record,
                         preview_freq=preview_freq, on_preview=on_preview, attn_maps=attn_maps, attn_layers=attn_layers)

  # ---- outpainting and masked-content fill ------------------------------
  def _fill_images(self, imgs, keep):
    """imgs [B,H,W,3] with the cells `keep` [B,H,W] (or [1,H,W], tiled; 1 = keep) does not keep filled from the kept
    ones on the device (ops.pushpull_fill): one eager call in front of the encoder, no state of the sampler's."""
    x = imgs.to(self.device, torch.float32).contiguous()
    m = _as_tensor(keep).to(self.device)
    m = m.expand(x.shape[0], *m.shape[1:]).contiguous()
    return ops.pushpull_fill(x, m)

  def ddim_p_sample_loop_outpaint(self, cond_model_inputs, images, pad, guidance_scale=5., strength=1.0,
                                  masked_content="fill", encode_noise=None, q_noises=None, noises=None, seed=0,
                                  first_sample_index=0, record=None, guidance_interval=None, preview_freq=None,
                                  on_preview=None, attn_maps=None, attn_layers=None, paste_back=False, mask_feather=0.,
                                  color_match=False):
    """Outpainting: `images` [B,H,W,3] (or [H,W,3], tiled) float32 in [-1, 1] grow by `pad` =
    (top, bottom, left, right) pixels (outpaint_geometry: both canvas extents multiples of f * 2^levels).  The images
    are placed on the canvas, the border -- zeros, i.e. grey, with `masked_content` "original" -- is filled with a
    smooth continuation of the images' pixels ("fill", the default; ops.pushpull_fill), the canvas is encoded and the
    masked img2img loop runs on it with the latent mask that keeps the cells lying wholly inside the images
    (latent_mask): the loop of ddim_p_sample_loop_img2img(canvas, mask=...), its graphs, state and launches, with one
    eager fill in front of the encoder.  `paste_back` / `mask_feather` / `color_match` put the
    images' own pixels back after the decode: the originals are the canvas before the fill, the keep is the images'
    box.  The other keywords as in ddim_p_sample_loop_img2img.  Returns the decoded canvas
    [B,H+top+bottom,W+left+right,3]; the final latents stay in self._xt."""
    if masked_content not in MASKED_CONTENTS:
      raise ValueError(f"masked_content must be one of {MASKED_CONTENTS}, got {masked_content!r}")
    paste = self._paste_args(paste_back, mask_feather, color_match, True)
    gsched = self._guidance(guidance_scale, guidance_interval)
    k = img2img_start(strength, len(self._ddim_steps))
    B = len(cond_model_inputs) // 2
    imgs = self._init_images(images, B)
    f, div = self._pixel_factor(), 1 << max(getattr(self._unet, "skip_lvl", (0,)))
    (Hc, Wc), (y0, x0, H, W) = outpaint_geometry(tuple(imgs.shape[1:3]), pad, f, div)
    canvas = torch.zeros(B, Hc, Wc, 3, dtype=torch.float32, device=self.device)
    canvas[:, y0:y0 + H, x0:x0 + W] = imgs.to(self.device)
    keep = np.zeros((1, Hc, Wc), dtype=np.float32)
    keep[:, y0:y0 + H, x0:x0 + W] = 1.
    originals = canvas
    if masked_content == "fill":
      canvas = self._fill_images(canvas, keep)
    mask = self._latent_mask(latent_mask(keep, f)[0], B)
    context = self._cond_stage_model(cond_model_inputs)
    z0 = self.get_latents(canvas, noise=encode_noise, seed=seed, first_sample_index=first_sample_index)
    images = self._sdedit(context, z0, k, guidance_scale, gsched, mask, q_noises, noises, seed, first_sample_index,
                          record, preview_freq=preview_freq, on_preview=on_preview, attn_maps=attn_maps,
                          attn_layers=attn_layers)
    return images if paste is None else self._paste_back(images, originals, keep, *paste)

  # ---- pixel-space paste-back ---------------------------------------------
  @staticmethod
  def _paste_args(paste_back, mask_feather, color_match, has_mask):
    """The checked paste-back keywords as (sigma, color_match), None when `paste_back` is off.  Raises before anything
    is allocated."""
    from .feather import feather_radius
    for name, v in (("paste_back", paste_back), ("color_match", color_match)):
      if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, got {v!r}")
    feather_radius(mask_feather)
    if not paste_back:
      if float(mask_feather) != 0.:
        raise ValueError("mask_feather feathers the seam of the paste-back: it needs paste_back=True")
      if color_match:
        raise ValueError("color_match corrects the decoded image before the paste-back: it needs paste_back=True")
      return None
    if not has_mask:
      raise ValueError("paste_back puts back the pixels a mask keeps: it needs mask")
    return float(mask_feather), bool(color_match)

  def _paste_back(self, images, originals, keep, sigma, color_match):
    """The decoded `images` [B,H,W,3] with the pixels of `originals` that `keep` [B,H,W] (or [1,H,W]; kept iff >= 1)
    keeps put back: ops.mask_feather, ops.keep_stats when `color_match`, ops.paste_back into `images`.  Eager, after
    the decode; no state of the loop's."""
    o = originals.to(self.device, torch.float32).contiguous()
    m = _as_tensor(keep).to(self.device).contiguous()
    w = ops.mask_feather(m, sigma)
    gain = offset = None
    if color_match:
      _, gain, offset = ops.keep_stats(o, images, m)
    self._paste_w, self._paste_cm = w, (gain, offset)
    return ops.paste_back(o, images, w, gain, offset, out=images)

  def last_paste_weights(self):
    """The weight map w [B,H,W] (or [1,H,W], one map for every sample) float32 of the last paste-back: 1 where the
    init images' pixels came back bit for bit, 0 where the decoded image stayed.  None before the first."""
    return getattr(self, "_paste_w", None)

  def last_color_match(self):
    """(gain, offset), [B,3] float32 each, of the last paste-back with color_match=True; (None, None) without it, None
    before the first paste-back."""
    return getattr(self, "_paste_cm", None)

  # ---- two-pass high-resolution sampling --------------------------------
  def ddim_p_sample_loop_hires(self, cond_model_inputs, shape, hires_shape, strength=0.5, resize="bilinear",
                               guidance_scale=5., x_T=None, noises=None, q_noises=None, seed=0, first_sample_index=0,
                               record=None, guidance_interval=None, pixel_filter=None, encode_noise=None,
                               attn_maps=None):
    """Two-pass sampling ("hires fix").  Pass 1 is ddim_p_sample_loop at `shape` [B,h,w,c], the
    U-Net's training size, without the decode.  Its latents are resized to `hires_shape` [B,H,W,c] on the device
    (ops.resize_nhwc; `resize` "nearest", "bilinear" or "bicubic").  Pass 2 is the unmasked img2img loop from those
    latents z0, no encoder involved: k = int(strength * N), start from q_sample(z0, steps[k-1], Q[k-1]), DDIM indices
    k-1 .. 0 at `hires_shape`, decode.  Every solver, step table, guidance schedule and noise source runs in both
    passes; each shape keeps its own state and captured graph, so a second call captures nothing.
    `x_T` [B,h,w,c] is pass 1's; `noises` (read when eta > 0) a pair (pass 1's [N,B,h,w,c], pass 2's [N,B,H,W,c]),
    either may be None; `q_noises` [N,B,H,W,c] is pass 2's Q.  What is not given is drawn from `seed` in pass 1 and
    from hires_seed(seed) in pass 2, so that no draw of one pass repeats a draw of the other.  `record` receives x
    after each of the N + k steps (eager, no graph).  Returns the decoded images [B,fH,fW,3]; the final latents stay
    in self._xt, a copy of pass 1's in self.hires_first_latents.
    `pixel_filter` "triangle", "cubic" or "lanczos3" (None: everything above, unchanged)
    enlarges in pixel space instead: pass 1's latents are decoded to the decoder's float image, the image is
    resampled to f times the extents of `hires_shape` (ops.resample_nhwc) and encoded again (get_latents with
    `encode_noise` [B,H,W,c], else drawn from hires_seed(seed)'s ENCODE_STREAM); those latents are pass 2's z0 and
    `resize` is not used.  Needs an autoencoder with its encoder that decodes at both sizes."""
    self._no_attn_maps(attn_maps, "the hires loop")
    shape, hires_shape = tuple(int(v) for v in shape), tuple(int(v) for v in hires_shape)
    if len(shape) != 4 or len(hires_shape) != 4:
      raise ValueError(f"shape {shape} and hires_shape {hires_shape} must both be [B,h,w,c]")
    if (shape[0], shape[3]) != (hires_shape[0], hires_shape[3]):
      raise ValueError(f"hires_shape {hires_shape} must keep the batch and channels of shape {shape}")
    if resize not in RESIZE_MODES:
      raise ValueError(f"resize must be one of {RESIZE_MODES}, got {resize!r}")
    div = 1 << max(getattr(self._unet, "skip_lvl", (0,)))
    if hires_shape[1] < 1 or hires_shape[2] < 1 or hires_shape[1] % div or hires_shape[2] % div:
      raise ValueError(f"hires_shape {hires_shape}: the U-Net halves its input {div.bit_length() - 1} times, the "
                       f"extents must be positive multiples of {div}")
    if pixel_filter is not None:
      check_filter(pixel_filter, "pixel_filter")
      if getattr(self._autoencoder, "_encoder", None) is None:
        raise ValueError("pixel_filter encodes the resampled image: the autoencoder was built without its encoder "
                         "(pass with_encoder=True)")
      bound = getattr(self._autoencoder, "_latent_size", None)
      if bound is not None and shape[1:3] != hires_shape[1:3]:
        raise ValueError(f"pixel_filter decodes at {shape[1:3]} and at {hires_shape[1:3]}: this autoencoder was built "
                         f"for the one latent size {bound}")
    elif encode_noise is not None:
      raise ValueError("encode_noise is the noise of pixel_filter's encode: it cannot be given without pixel_filter")
    n = len(self._ddim_steps)
    k = img2img_start(strength, n)
    noises1, noises2 = (None, None) if noises is None else noises
    gsched = self._guidance(guidance_scale, guidance_interval)
    context = self._cond_stage_model(cond_model_inputs)
    first = self._sample_from(context, shape, n, guidance_scale, gsched, x_T, noises1, seed, first_sample_index,
                              record, decode=False)
    self.hires_first_latents = first.clone()   # (pass 2 reuses the buffer when both shapes are the same)
    self._hires_events = (self._loop_events, None)
    if pixel_filter is None:
      z0 = ops.resize_nhwc(first, hires_shape[1:3], resize)
    else:
      image = self.decode_first_stage(first)   # (the decoder's float image: no min-max, no uint8)
      f = image.shape[1] // shape[1]
      image = ops.resample_nhwc(image, (f * hires_shape[1], f * hires_shape[2]), pixel_filter)
      z0 = self.get_latents(image, noise=encode_noise, seed=hires_seed(seed), first_sample_index=first_sample_index)
    images = self._sdedit(context, z0, k, guidance_scale, gsched, None, q_noises, noises2, hires_seed(seed),
                          first_sample_index, record)
    self._hires_events = (self._hires_events[0], self._loop_events)
    return images

  def last_hires_ms(self):
    """(ms of pass 1's loop, ms of pass 2's loop) of the last ddim_p_sample_loop_hires call: device time, all steps of
    each (synchronises)."""
    out = []
    for t0, t1, _ in self._hires_events:
      t1.synchronize()
      out.append(t0.elapsed_time(t1))
    return tuple(out)

  def _init_images(self, init_images, B):
    """init_images [B,H,W,3] (or [H,W,3], tiled over the batch) as a contiguous float32 tensor."""
    imgs = _as_tensor(init_images)
    if imgs.dim() == 3:
      imgs = imgs[None].expand(B, *imgs.shape)
    if imgs.dim() != 4 or imgs.shape[0] != B or imgs.shape[-1] != 3:
      raise ValueError(f"init_images must be [B={B},H,W,3] or [H,W,3], got {tuple(imgs.shape)}")
    return imgs.contiguous()

  @staticmethod
  def _latent_mask(mask, B, hw=None):
    """A latent mask [B,h,w] (or [h,w], tiled over the batch) as a float32 tensor; with `hw` = (h, w), the latents'
    extents, checked against them."""
    mask = _as_tensor(mask)
    if mask.dim() == 2:
      mask = mask[None].expand(B, *mask.shape)
    if hw is not None and tuple(mask.shape) != (B, *hw):
      raise ValueError(f"mask must be [B,h,w] = {(B, *hw)} (or [h,w]) at latent resolution, "
                       f"got {tuple(mask.shape)}")
    return mask

  # ---- init images and masks of any size ------------------------------
  def _pixel_factor(self):
    """Image pixels per latent cell along an axis: the autoencoder halves len(multipliers) - 1 times (1 for an
    autoencoder that does not say)."""
    mult = getattr(self._autoencoder, "_multipliers", None)
    return 1 if mult is None else 2 ** (len(mult) - 1)

  def _image_size(self, image_size, fit, resample):
    """The checked `image_size` keyword as (H, W), None when it was not given.  Raises before anything is allocated:
    an unknown `fit` or filter, or extents that are not positive multiples of f * 2^levels (f the autoencoder's
    pixels per latent cell, levels the U-Net's halvings)."""
    if image_size is None:
      return None
    if fit not in FITS:
      raise ValueError(f"fit must be one of {FITS}, got {fit!r}")
    check_filter(resample, "resample")
    if np.ndim(image_size) != 1 or len(image_size) != 2 or any(int(v) != v for v in image_size):
      raise ValueError(f"image_size must be (H, W) in pixels, got {image_size!r}")
    H, W = (int(v) for v in image_size)
    f, div = self._pixel_factor(), 1 << max(getattr(self._unet, "skip_lvl", (0,)))
    if H < 1 or W < 1 or H % (f * div) or W % (f * div):
      raise ValueError(f"image_size {(H, W)}: the autoencoder maps {f} pixels to a latent cell and the U-Net halves "
                       f"its input {div.bit_length() - 1} times, the extents must be positive multiples of {f * div}")
    return H, W

  def _fit_images(self, imgs, size, fit, resample):
    """init images [B,Hs,Ws,3] -> [B,H,W,3] on the device: the crop box (`fit` "crop"), then ops.resample_nhwc.
    Images that already are (H, W) come back as they are (the host tensor: the encoder's path of today)."""
    src = tuple(int(v) for v in imgs.shape[1:3])
    if src == tuple(size):
      return imgs
    x = imgs.to(self.device)
    if fit == "crop":
      y0, x0, hc, wc = crop_box(src, size)
      x = x[:, y0:y0 + hc, x0:x0 + wc]
    return ops.resample_nhwc(x.contiguous(), size, resample)

  def _fit_mask(self, mask, src, size, fit):
    """`mask` with image_size=: a latent mask ([B,h,w] or [h,w], (h, w) = size / f) is returned as given; a pixel
    mask at the source images' extents `src` becomes the latent mask of the same box the images keep
    (latent_mask_fit); any other shape is a ValueError."""
    f = self._pixel_factor()
    h, w = size[0] // f, size[1] // f
    shape = tuple(int(v) for v in np.shape(mask))
    if len(shape) in (2, 3) and shape[-2:] == (h, w):
      return mask
    if len(shape) not in (2, 3) or shape[-2:] != tuple(src):
      raise ValueError(f"mask of shape {shape} is neither a latent mask [B,{h},{w}] (or [{h},{w}]) nor a pixel mask "
                       f"at the init images' size [B,{src[0]},{src[1]}] (or [{src[0]},{src[1]}])")
    m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask)
    if fit == "crop" and tuple(src) != tuple(size):
      y0, x0, hc, wc = crop_box(src, size)
      m = m[..., y0:y0 + hc, x0:x0 + wc]
    lm = latent_mask_fit(m, (h, w))
    return lm[0] if len(shape) == 2 else lm

  # ---- DDIM inversion ---------------------------------------------------
  def inversion_timesteps(self):
    """t_in [N] int32: the training timestep of the level below DDIM index i, where the inversion step at index i
    evaluates the U-Net: t_in[0] = 0, t_in[i] = steps[i-1], so that abar[t_in[i]] == a_prev[i]."""
    return np.concatenate([[0], self._ddim_steps[:-1]]).astype(np.int32)

  def _invert_tables(self):
    """The inversion's own device tables, made on first use.  The loop counter only ever walks down (the U-Net's
    first launch pre-decrements it), so both tables are stored reversed: row N-1-i holds inversion index i.  (coef
    rows, t_in as the step table of the four temb launches)."""
    if self._inv_tbl is None:
      t_rev = np.ascontiguousarray(self.inversion_timesteps()[::-1])
      self._inv_tbl = (self._coef_dev.flip(0).contiguous(), torch.from_numpy(t_rev).to(self.device))
    return self._inv_tbl

  def _invert_temb_kwargs(self, dec_index):
    """_temb_kwargs for an inversion step: the temb table of the reversed t_in (built on first use)."""
    if self._inv_temb is None and hasattr(self._unet, "temb_table") and self._use_temb_table:
      self._inv_temb = self._unet.temb_table(self._invert_tables()[1]).clone()
    self._pre_dec = self._inv_temb is not None
    if self._inv_temb is None:
      return {}
    return dict(temb_table=self._inv_temb, pre_decrement=bool(dec_index))

  def _invert_counter_start(self):
    """Value of the device counter before the first inversion step, whatever the depth: the step at inversion index
    i reads row N-1-i, and a pre-decrementing step starts one above its row.  After k steps it holds this - k."""
    self._invert_temb_kwargs(True)
    n = len(self._ddim_steps)
    return n if self._pre_dec else n - 1

  def _step_invert(self, guidance_scale, dec_index, pred_x0_out=None):
    """One inversion step: the U-Net at t_in on the level x is on, then ldm_cfg_ddim_invert_update.  A scale of
    exactly 1 with skip_unguided: the conditional rows x2[B:] against the resident context's rows B .. 2B-1 and the
    conditional-only update; else the paired 2B rows and the scaled update.  Either writes both halves of x2."""
    B = self._xt.shape[0]
    coef, t_rev = self._invert_tables()
    cond_only = float(guidance_scale) == 1. and self._skip_unguided
    kw = self._invert_temb_kwargs(dec_index)
    if cond_only:
      self._unet.forward(self._x2[B:], steps=t_rev, index=self._index_dev, out=self._eps[B:], paired_rows=False,
                         context_rows=(B, 2 * B), **kw)
    else:
      self._unet.forward(self._x2, steps=t_rev, index=self._index_dev, out=self._eps, paired_rows=True, **kw)
    ops.cfg_ddim_invert_update(self._eps, self._xt, self._xt, coef, self._index_dev, not cond_only, guidance_scale,
                               x_unet_out=self._x2, dec_index=dec_index and not self._pre_dec,
                               pred_x0_out=pred_x0_out)

  def ddim_invert_loop(self, cond_model_inputs, init_images=None, latents=None, guidance_scale=1., strength=1.,
                       encode_noise=None, seed=0, first_sample_index=0, record=None, image_size=None,
                       fit="stretch", resample="lanczos3", attn_maps=None, trajectory=False):
    """DDIM inversion: the deterministic, first-order DDIM ODE run upwards from z0, whatever
    sampler= and eta the sampler was built with.  cond_model_inputs: token ids [uncond x B; cond x B].  Exactly one
    of `init_images` ([B,H,W,3] or [H,W,3], tiled; float32 in [-1, 1]; z0 = get_latents(init_images, encode_noise))
    and `latents` (z0 [B,h,w,c], already scaled).  k = int(strength * N) as for img2img; the loop runs inversion
    indices 0 .. k-1: e = eps(x, t_in[i]) with the guidance scale (1: the conditional eps alone), x0 = (x -
    sqrt(1 - a_prev[i]) e) / sqrt(a_prev[i]), x <- (x0 + c2[i] e) / c1[i].  `record` receives x after each step
    (eager, no graph).  Returns the latents on the level of steps[k-1], float32 [B,h,w,c] on the device (a copy;
    they also stay in self._xt): ddim_p_sample_loop(x_T=, start_index=k) maps them back.  `image_size` / `fit` /
    `resample` as in ddim_p_sample_loop_img2img, with `init_images` only.
    `trajectory=True`: every step also stores its output, the latents on the level of steps[j]
    for the inversion index j, into row j of a table [N,B,h,w,c] the sampler owns -- one ldm_store_row launch after
    the update, inside the captured step, in a graph slot of its own; last_trajectory() returns the k rows.  False:
    the launches, the graph and its key are what they were."""
    self._no_attn_maps(attn_maps, "the inversion loop")
    size = self._image_size(image_size, fit, resample)
    if np.ndim(guidance_scale) > 0:
      raise ValueError("the inversion loop takes one float guidance_scale: a guidance schedule is not supported")
    guidance_scale = float(guidance_scale)
    k = img2img_start(strength, len(self._ddim_steps))
    B = len(cond_model_inputs) // 2
    z0 = self._edit_z0(init_images, latents, B, size, fit, resample, encode_noise, seed, first_sample_index)
    context = self._cond_stage_model(cond_model_inputs)
    _, h, w, c = z0.shape
    self._alloc_state(B, h, w, c)
    self._set_context(context)
    z0_buf = self._owned("_z0_buf", z0, (B, h, w, c))
    self._invert_tables()                      # (made before any capture: the graph reads them at fixed addresses)

    def reset():
      self._copy_start(z0_buf)
      self._index_dev.fill_(self._invert_counter_start())

    cond_only = guidance_scale == 1. and self._skip_unguided
    # (the scale is an argument of the captured launch, and the conditional-only form has none; the depth k is not
    # in the key: the counter is on the device)
    gkey = ("invert", None if cond_only else guidance_scale, self._ctx_shape, self._step_spacing)
    if trajectory:
      n = len(self._ddim_steps)
      if getattr(self, "_traj", None) is None:
        self._traj = torch.zeros(n, B, h, w, c, dtype=torch.float32, device=self.device)
        self._clear_slots("_invt_graph", "_de_graph")

      def step(dec):
        # after the update the counter holds N-1-j when the U-Net's first launch pre-decremented it and one less when
        # the update itself moved it (temb_table=False); the uncounted warm-up step moves nothing
        self._step_invert(guidance_scale, dec)
        ops.store_row(self._xt, self._traj, self._index_dev, index_sign=-1,
                      index_bias=n - 1 - (1 if dec and not self._pre_dec else 0))

      self._sample_loop(k, reset, step, gkey + ("trajectory",), record, slot="_invt_graph")
      self._traj_last = (k, self._traj)
      return self._xt.clone()
    self._sample_loop(k, reset, lambda dec: self._step_invert(guidance_scale, dec), gkey, record, slot="_inv_graph")
    return self._xt.clone()

  def last_trajectory(self):
    """The trajectory of the last ddim_invert_loop(trajectory=True): float32 [k,B,h,w,c] on the device, row j the
    latents on the level of steps[j] (a copy of the table's first k rows)."""
    if self._traj_last is None:
      raise ValueError("no inversion has run with trajectory=True")
    k, traj = self._traj_last
    return traj[:k].clone()

  def ddim_p_sample_loop_edit(self, source_inputs, target_inputs, init_images, guidance_scale=5., strength=0.75,
                              invert_guidance_scale=1., encode_noise=None, noises=None, seed=0, first_sample_index=0,
                              record=None, guidance_interval=None, image_size=None, fit="stretch",
                              resample="lanczos3", attn_maps=None):
    """Prompt editing of a real image: z0 = get_latents(init_images); k = int(strength * N)
    inversion steps under the source prompt (`source_inputs`, scale `invert_guidance_scale`); then DDIM indices
    k-1 .. 0 of the configured solver under the target prompt (`target_inputs`, `guidance_scale` /
    `guidance_interval` as in ddim_p_sample_loop).  Both id arrays are [uncond x B; cond x B].  With the same ids and
    both scales 1 this reconstructs the image.  `record` receives x after each sampling step.  `image_size` / `fit` /
    `resample` as in ddim_p_sample_loop_img2img.  Returns the decoded images; the final latents
    stay in self._xt."""
    self._no_attn_maps(attn_maps, "the edit loop")
    self._image_size(image_size, fit, resample)
    if np.shape(source_inputs) != np.shape(target_inputs):
      raise ValueError(f"source_inputs {np.shape(source_inputs)} and target_inputs {np.shape(target_inputs)} must "
                       "have the same shape")
    k = img2img_start(strength, len(self._ddim_steps))
    x = self.ddim_invert_loop(source_inputs, init_images=init_images, guidance_scale=invert_guidance_scale,
                              strength=strength, encode_noise=encode_noise, seed=seed,
                              first_sample_index=first_sample_index, image_size=image_size, fit=fit,
                              resample=resample)
    return self.ddim_p_sample_loop(target_inputs, tuple(x.shape), guidance_scale, x_T=x, noises=noises, seed=seed,
                                   first_sample_index=first_sample_index, record=record,
                                   guidance_interval=guidance_interval, start_index=k)

  # ---- DiffEdit -----------------------------------------------------------
  def _diffedit_args(self, source_inputs, target_inputs, mask_strength, num_maps, mask_threshold, mask_clamp_ratio,
                     mask_dilate):
    """The checked mask keywords -> (k_m, n, tau, dilate); raises before anything is allocated."""
    if np.shape(source_inputs) != np.shape(target_inputs):
      raise ValueError(f"source_inputs {np.shape(source_inputs)} and target_inputs {np.shape(target_inputs)} must "
                       "have the same shape")
    if isinstance(num_maps, bool) or int(num_maps) != num_maps or int(num_maps) < 1:
      raise ValueError(f"num_maps must be an int of at least 1, got {num_maps!r}")
    if isinstance(mask_dilate, bool) or int(mask_dilate) != mask_dilate or not 0 <= int(mask_dilate) <= 3:
      raise ValueError(f"mask_dilate must be an int in [0, 3], got {mask_dilate!r}")
    try:
      k_m = img2img_start(mask_strength, len(self._ddim_steps))
    except ValueError as e:
      raise ValueError(f"mask_strength: {e}") from None
    tau = float(mask_threshold) * float(mask_clamp_ratio)
    if not np.isfinite(tau) or tau < 0.:
      raise ValueError(f"mask_threshold * mask_clamp_ratio must be finite and not negative, got {mask_threshold!r} * "
                       f"{mask_clamp_ratio!r}")
    return k_m, int(num_maps), tau, int(mask_dilate)

  def _edit_z0(self, init_images, latents, B, size, fit, resample, encode_noise, seed, first_sample_index):
    """z0 [B,h,w,c] float32 of exactly one of `init_images` (get_latents, after image_size=) and `latents`."""
    if (init_images is None) == (latents is None):
      raise ValueError("exactly one of init_images and latents must be given")
    if latents is None:
      imgs = self._init_images(init_images, B)
      if size is not None:
        imgs = self._fit_images(imgs, size, fit, resample)
      return self.get_latents(imgs, noise=encode_noise, seed=seed, first_sample_index=first_sample_index)
    if size is not None:
      raise ValueError("image_size resamples init_images: it cannot be given with latents")
    z0 = _as_tensor(latents)
    if z0.dim() != 4 or z0.shape[0] != B:
      raise ValueError(f"latents must be [B={B},h,w,c], got {tuple(z0.shape)}")
    return z0

  def diffedit_mask(self, source_inputs, target_inputs, init_images=None, latents=None, mask_strength=0.5, num_maps=10,
                    mask_threshold=0.5, mask_clamp_ratio=3., mask_dilate=0, map_noises=None, encode_noise=None, seed=0,
                    first_sample_index=0, image_size=None, fit="stretch", resample="lanczos3"):
    """DiffEdit's mask (Couairon et al. 2022): where the source and the target prompt disagree
    about the noise in an image.  Both id arrays are [uncond x B; cond x B]; exactly one of `init_images` and `latents`
    gives z0.  k_m = int(mask_strength * N), t_m = steps[k_m - 1]; for each of n = `num_maps` draws r (in this order)
    x_r = q_sample(z0, t_m, M[r]), one paired U-Net evaluation of [x_r; x_r] against [source cond x B; target cond x B]
    and acc[b,p] += sum_j |e_tgt - e_src| (ldm_eps_contrast_accum): one captured step replayed n times.  M is
    `map_noises` [n,B,h,w,c], else drawn per global sample index from the streams MAP_STREAM + r (by ldm_normal_fill
    when the noise source is "device").  Then ldm_contrast_mask: edit = acc > tau * (the sample's mean of acc), tau =
    mask_threshold * mask_clamp_ratio (HF diffusers' clamp(map, 0, ratio mean) / (ratio mean) > threshold with the
    mean per sample), dilated by `mask_dilate` cells (0..3).  Returns the mask float32 [B,h,w] on the device, 1 = keep
    (a copy); last_contrast_map() has the map and the statistics.  `image_size` / `fit` / `resample` as in
    ddim_p_sample_loop_img2img, with `init_images` only."""
    size = self._image_size(image_size, fit, resample)
    k_m, n, tau, dilate = self._diffedit_args(source_inputs, target_inputs, mask_strength, num_maps, mask_threshold,
                                              mask_clamp_ratio, mask_dilate)
    B = len(source_inputs) // 2
    z0 = self._edit_z0(init_images, latents, B, size, fit, resample, encode_noise, seed, first_sample_index)
    return self._diffedit_mask(source_inputs, target_inputs, z0, k_m, n, tau, dilate, map_noises, seed,
                               first_sample_index).clone()

  def _diffedit_mask(self, source_inputs, target_inputs, z0, k_m, n, tau, dilate, map_noises, seed, first_sample_index):
    """diffedit_mask from z0 on; returns the sampler's own mask buffer."""
    B, h, w, c = (int(v) for v in z0.shape)
    if not ops.contrast_mask_supported(h, w, dilate):
      raise ValueError(f"the mask kernel takes latents of at most 65536 cells, got {h} x {w}")
    ids = np.concatenate([np.asarray(source_inputs)[B:], np.asarray(target_inputs)[B:]], axis=0)
    context = self._cond_stage_model(ids)
    self._alloc_state(B, h, w, c)
    self._set_context(context)
    z0_buf = self._owned("_z0_buf", z0, (B, h, w, c))
    # the draw table is stored reversed, as the inversion's tables are: the draw counter only walks down (from n - 1),
    # and row n-1-r holds draw r, so the draws run r = 0 .. n-1
    if map_noises is None and self._noise_source == "device":
      buf = getattr(self, "_dm_noise", None)
      if buf is None or tuple(buf.shape) != (n, B, h, w, c):
        buf = self._dm_noise = torch.zeros(n, B, h, w, c, dtype=torch.float32, device=self.device)
        self._drop_graphs()
      rng = self._set_rng(seed, first_sample_index)
      for r in range(n):
        ops.normal_fill(buf[n - 1 - r], rng, MAP_STREAM + r)
    else:
      if map_noises is None:
        map_noises = np.stack([normal_latents(seed, first_sample_index, B, (h, w, c), stream=MAP_STREAM + r)
                               for r in range(n)])
      m = _as_tensor(map_noises)
      if tuple(m.shape) != (n, B, h, w, c):
        raise ValueError(f"map_noises: shape {tuple(m.shape)}, expected {(n, B, h, w, c)}")
      buf = self._owned("_dm_noise", m.flip(0), (n, B, h, w, c))
    t_m = self._owned("_dm_t", np.full(B, self._ddim_steps[k_m - 1]), (B,), dtype=torch.int32)
    if getattr(self, "_dm_acc", None) is None:
      self._dm_acc = torch.zeros(B, h, w, dtype=torch.float32, device=self.device)
      self._dm_out = (torch.empty(B, h, w, dtype=torch.float32, device=self.device),
                      torch.empty(B, dtype=torch.float32, device=self.device),
                      torch.empty(B, dtype=torch.float32, device=self.device),
                      torch.empty(B, dtype=torch.int32, device=self.device))
      self._clear_slots("_dm_graph")
    if self._dm_counters is None:
      self._dm_counters = torch.zeros(2, dtype=torch.int32, device=self.device)
    t_index, draw = self._dm_counters[0:1], self._dm_counters[1:2]
    sa, sb, _ = self._device_q_tables()
    acc, stride = self._dm_acc, buf[0].numel()

    def reset():
      t_index.fill_(k_m - 1)                   # (the U-Net's time index: read, never moved)
      draw.fill_(n - 1)
      acc.zero_()                              # (outside the graph: the warm-up and capture steps added theirs)

    def step(dec):
      ops.q_sample(z0_buf, buf, t_m, sa, sb, self._xt, x_unet_out=self._x2, index=draw, noise_index_stride=stride)
      kw = dict(self._temb_kwargs(False))
      self._unet.forward(self._x2, steps=self._steps_dev, index=t_index, out=self._eps, paired_rows=True, **kw)
      ops.eps_contrast_accum(self._eps, acc, counter=draw if dec else None)

    gkey = ("diffedit_map", self._ctx_shape, self._step_spacing)
    self._sample_loop(n, reset, step, gkey, None, slot="_dm_graph")
    mask, mean, thr, count = self._dm_out
    ops.contrast_mask(acc, mask, tau, dilate, mean_out=mean, thr_out=thr, count_out=count)
    self._dm_last = (n, c, acc, self._dm_out)
    return mask

  def last_contrast_map(self):
    """Of the last mask estimate: dict(map= float32 [B,h,w], acc / (c n): the mean absolute difference of the two
    prompts' eps per cell; mask= float32 [B,h,w], 1 = keep; mean=, threshold= float32 [B] in acc's units (the scale
    1 / (c n) cancels in the rule); edited= int32 [B], the edited cells after dilation), all NumPy.  Synchronises."""
    if self._dm_last is None:
      raise ValueError("no contrast map has been estimated")
    n, c, acc, (mask, mean, thr, count) = self._dm_last
    return dict(map=(acc / float(c * n)).cpu().numpy(), mask=mask.cpu().numpy(), mean=mean.cpu().numpy(),
                threshold=thr.cpu().numpy(), edited=count.cpu().numpy())

  def ddim_p_sample_loop_diffedit(self, source_inputs, target_inputs, init_images, guidance_scale=5., strength=0.75,
                                  invert_guidance_scale=1., mask=None, mask_strength=0.5, num_maps=10,
                                  mask_threshold=0.5, mask_clamp_ratio=3., mask_dilate=0, map_noises=None,
                                  encode_noise=None, noises=None, record=None, seed=0, first_sample_index=0,
                                  image_size=None, fit="stretch", resample="lanczos3", guidance_interval=None,
                                  preview_freq=None, on_preview=None, attn_maps=None, attn_layers=None):
    """DiffEdit: the prompt edit of ddim_p_sample_loop_edit kept inside a mask.  z0 =
    get_latents(init_images), once; the mask is diffedit_mask's estimate on z0 (its keywords above) unless `mask`
    (latent [B,h,w] or [h,w], 1 = keep) is given; k = int(strength * N) inversion steps under the source prompt keep
    their trajectory traj[0 .. k-1]; sampling starts from traj[k-1] under the target prompt with the configured solver,
    and before the step at every index i < k-1, x <- m traj[i] + (1 - m) x -- the update launch's own blend reading
    the trajectory for Q under the coefficients (0, 1), so a kept cell is traj[i] bit for bit; nothing is blended at
    index 0.  Every solver, step table and noise source; the eta noise comes from `noises` or the loop's table.
    `record` receives x after each sampling step (eager, no graph).  A guidance schedule or interval, previews and
    attn_maps do not combine with it.  Returns the decoded images; the final latents stay in self._xt."""
    if np.ndim(guidance_scale) > 0 or guidance_interval is not None:
      raise ValueError("the DiffEdit loop takes one float guidance_scale: a guidance schedule (a sequence "
                       "guidance_scale or guidance_interval) is not supported")
    if preview_freq is not None or on_preview is not None:
      raise ValueError("preview_freq and the DiffEdit loop do not combine")
    if attn_layers is not None and attn_maps is None:
      raise ValueError("attn_layers needs attn_maps")
    self._no_attn_maps(attn_maps, "the DiffEdit loop")
    size = self._image_size(image_size, fit, resample)
    k_m, n_maps, tau, dilate = self._diffedit_args(source_inputs, target_inputs, mask_strength, num_maps,
                                                   mask_threshold, mask_clamp_ratio, mask_dilate)
    n = len(self._ddim_steps)
    k = img2img_start(strength, n)
    B = len(source_inputs) // 2
    z0 = self._edit_z0(init_images, None, B, size, fit, resample, encode_noise, seed, first_sample_index)
    _, h, w, c = z0.shape
    if mask is None:
      mask = self._diffedit_mask(source_inputs, target_inputs, z0, k_m, n_maps, tau, dilate, map_noises, seed,
                                 first_sample_index)
    else:
      mask = self._latent_mask(mask, B, (h, w))
    # (every buffer the sampler owns is settled before the inversion captures: a new one drops the shape's graphs)
    self._alloc_state(B, h, w, c)
    self._owned("_mask_buf", mask, (B, h, w))
    if self._de_qcoef is None:
      self._de_qcoef = torch.tensor([[0., 1.]] * n, dtype=torch.float32, device=self.device).contiguous()
    noise_table = self._eta_noise_table(noises, seed, first_sample_index, B, h, w, c)
    self.ddim_invert_loop(source_inputs, latents=z0, guidance_scale=invert_guidance_scale, strength=strength,
                          trajectory=True)
    context = self._cond_stage_model(target_inputs)
    self._set_context(context)
    start = self._traj[k - 1]

    self._blend_traj = True
    try:
      return self._denoise(k, lambda: self._copy_start(start), guidance_scale, None, noise_table, True, False, record)
    finally:
      self._blend_traj = False

  # ---- panorama ---------------------------------------------------------
  def _alloc_windows(self, B, n_win, h, w, c):
    """The window batch: the U-Net's input and output rows [uncond ; cond] x B x n_win, float32 (the U-Net's input
    dtype).  A new address drops the captured graphs."""
    key = (B, n_win, h, w, c)
    if getattr(self, "_win_key", None) != key:
      rows = 2 * B * n_win
      self._x_win = torch.empty(rows, h, w, c, dtype=torch.float32, device=self.device)
      self._eps_win = torch.empty(rows, h, w, c, dtype=torch.float32, device=self.device)
      self._win_key = key
      self._drop_graphs()

  def _step_panorama(self, guidance_scale, noise_table, dec_index, window, stride, rng=False, wrap=(False, False),
                     weights=None):
    """gather(canvas) -> unet(window rows) -> fold(eps) -> the solver's update on the canvas.  The update writes no
    U-Net input: the next step's gather reads the canvas.  A wrapped axis or `weights` = (wy, wx) device tables
     makes the gather and the fold the _ex pair; otherwise the calls are section 12's."""
    B, H, W, c = self._xt.shape
    ex = any(wrap) or weights is not None
    if ex:
      ops.window_gather_ex(self._xt, self._x_win, window, stride, wrap)
    else:
      ops.window_gather(self._xt, self._x_win, window, stride)
    self._unet.forward(self._x_win, steps=self._steps_dev, index=self._index_dev, out=self._eps_win, paired_rows=True,
                       **self._temb_kwargs(dec_index))
    if ex:
      ops.window_fold_ex(self._eps_win, self._eps.view(2, B, H, W, c), window, stride, wrap, weights)
    else:
      ops.window_fold(self._eps_win, self._eps.view(2, B, H, W, c), window, stride)
    self._update(guidance_scale, False, noise_table, dec_index, None, rng=rng)

  def _finish_wrapped(self, latents, pad):
    """_finish for a wrapped canvas: the decoder's zero-padded convolutions see across the wrap
    through `pad` = (py, px) cells of circular padding, whose pixels are cropped from the images."""
    py, px = pad
    B, H, W, c = (int(v) for v in latents.shape)
    try:
      images = self._finish(ops.wrap_pad(latents, pad) if py or px else latents)
    except LdmHipError as e:
      raise ValueError(f"the decoder cannot decode a canvas of shape {[B, H + 2 * py, W + 2 * px, c]}: {e}") from e
    if not (py or px):
      return images
    f = self._pixel_factor()
    return images[:, py * f:(py + H) * f, px * f:(px + W) * f].contiguous()

  def ddim_p_sample_loop_panorama(self, cond_model_inputs, shape, window, stride=None, guidance_scale=5., x_T=None,
                                  noises=None, seed=0, first_sample_index=0, record=None, guidance_interval=None,
                                  wrap=(False, False), window_weights="uniform", wrap_decode_margin=0, attn_maps=None):
    """MultiDiffusion (Bar-Tal et al. 2023) on the loop of ddim_p_sample_loop.  `shape` is the
    canvas [B,H,W,c]; `window` = (h, w) the size the U-Net runs at; `stride` = (sy, sx), default half the window
    (at least 1); one int means both axes.  Windows lie at window_origins() along each axis, the last one clamped to the edge.  Every step
    evaluates the U-Net on the 2 * B * nW window rows and steps the canvas once with the mean eps of the windows
    covering each cell.  x_T, noises ([N,B,H,W,c]), seed and record are the canvas's, as in ddim_p_sample_loop; every
    sampler=, step table and noise source runs.  A window equal to the canvas is ddim_p_sample_loop bit for bit.
    `guidance_scale` is one float: schedules (a sequence, `guidance_interval`) are not supported here.
    Seamless panoramas: `wrap` = (wrap_y, wrap_x) lays the windows of a wrapped axis at
    wrap_origins(), crossing the edge and coming back on the other side.  `window_weights`: "uniform" (the plain
    mean), "tent", "gaussian" (window_profile) or a pair of positive arrays (wy [h], wx [w]): the fold is the mean
    weighted by wy[jy] * wx[jx] at each window element.  `wrap_decode_margin`: latent cells of circular padding the
    decoder sees on each side of a wrapped axis (cropped from the images; 0 = the plain decode)."""
    self._no_attn_maps(attn_maps, "the panorama loop")
    if np.ndim(guidance_scale) > 0 or guidance_interval is not None:
      raise ValueError("the panorama loop takes one float guidance_scale: a sequence guidance_scale or a "
                       "guidance_interval is not supported")
    B, H, W, c = (int(s) for s in shape)
    (h, w), (sy, sx) = window_and_stride(window, stride)
    wrap = wrap_pair(wrap)
    # (ValueError: no such grid)
    n_win = (len((wrap_origins if wrap[0] else window_origins)(H, h, sy)) *
             len((wrap_origins if wrap[1] else window_origins)(W, w, sx)))
    profile, tables = window_weight_tables(window_weights, (h, w))
    margin = int(wrap_decode_margin)
    if margin != wrap_decode_margin or margin < 0:
      raise ValueError(f"wrap_decode_margin must be an int of at least 0, got {wrap_decode_margin!r}")
    pad = (margin if wrap[0] else 0, margin if wrap[1] else 0)
    if pad[0] > H or pad[1] > W:
      raise ValueError(f"wrap_decode_margin {margin} exceeds the canvas extent along a wrapped axis ({H}x{W})")
    context = self._cond_stage_model(cond_model_inputs)
    n = len(self._ddim_steps)
    xt = self._x_T(x_T, seed, first_sample_index, B, H, W, c)
    self._alloc_state(B, H, W, c)
    self._alloc_windows(B, n_win, h, w, c)
    weights = None
    if tables is not None:                           # (owned: the captured fold reads them at fixed addresses)
      weights = (self._owned("_win_wy", tables[0], (h,)), self._owned("_win_wx", tables[1], (w,)))
    # row (half, b, k) of the window batch attends to context[half * B + b]
    context = torch.as_tensor(context).to(self.device)
    if context.shape[0] != 2 * B:
      raise ValueError(f"cond_model_inputs gives {context.shape[0]} context rows, the canvas batch needs {2 * B}")
    self._set_context(torch.cat([context[:B].repeat_interleave(n_win, 0), context[B:].repeat_interleave(n_win, 0)]))
    rng = self._draws_on_device(noises)
    noise_table = None if rng else self._eta_noise_table(noises, seed, first_sample_index, B, H, W, c)

    def reset():
      # (the first gather reads the canvas: no [xt; xt] copies)
      if self._noise_source == "device":
        self._set_rng(seed, first_sample_index)
      if xt is None:
        ops.normal_fill(self._xt, self._rng, XT_STREAM)
      else:
        self._xt.copy_(xt)
      self._start_counters(n)

    gkey = ("panorama", (B, H, W, c), (h, w), (sy, sx), float(guidance_scale), noise_table is not None,
            self._ctx_shape, False, self._noise_source, rng, self._step_spacing, self._sampler, wrap, profile)
    self._sample_loop(n, reset, lambda dec: self._step_panorama(guidance_scale, noise_table, dec, (h, w), (sy, sx),
                                                                rng=rng, wrap=wrap, weights=weights), gkey, record)
    return self._finish_wrapped(self._xt, pad)

  def ddim_p_sample_loop_progressive(self, cond_model_inputs, shape, guidance_scale=5.,
                                     record_freq=5, x_T=None, noises=None, seed=0,
                                     first_sample_index=0, guidance_interval=None, attn_maps=None):
    """Intended semantics of model_runners.py:511-575 (the reference version calls a method
    that does not exist, :535, and returns three values to a caller unpacking two,
    run_ldm_sampler.py:90 -- neither bug is reproduced).  Runs the same loop as
    ddim_p_sample_loop and keeps, for each record slot r < N // record_freq, the sample and
    the predicted x0 of the LAST step whose index // record_freq == r (the reference's
    insert_mask overwrites a slot on every such step, :545-553), i.e. of index r*record_freq.
    Returns (images [B,H,W,3], sample_progress [B,R,H,W,3], pred_x0_progress [B,R,H,W,3]),
    all decoded with decode_first_stage.  `guidance_scale` / `guidance_interval` as in ddim_p_sample_loop."""
    self._no_attn_maps(attn_maps, "the progressive sampler")
    gsched = self._guidance(guidance_scale, guidance_interval)
    B, h, w, c = (int(s) for s in shape)
    context = self._cond_stage_model(cond_model_inputs)
    n = len(self._ddim_steps)
    num_records = n // record_freq
    xt = self._x_T(x_T, seed, first_sample_index, B, h, w, c)
    self._alloc_state(B, h, w, c)
    self._set_context(context)
    rng = self._draws_on_device(noises)
    noise_table = None if rng else self._eta_noise_table(noises, seed, first_sample_index, B, h, w, c)
    self._set_x_T(xt, seed, first_sample_index, B)
    self._start_counters(n)
    sample_prog = torch.zeros(B, num_records, h, w, c, dtype=torch.float32, device=self.device)
    x0_prog = torch.zeros_like(sample_prog)
    pred_x0 = torch.empty_like(self._xt)
    for index in range(n - 1, -1, -1):
      if gsched is not None:
        self._step_sched(bool(gsched[index] != 1.), True, pred_x0_out=pred_x0, rng=rng)
      else:
        self._step(guidance_scale, False, noise_table, dec_index=True, pred_x0_out=pred_x0, rng=rng)
      r = index // record_freq
      if r < num_records:                      # later (smaller) indices overwrite the slot
        sample_prog[:, r].copy_(self._xt)
        x0_prog[:, r].copy_(pred_x0)
    images = self.decode_first_stage(self._xt)
    flat = (B * num_records, h, w, c)
    # the decoder chunks large batches itself (B * N // record_freq frames: 160 at B=4, N=200)
    sp = self.decode_first_stage(sample_prog.reshape(flat))
    sp = sp.reshape(B, num_records, *sp.shape[1:])
    xp = self.decode_first_stage(x0_prog.reshape(flat))
    xp = xp.reshape(B, num_records, *xp.shape[1:])
    return images, sp, xp

  def last_loop_ms_per_step(self):
    """Device time of the last DDIM loop divided by its step count (synchronises)."""
    t0, t1, n = self._loop_events
    t1.synchronize()
    return t0.elapsed_time(t1) / n
