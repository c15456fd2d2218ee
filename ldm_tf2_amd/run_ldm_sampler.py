"""Sampler harness: YAML -> three models -> prompt tokens -> DDIM loop -> images.npy.

Same I/O contract as the reference CLI (run_ldm_sampler.py:49-99): reads the YAML
sections `ldm_sampling`, `pre_ckpt_paths`, `cond_stage_model`, `autoencoder_kl|vq`,
`unet`, `ldm` (keys == constructor kwargs), tiles the prompt into ids
[uncond x B; cond x B], samples, converts with the per-image min-max rule
(:18-25) and writes uint8 NHWC `images.npy`.

    python -m ldm_tf2_amd.run_ldm_sampler --config_path all_in_one_config.yaml \
        [--dtype bf16|f32] [--seed 0] [--out images.npy]

Checkpoints: the reference restores TF checkpoints with expect_partial(), which
silently leaves random-init weights when nothing matches.
TF checkpoints cannot be read here; `pre_ckpt_paths` entries that point at an
`.npz` of reference-layout arrays (weights.py names) are loaded, and an extra key
`pre_ckpt_paths.compvis` naming the original PyTorch checkpoint loads all three models
through checkpoint.py; anything else falls back to seeded random init with a warning --
the same observable behaviour.

img2img / inpainting: optional `ldm_sampling` keys `init_image` (a .npy of uint8 [H,W,3] or
[B,H,W,3], read as x/127.5 - 1), `strength` (default 0.75) and `mask` (a .npy [H,W] or
[B,H,W], nonzero = keep; needs `init_image`).  With `init_image` the autoencoder is built
or loaded with its encoder.  Without these keys nothing changes.

Solver: optional `ldm_sampling` key `sampler`, `ddim` (default), `plms` (pseudo linear multistep, needs
`ldm.eta` 0) or `deis` (the same step with weights computed for the step table walked, needs
`ldm.eta` 0); every loop above honours it.

Step table: optional `ldm_sampling` key `step_spacing`, `uniform` (default: the reference's table), `logsnr` or
`karras`; every loop and every solver runs on any of them.

Noise: optional `ldm_sampling` key `noise_source`, `host` (default: NumPy generators, tables uploaded before the loop)
or `device` (Philox streams drawn inside the update launches, no tables).  The two sources draw
different numbers from the same `--seed`.

Guidance schedule: `ldm_sampling.guidance_scale` may be a list of `ldm.num_ddim_steps` floats (one per DDIM index), and
the optional key `ldm_sampling.guidance_interval: [t_lo, t_hi]` (training timesteps, inclusive) guides only the steps
inside it; steps whose scale is 1 evaluate the U-Net on the conditional rows alone (needs `ldm.eta` 0; DESIGN.md
section 11).  Every loop above honours both.

Panorama: optional `ldm_sampling` keys `window: [h, w]` and `window_stride: [sy, sx]` (default: half the window).  With
`window`, `latent_shape` is a canvas larger than the U-Net's training size: every step runs the U-Net on overlapping
`window`-sized crops of the canvas and averages their predictions where they overlap (MultiDiffusion; DESIGN.md
section 12).  Every solver, step table and noise source runs; `init_image`, `mask`, `sample_save_progress`,
`guidance_interval` and a list `guidance_scale` cannot be combined with it.  Without `window` nothing changes.
Seamless panoramas, each key needing `window`: `window_wrap: [wrap_y, wrap_x]` (bools) lets the
windows of an axis cross the edge and come back on the other side (a 360-degree panorama, a tileable texture);
`window_weights: uniform | tent | gaussian` weights each window by a profile that falls off towards its border instead
of the plain mean; `wrap_decode_margin: m` decodes the canvas with m latent cells of circular padding on each side of
a wrapped axis and crops them from the images, so the decoder sees across the wrap column.

Prompt editing: optional `ldm_sampling` key `source_prompt` (a string; needs `init_image`).  The init image is encoded,
inverted `int(strength * N)` DDIM steps under `source_prompt` (DDIM inversion, guidance scale `invert_guidance_scale`,
default 1) and sampled back under `text_prompt`, the target, with `guidance_scale`.  The same
prompt twice with both scales 1 reconstructs the image.  `mask`, `window` and `sample_save_progress` cannot be combined
with it.  Without `source_prompt` nothing changes.

DiffEdit: optional `ldm_sampling` key `edit_mask: auto` (needs `source_prompt` and `init_image`).
The edit stays inside a mask estimated from the two prompts: `edit_mask_maps` (default 10) noise draws at
`edit_mask_strength` (default 0.5) of the schedule give a map of where the prompts' noise predictions differ, cells
above `edit_mask_threshold` (0.5) times `edit_mask_clamp_ratio` (3.0) times the map's mean are edited, grown by
`edit_mask_dilate` (0..3, default 0) cells, and every other cell follows the image's own inversion.  Each of the five
keys needs `edit_mask`; `guidance_interval` and a list `guidance_scale` cannot be combined with it.  Without `edit_mask`
nothing changes.

Two-pass high resolution ("hires fix"): optional `ldm_sampling` keys `hires_shape: [B, H, W, c]`, `hires_strength`
(default 0.5) and `hires_resize` (`nearest`, `bilinear` (default) or `bicubic`).  With `hires_shape`, `latent_shape` is
sampled as usual, the latents are resized to `hires_shape` on the device and the last `int(hires_strength * N)` DDIM
steps run again at that size from the re-noised latents; the images are decoded at
`hires_shape`.  Every solver, step table, noise source and guidance schedule runs in both passes; `init_image`, `mask`,
`window`, `source_prompt` and `sample_save_progress` cannot be combined with it.  Without `hires_shape` nothing changes.

Init images and masks of any size: optional `ldm_sampling` keys `init_fit`, `exact` (default:
`init_image` must already have f times the extents of `latent_shape`, as above), `stretch` (the whole image is resampled to
that size on the device) or `crop` (its centred box of that aspect ratio is), and `init_filter`, `triangle`, `cubic` or
`lanczos3` (default), the antialiased filter.  With `stretch` or `crop`, `mask` may be a pixel mask at the init image's
own size.  Optional key `hires_pixel_filter` (the same three names; needs `hires_shape`): the two-pass loop enlarges
in pixel space -- decode, resample, encode -- instead of resizing the latents, and the autoencoder is built with its
encoder.  Without these keys nothing changes.

Latent previews: optional `ldm_sampling` key `preview_freq: q` (an int of at least 1).  Every step
whose DDIM index is a multiple of q also writes a small RGB picture of the current latents and of the predicted x_0 --
an affine map of the latent channels to RGB, an upscale and an 8-bit quantisation, one extra launch inside the captured
step -- and main() saves the two strips, uint8 [B,R,H,W,3], as `preview_sample.npy` and `preview_x0.npy` beside `--out`.
`preview_scale` (default: the autoencoder's downsampling factor, so a preview has the image's size), `preview_mode`
(`nearest` or `bilinear`, the default) and `preview_matrix` (a .npy of float32 [c+1,3]: c weight rows, then the bias;
default: fitted on the decoder with a few noise latents, which is rough -- tools/fit_preview.py fits one on a run's
latents) each need `preview_freq`.  The txt2img and img2img loops take it; `window`, `hires_shape`, `source_prompt` and
`sample_save_progress` cannot be combined with it.  Without `preview_freq` nothing changes.

Cross-attention heat maps: optional `ldm_sampling` key `attention_maps: true`.  Every U-Net
evaluation of the loop also adds the head-averaged cross-attention probabilities of the prompt's rows into one
accumulator per transformer block -- one extra launch per block inside the captured step -- and main() saves the
per-token maps, float32 [B,Tk,H,W], as `attention_maps.npy` and the prompt's words with their token positions as
`attention_words.json` beside `--out` (model_runners.word_heatmaps sums a word's maps).  `attention_map_steps:
[i_lo, i_hi]` (an inclusive range of DDIM indices; default: all) restricts the steps that count,
`attention_map_size: [H, W]` (default: the latent size) is the size the maps are resized to; both need
`attention_maps`.  The txt2img and img2img loops take it; `guidance_interval`, a list `guidance_scale`,
`preview_freq`, `window`, `hires_shape`, `source_prompt` and `sample_save_progress` cannot be combined with it.
Without `attention_maps` nothing changes.

Outpainting and masked content: optional `ldm_sampling` key `outpaint: [top, bottom, left,
right]` (pixels, each at least 0 and not all 0; needs `init_image`).  The init image is placed on a canvas that many
pixels larger -- `latent_shape` is the canvas's, so the grown image must have f times its extents -- the new border is
filled with a smooth continuation of the image (a push-pull image pyramid on the device), and the masked img2img loop
regenerates the border while it keeps the image; `strength` defaults to 1.0 here.  `mask`, `window`, `hires_shape`,
`source_prompt`, `sample_save_progress` and an `init_fit` other than `exact` cannot be combined with it.  Optional key
`masked_content`, `original` (default: a regenerated region starts from the init image's own content, as above) or
`fill` (it starts from the same smooth continuation of the kept pixels; needs `mask` or `outpaint`, where it is the
default); needs `init_image`, and `source_prompt` cannot be combined with it.  Without these keys nothing changes.

Paste-back: optional `ldm_sampling` keys `paste_back: true` (after the decode the init image's
own pixels are put back bit for bit wherever the mask keeps them), `mask_feather: sigma` (pixels, 0 .. 16: the seam is
hidden by a ramp that lies inside the kept region) and `color_match: true` (the decoded image first gets the
per-channel gain and offset that bring its mean and variance over the kept pixels to the init image's); the last two
need `paste_back`.  Each needs `init_image` and `mask` or `outpaint`; `source_prompt`, `window` and `hires_shape`
cannot be combined with them.  Three eager launches after the decode; without these keys nothing changes.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import yaml

from . import ops
from .autoencoder import AutoencoderKL, AutoencoderVQ
from ._lib import RESAMPLE_FILTERS
from .model_runners import (FITS, MASKED_CONTENTS, PREVIEW_MODES, RESIZE_MODES, WINDOW_WEIGHTS,
                            LatentDiffusionModelSampler, latent_mask, window_and_stride)
from .tokenizer import get_token_ids
from .transformer import TransformerModel
from .unet import UNet


def tensor_to_image(images):
  """run_ldm_sampler.py:18-25 on the device: per image (x-min)/(max-min)*255 ->
  uint8 (truncation).  Returns a NumPy uint8 array."""
  x = images.contiguous()
  out = torch.empty(tuple(x.shape), dtype=torch.uint8, device=x.device)
  ops.minmax_u8(x, out)
  return out.cpu().numpy()


_preloaded = {}


def _load_weights(path, what):
  if what in _preloaded:
    return _preloaded.pop(what)
  if path and os.path.isfile(path) and path.endswith(".npz"):
    return dict(np.load(path))
  print(f"[WARN] no loadable checkpoint for {what} at {path!r}: using random-init weights "
        "(the reference's expect_partial() behaviour)", file=sys.stderr)
  return None


def compvis_manifest_configs(config):
  """Manifest kwargs of the three models as `build_from_config` will build them (what a CompVis
  checkpoint must be mapped onto): U-Net with the text model's hidden size as context width, the
  autoencoder section the sampler selects, for VQ with the run-time latent size and codebook."""
  kind = config["ldm_sampling"]["autoencoder_type"]
  unet_cfg = dict(config["unet"], context_dim=config["cond_stage_model"]["hidden_size"])
  if kind == "kl":
    ae_cfg = dict(config["autoencoder_kl"], attention_resolutions=())      # KL ignores it (autoencoder.py:339)
  else:
    ae_cfg = dict(config["autoencoder_vq"], latent_size=decode_latent_size(config))
  return dict(unet_cfg=unet_cfg, transformer_cfg=dict(config["cond_stage_model"]), autoencoder_cfg=ae_cfg)


def needs_encoder(config):
  """img2img (`ldm_sampling.init_image`) encodes its init image, and the two-pass loop with
  `ldm_sampling.hires_pixel_filter` its resampled first pass: the autoencoder is built with its encoder."""
  samp = config["ldm_sampling"]
  return bool(samp.get("init_image")) or samp.get("hires_pixel_filter") is not None


def _filter_name(samp, key, default=None):
  name = samp.get(key, default)
  if name is not None and name not in RESAMPLE_FILTERS:
    raise ValueError(f"ldm_sampling.{key} must be one of {RESAMPLE_FILTERS}, got {name!r}")
  return name


def init_fit_kwargs(config):
  """`ldm_sampling.init_fit` / `init_filter` (the reference's YAML has no such keys) as the
  image-driven loops' keywords: nothing for `exact` (default), else the target size f * `latent_shape`'s extents,
  the fit and the filter."""
  samp = config["ldm_sampling"]
  fit = samp.get("init_fit", "exact")
  if fit not in ("exact",) + FITS:
    raise ValueError(f"ldm_sampling.init_fit must be one of {('exact',) + FITS}, got {fit!r}")
  resample = _filter_name(samp, "init_filter", "lanczos3")
  if fit == "exact":
    return {}
  f = downsampling_factor(config)
  return dict(image_size=(f * samp["latent_shape"][1], f * samp["latent_shape"][2]), fit=fit, resample=resample)


def downsampling_factor(config):
  kind = config["ldm_sampling"]["autoencoder_type"]
  mult = config["autoencoder_kl" if kind == "kl" else "autoencoder_vq"].get(
      "multipliers", (1, 2, 4, 4) if kind == "kl" else (1, 2, 2, 4))
  return 2 ** (len(mult) - 1)


def sampler_name(config):
  """`ldm_sampling.sampler`: "ddim" (default; the reference's YAML has no such key) or "plms" (DESIGN.md section 8)."""
  return config["ldm_sampling"].get("sampler", "ddim")


def step_spacing_name(config):
  """`ldm_sampling.step_spacing`: "uniform" (default; the reference's YAML has no such key), "logsnr" or "karras"
  (DESIGN.md section 10)."""
  return config["ldm_sampling"].get("step_spacing", "uniform")


def noise_source_name(config):
  """`ldm_sampling.noise_source`: "host" (default; the reference's YAML has no such key) or "device" (DESIGN.md
  section 9)."""
  return config["ldm_sampling"].get("noise_source", "host")


def guidance_kwargs(config):
  """`ldm_sampling.guidance_interval: [t_lo, t_hi]` as the loops' keyword (nothing when the key is absent; the
  reference's YAML has no such key).  `ldm_sampling.guidance_scale` itself may be a float or a list (DESIGN.md
  section 11) and is passed on as it is."""
  iv = config["ldm_sampling"].get("guidance_interval")
  if iv is None:
    return {}
  if not isinstance(iv, (list, tuple)) or len(iv) != 2:
    raise ValueError(f"ldm_sampling.guidance_interval must be [t_lo, t_hi], got {iv!r}")
  return dict(guidance_interval=(iv[0], iv[1]))


def panorama_kwargs(config, seed):
  """`ldm_sampling.window: [h, w]` / `window_stride: [sy, sx]` (default: half the window) as the panorama loop's
  keywords (the reference's YAML has no such keys).  The loop has no init image, mask, progress
  frames or guidance schedule."""
  samp = config["ldm_sampling"]
  for key in ("init_image", "mask", "sample_save_progress", "guidance_interval"):
    if samp.get(key) is not None and samp.get(key) is not False:
      raise ValueError(f"ldm_sampling.window cannot be combined with ldm_sampling.{key}")
  if np.ndim(samp["guidance_scale"]) > 0:
    raise ValueError("ldm_sampling.window needs one float guidance_scale, not a list")
  for key in ("window", "window_stride"):
    v = samp.get(key)
    if v is not None and (not isinstance(v, (list, tuple)) or len(v) != 2):
      raise ValueError(f"ldm_sampling.{key} must be a pair of ints, got {v!r}")
  window, stride = window_and_stride(samp["window"], samp.get("window_stride"))
  return dict(window=window, stride=stride, seed=seed, **panorama_wrap_kwargs(config))


PANORAMA_WRAP_KEYS = ("window_wrap", "window_weights", "wrap_decode_margin")


def panorama_wrap_kwargs(config):
  """`ldm_sampling.window_wrap: [bool, bool]`, `window_weights: uniform | tent | gaussian` and `wrap_decode_margin:
  int` as the panorama loop's keywords (the reference's YAML has no such keys); nothing for a
  key that is absent."""
  samp = config["ldm_sampling"]
  kwargs = {}
  v = samp.get("window_wrap")
  if v is not None:
    if not isinstance(v, (list, tuple)) or len(v) != 2 or any(not isinstance(x, bool) for x in v):
      raise ValueError(f"ldm_sampling.window_wrap must be a pair of bools [wrap_y, wrap_x], got {v!r}")
    kwargs["wrap"] = (v[0], v[1])
  v = samp.get("window_weights")
  if v is not None:
    if v not in WINDOW_WEIGHTS:
      raise ValueError(f"ldm_sampling.window_weights must be one of {WINDOW_WEIGHTS}, got {v!r}")
    kwargs["window_weights"] = v
  v = samp.get("wrap_decode_margin")
  if v is not None:
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
      raise ValueError(f"ldm_sampling.wrap_decode_margin must be an int of at least 0, got {v!r}")
    kwargs["wrap_decode_margin"] = v
  return kwargs


def hires_call(config, token_ids, seed):
  """`ldm_sampling.hires_shape: [B, H, W, c]` with `hires_strength` / `hires_resize` (the
  reference's YAML has no such keys): the two-pass loop's call.  The loop has no init image, mask, windows, source
  prompt or progress frames."""
  samp = config["ldm_sampling"]
  for key in ("init_image", "mask", "window", "source_prompt", "sample_save_progress"):
    if samp.get(key) is not None and samp.get(key) is not False:
      raise ValueError(f"ldm_sampling.hires_shape cannot be combined with ldm_sampling.{key}")
  hs = samp["hires_shape"]
  if not isinstance(hs, (list, tuple)) or len(hs) != 4 or any(not isinstance(v, int) for v in hs):
    raise ValueError(f"ldm_sampling.hires_shape must be [B, H, W, c] (ints), got {hs!r}")
  resize = samp.get("hires_resize", "bilinear")
  if resize not in RESIZE_MODES:
    raise ValueError(f"ldm_sampling.hires_resize must be one of {RESIZE_MODES}, got {resize!r}")
  kwargs = dict(strength=float(samp.get("hires_strength", 0.5)), resize=resize, guidance_scale=samp["guidance_scale"],
                seed=seed, **guidance_kwargs(config))
  if _filter_name(samp, "hires_pixel_filter") is not None:
    kwargs["pixel_filter"] = samp["hires_pixel_filter"]
  return "ddim_p_sample_loop_hires", (token_ids, samp["latent_shape"], list(hs)), kwargs


def decode_latent_size(config):
  """The latent extent the autoencoder decodes at: `hires_shape`'s when the key is there, else `latent_shape`'s."""
  samp = config["ldm_sampling"]
  return (samp.get("hires_shape") or samp["latent_shape"])[1]


def _init_images(samp):
  """`ldm_sampling.init_image`: a .npy of uint8 [H,W,3] or [B,H,W,3], read as x / 127.5 - 1."""
  img = np.load(samp["init_image"])
  if img.dtype != np.uint8 or img.ndim not in (3, 4) or img.shape[-1] != 3:
    raise ValueError(f"init_image must be uint8 [H,W,3] or [B,H,W,3], got {img.dtype} {img.shape}")
  return img.astype(np.float32) / np.float32(127.5) - np.float32(1.0)


def edit_call(config, token_ids, source_ids, seed):
  """`ldm_sampling.source_prompt` (the reference's YAML has no such key): the edit loop's call.
  `source_ids`: the source prompt's token ids, laid out like `token_ids` (the target's)."""
  samp = config["ldm_sampling"]
  if not isinstance(samp["source_prompt"], str):
    raise ValueError(f"ldm_sampling.source_prompt must be a string, got {samp['source_prompt']!r}")
  for key in ("mask", "window", "sample_save_progress"):
    if samp.get(key) is not None and samp.get(key) is not False:
      raise ValueError(f"ldm_sampling.source_prompt cannot be combined with ldm_sampling.{key}")
  if not samp.get("init_image"):
    raise ValueError("ldm_sampling.source_prompt needs ldm_sampling.init_image")
  if source_ids is None:
    raise ValueError("ldm_sampling.source_prompt is set: its token ids are needed")
  kwargs = dict(strength=float(samp.get("strength", 0.75)),
                invert_guidance_scale=float(samp.get("invert_guidance_scale", 1.)), seed=seed,
                **guidance_kwargs(config), **init_fit_kwargs(config))
  em = edit_mask_kwargs(config)
  if em is not None:
    return ("ddim_p_sample_loop_diffedit", (source_ids, token_ids, _init_images(samp), samp["guidance_scale"]),
            dict(kwargs, **em))
  return "ddim_p_sample_loop_edit", (source_ids, token_ids, _init_images(samp), samp["guidance_scale"]), kwargs


# `edit_mask_*` key -> (the DiffEdit loop's keyword, its type)
EDIT_MASK_KEYS = {"edit_mask_strength": ("mask_strength", float), "edit_mask_maps": ("num_maps", int),
                  "edit_mask_threshold": ("mask_threshold", float), "edit_mask_clamp_ratio": ("mask_clamp_ratio", float),
                  "edit_mask_dilate": ("mask_dilate", int)}


def edit_mask_kwargs(config):
  """`ldm_sampling.edit_mask: auto` with `edit_mask_strength` / `edit_mask_maps` / `edit_mask_threshold` /
  `edit_mask_clamp_ratio` / `edit_mask_dilate` (the reference's YAML has no such keys), checked:
  None without `edit_mask`, else the DiffEdit loop's mask keywords (those of the keys given; the loop has the
  defaults).  The mask belongs to the prompt edit with one float guidance scale."""
  samp = config["ldm_sampling"]
  on = samp.get("edit_mask")
  if on is None:
    for key in EDIT_MASK_KEYS:
      if samp.get(key) is not None:
        raise ValueError(f"ldm_sampling.{key} needs ldm_sampling.edit_mask")
    return None
  if on != "auto":
    raise ValueError(f"ldm_sampling.edit_mask must be 'auto', got {on!r}")
  for key in ("source_prompt", "init_image"):
    if not samp.get(key):
      raise ValueError(f"ldm_sampling.edit_mask needs ldm_sampling.{key}")
  if samp.get("guidance_interval") is not None:
    raise ValueError("ldm_sampling.edit_mask cannot be combined with ldm_sampling.guidance_interval")
  if np.ndim(samp["guidance_scale"]) > 0:
    raise ValueError("ldm_sampling.edit_mask cannot be combined with a list ldm_sampling.guidance_scale")
  out = {}
  for key, (name, kind) in EDIT_MASK_KEYS.items():
    v = samp.get(key)
    if v is None:
      continue
    ok = isinstance(v, int) and not isinstance(v, bool) if kind is int else \
        isinstance(v, (int, float)) and not isinstance(v, bool)
    if not ok:
      raise ValueError(f"ldm_sampling.{key} must be {'an int' if kind is int else 'a number'}, got {v!r}")
    out[name] = kind(v)
  if "num_maps" in out and out["num_maps"] < 1:
    raise ValueError(f"ldm_sampling.edit_mask_maps must be at least 1, got {out['num_maps']!r}")
  if "mask_dilate" in out and not 0 <= out["mask_dilate"] <= 3:
    raise ValueError(f"ldm_sampling.edit_mask_dilate must be in [0, 3], got {out['mask_dilate']!r}")
  if "mask_strength" in out and not 0. < out["mask_strength"] <= 1.:
    raise ValueError(f"ldm_sampling.edit_mask_strength must be in (0, 1], got {out['mask_strength']!r}")
  for key in ("edit_mask_threshold", "edit_mask_clamp_ratio"):
    name = EDIT_MASK_KEYS[key][0]
    if name in out and not (np.isfinite(out[name]) and out[name] >= 0.):
      raise ValueError(f"ldm_sampling.{key} must be finite and not negative, got {out[name]!r}")
  return out


PREVIEW_KEYS = ("preview_scale", "preview_mode", "preview_matrix")


def preview_settings(config):
  """`ldm_sampling.preview_freq` with `preview_scale` / `preview_mode` / `preview_matrix` (the
  reference's YAML has no such keys), checked: None without `preview_freq`, else dict(freq=, scale=, mode=, matrix=
  the .npy's path or None).  The previews belong to the txt2img and img2img loops."""
  samp = config["ldm_sampling"]
  q = samp.get("preview_freq")
  if q is None:
    for key in PREVIEW_KEYS:
      if samp.get(key) is not None:
        raise ValueError(f"ldm_sampling.{key} needs ldm_sampling.preview_freq")
    return None
  if isinstance(q, bool) or not isinstance(q, int) or q < 1:
    raise ValueError(f"ldm_sampling.preview_freq must be an int of at least 1, got {q!r}")
  for key in ("window", "hires_shape", "source_prompt", "sample_save_progress"):
    if samp.get(key) is not None and samp.get(key) is not False:
      raise ValueError(f"ldm_sampling.preview_freq cannot be combined with ldm_sampling.{key}")
  scale = samp.get("preview_scale", downsampling_factor(config))
  if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= 16:
    raise ValueError(f"ldm_sampling.preview_scale must be an int in [1, 16], got {scale!r}")
  mode = samp.get("preview_mode", "bilinear")
  if mode not in PREVIEW_MODES:
    raise ValueError(f"ldm_sampling.preview_mode must be one of {PREVIEW_MODES}, got {mode!r}")
  matrix = samp.get("preview_matrix")
  if matrix is not None and not isinstance(matrix, str):
    raise ValueError(f"ldm_sampling.preview_matrix must be the path of a .npy, got {matrix!r}")
  return dict(freq=q, scale=scale, mode=mode, matrix=matrix)


def preview_kwargs(config):
  """The loops' keyword of `ldm_sampling.preview_freq`: nothing when the key is absent."""
  pv = preview_settings(config)
  return {} if pv is None else dict(preview_freq=pv["freq"])


def setup_preview(sampler, config, seed):
  """Hands the sampler the previews' matrix, scale and mode before the loop: `preview_matrix`'s .npy, else a matrix
  fitted on the decoder at `latent_shape` (fit_preview).  Nothing without `preview_freq`."""
  pv = preview_settings(config)
  if pv is None:
    return
  if pv["matrix"] is not None:
    proj = np.load(pv["matrix"])
    c = config["ldm_sampling"]["latent_shape"][3]
    if proj.dtype != np.float32 or proj.shape != (c + 1, 3):
      raise ValueError(f"preview_matrix must be float32 [{c + 1},3], got {proj.dtype} {proj.shape}")
  else:
    proj = sampler.fit_preview(seed=seed, shape=config["ldm_sampling"]["latent_shape"][1:])
  sampler.set_preview(proj, scale=pv["scale"], mode=pv["mode"])


ATTENTION_MAP_KEYS = ("attention_map_steps", "attention_map_size")


def attention_map_settings(config):
  """`ldm_sampling.attention_maps` with `attention_map_steps` / `attention_map_size` (the
  reference's YAML has no such keys), checked: None without `attention_maps`, else dict(weights= the loops' attn_maps
  value, size= (H, W) or None).  The maps belong to the txt2img and img2img loops with one float guidance scale."""
  samp = config["ldm_sampling"]
  on = samp.get("attention_maps")
  if on is None or on is False:
    for key in ATTENTION_MAP_KEYS:
      if samp.get(key) is not None:
        raise ValueError(f"ldm_sampling.{key} needs ldm_sampling.attention_maps")
    return None
  if on is not True:
    raise ValueError(f"ldm_sampling.attention_maps must be true or false, got {on!r}")
  for key in ("guidance_interval", "preview_freq", "window", "hires_shape", "source_prompt", "sample_save_progress"):
    if samp.get(key) is not None and samp.get(key) is not False:
      raise ValueError(f"ldm_sampling.attention_maps cannot be combined with ldm_sampling.{key}")
  if np.ndim(samp["guidance_scale"]) > 0:
    raise ValueError("ldm_sampling.attention_maps cannot be combined with a list ldm_sampling.guidance_scale")
  is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
  n = config["ldm"]["num_ddim_steps"] if "num_ddim_steps" in config.get("ldm", {}) else None
  weights = True
  rng = samp.get("attention_map_steps")
  if rng is not None:
    if not isinstance(rng, (list, tuple)) or len(rng) != 2 or not all(is_int(v) for v in rng) or not 0 <= rng[0] <= rng[1]:
      raise ValueError(f"ldm_sampling.attention_map_steps must be [i_lo, i_hi] with 0 <= i_lo <= i_hi, got {rng!r}")
    if n is None:
      raise ValueError("ldm_sampling.attention_map_steps needs ldm.num_ddim_steps")
    if rng[1] >= n:
      raise ValueError(f"ldm_sampling.attention_map_steps {rng!r} exceeds the {n} DDIM indices")
    weights = [1.0 if rng[0] <= i <= rng[1] else 0.0 for i in range(n)]
  size = samp.get("attention_map_size")
  if size is not None:
    if not isinstance(size, (list, tuple)) or len(size) != 2 or not all(is_int(v) and v >= 1 for v in size):
      raise ValueError(f"ldm_sampling.attention_map_size must be [H, W] of positive ints, got {size!r}")
    size = (size[0], size[1])
  return dict(weights=weights, size=size)


def attention_map_kwargs(config):
  """The loops' keyword of `ldm_sampling.attention_maps`: nothing when the key is absent."""
  am = attention_map_settings(config)
  return {} if am is None else dict(attn_maps=am["weights"])


def outpaint_pad(config):
  """`ldm_sampling.outpaint: [top, bottom, left, right]` (pixels; the reference's YAML has no
  such key), checked: None without the key, else the outpaint loop's `pad`.  The loop grows `init_image`; it has no
  mask of the caller's, windows, second pass, source prompt or progress frames, and takes the image as it is."""
  samp = config["ldm_sampling"]
  pad = samp.get("outpaint")
  if pad is None:
    return None
  if not isinstance(pad, (list, tuple)) or len(pad) != 4 or \
      any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in pad) or not any(pad):
    raise ValueError("ldm_sampling.outpaint must be [top, bottom, left, right], ints of at least 0 and not all 0, "
                     f"got {pad!r}")
  if not samp.get("init_image"):
    raise ValueError("ldm_sampling.outpaint needs ldm_sampling.init_image")
  for key in ("mask", "window", "hires_shape", "source_prompt", "sample_save_progress"):
    if samp.get(key) is not None and samp.get(key) is not False:
      raise ValueError(f"ldm_sampling.outpaint cannot be combined with ldm_sampling.{key}")
  if samp.get("init_fit", "exact") != "exact":
    raise ValueError("ldm_sampling.outpaint cannot be combined with ldm_sampling.init_fit")
  return tuple(pad)


def masked_content_name(config):
  """`ldm_sampling.masked_content: original | fill` (the reference's YAML has no such key),
  checked: None without the key.  It belongs to the img2img loop with a mask and to the outpaint loop."""
  samp = config["ldm_sampling"]
  mc = samp.get("masked_content")
  if mc is None:
    return None
  if mc not in MASKED_CONTENTS:
    raise ValueError(f"ldm_sampling.masked_content must be one of {MASKED_CONTENTS}, got {mc!r}")
  if not samp.get("init_image"):
    raise ValueError("ldm_sampling.masked_content needs ldm_sampling.init_image")
  if samp.get("source_prompt") is not None:
    raise ValueError("ldm_sampling.masked_content cannot be combined with ldm_sampling.source_prompt")
  if mc == "fill" and samp.get("mask") is None and samp.get("outpaint") is None:
    raise ValueError("ldm_sampling.masked_content 'fill' needs ldm_sampling.mask or ldm_sampling.outpaint")
  return mc


PASTE_BACK_KEYS = ("paste_back", "mask_feather", "color_match")


def paste_back_kwargs(config):
  """`ldm_sampling.paste_back: true`, `mask_feather: sigma` (pixels, 0 .. 16) and `color_match: true` (DESIGN.md
  section 22; the reference's YAML has no such keys), checked: the loops' keywords, nothing without the keys.  They
  belong to the img2img loop with a mask and to the outpaint loop; `mask_feather` and `color_match` need `paste_back`."""
  from .feather import feather_radius
  samp = config["ldm_sampling"]
  out = {}
  for key in PASTE_BACK_KEYS:
    v = samp.get(key)
    if v is None:
      continue
    if key == "mask_feather":
      if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"ldm_sampling.mask_feather must be a number of pixels in [0, 16], got {v!r}")
      try:
        feather_radius(v)
      except ValueError:
        raise ValueError(f"ldm_sampling.mask_feather must be a number of pixels in [0, 16], got {v!r}") from None
      v = float(v)
    elif not isinstance(v, bool):
      raise ValueError(f"ldm_sampling.{key} must be true or false, got {v!r}")
    if not samp.get("init_image"):
      raise ValueError(f"ldm_sampling.{key} needs ldm_sampling.init_image")
    if samp.get("mask") is None and samp.get("outpaint") is None:
      raise ValueError(f"ldm_sampling.{key} needs ldm_sampling.mask or ldm_sampling.outpaint")
    for other in ("source_prompt", "window", "hires_shape"):
      if samp.get(other) is not None:
        raise ValueError(f"ldm_sampling.{key} cannot be combined with ldm_sampling.{other}")
    out[key] = v
  if not out.get("paste_back"):
    for key in ("mask_feather", "color_match"):
      if out.get(key):
        raise ValueError(f"ldm_sampling.{key} needs ldm_sampling.paste_back")
  return out


def outpaint_call(config, token_ids, seed, extra):
  """The outpaint loop's call: `init_image` grown by `outpaint` must have f times the extents of `latent_shape`."""
  samp = config["ldm_sampling"]
  pad = outpaint_pad(config)
  images = _init_images(samp)
  f = downsampling_factor(config)
  want = (f * samp["latent_shape"][1], f * samp["latent_shape"][2])
  got = (images.shape[-3] + pad[0] + pad[1], images.shape[-2] + pad[2] + pad[3])
  if got != want:
    raise ValueError(f"ldm_sampling.outpaint: init_image {images.shape[-3:-1]} grown by {list(pad)} is {got}, "
                     f"latent_shape needs {want}")
  kwargs = dict(strength=float(samp.get("strength", 1.0)), seed=seed, **guidance_kwargs(config), **extra)
  mc = masked_content_name(config)
  if mc is not None:
    kwargs["masked_content"] = mc
  kwargs.update(paste_back_kwargs(config))
  return "ddim_p_sample_loop_outpaint", (token_ids, images, pad, samp["guidance_scale"]), kwargs


def sampling_call(config, token_ids, seed, source_ids=None):
  """(sampler method name, positional args, kwargs) of the call main() makes for `config`.  `source_ids`: the token
  ids of `ldm_sampling.source_prompt` when the key is there."""
  samp = config["ldm_sampling"]
  base = (token_ids, samp["latent_shape"], samp["guidance_scale"])
  init_fit_kwargs(config)                        # (ValueError: an unknown init_fit or init_filter, whatever the loop)
  preview = preview_kwargs(config)               # (ValueError: a loop without previews, or a key without preview_freq)
  preview.update(attention_map_kwargs(config))   # (the heat maps go where the previews go, and refuse the same loops)
  edit_mask_kwargs(config)                       # (ValueError: a key without edit_mask, edit_mask without its prompt)
  outpaint = outpaint_pad(config)                # (ValueError: a loop that cannot outpaint, whatever the order below)
  masked_content = masked_content_name(config)
  paste = paste_back_kwargs(config)              # (ValueError: a loop without a paste-back, whatever the order below)
  for key in PANORAMA_WRAP_KEYS:
    if samp.get(key) is not None and samp.get("window") is None:
      raise ValueError(f"ldm_sampling.{key} needs ldm_sampling.window")
  if samp.get("hires_shape") is not None:
    return hires_call(config, token_ids, seed)
  if samp.get("hires_pixel_filter") is not None:
    raise ValueError("ldm_sampling.hires_pixel_filter needs ldm_sampling.hires_shape")
  if samp.get("source_prompt") is not None:
    return edit_call(config, token_ids, source_ids, seed)
  if samp.get("window") is not None:
    return "ddim_p_sample_loop_panorama", base, panorama_kwargs(config, seed)
  if samp.get("mask") is not None and not samp.get("init_image"):
    raise ValueError("ldm_sampling.mask needs ldm_sampling.init_image")
  if outpaint is not None:
    return outpaint_call(config, token_ids, seed, preview)
  if samp.get("init_image"):
    if samp.get("sample_save_progress"):
      raise ValueError("sample_save_progress is not supported with init_image")
    images = _init_images(samp)
    fit = init_fit_kwargs(config)
    kwargs = dict(strength=float(samp.get("strength", 0.75)), seed=seed, **guidance_kwargs(config), **fit, **preview)
    if samp.get("mask") is not None:
      pm = np.load(samp["mask"])
      if fit:
        kwargs["mask"] = pm                                     # (at the init image's size: the loop fits it)
      else:
        lm = latent_mask(pm, downsampling_factor(config))
        kwargs["mask"] = lm[0] if pm.ndim == 2 else lm          # [h,w]: one mask, tiled over the batch
    if masked_content is not None:
      kwargs["masked_content"] = masked_content
    kwargs.update(paste)
    return "ddim_p_sample_loop_img2img", (token_ids, images, samp["guidance_scale"]), kwargs
  if samp.get("sample_save_progress"):
    return "ddim_p_sample_loop_progressive", base, dict(seed=seed, **guidance_kwargs(config))
  return "ddim_p_sample_loop", base, dict(seed=seed, **guidance_kwargs(config), **preview)


def build_from_config(config, dtype=torch.bfloat16, device="cuda:0", seed=2, use_graph=True,
                      verbose=True):
  ck = dict(config.get("pre_ckpt_paths", {}))
  with_encoder = needs_encoder(config)
  kind = config["ldm_sampling"]["autoencoder_type"]
  if kind not in ("kl", "vq"):
    raise NotImplementedError("invalid autoencoder type.")
  latent_size = decode_latent_size(config)
  hidden = config["cond_stage_model"]["hidden_size"]
  if ck.get("compvis"):
    # one CompVis PyTorch checkpoint for all three models (checkpoint.py; what the
    # reference reaches through convert_ckpt_pytorch_to_tf2.py + three TF checkpoints).  txt2img
    # decodes only: the checkpoint's encoder is loaded for img2img alone; the U-Net's context width
    # is the text model's hidden size; a VQ decoder's attention blocks depend on the latent size it
    # will run at.
    from .checkpoint import from_compvis_state_dict
    sd = torch.load(ck["compvis"], map_location="cpu", weights_only=True)
    sd = {k: v.float().numpy() for k, v in sd.get("state_dict", sd).items() if torch.is_tensor(v)}
    loaded = from_compvis_state_dict(sd, **compvis_manifest_configs(config), with_encoder=with_encoder,
                                     kl=(kind == "kl"))
    _preloaded.update(loaded)
  transformer = TransformerModel(**config["cond_stage_model"], dtype=dtype, device=device, seed=seed,
                                 weights=_load_weights(ck.get("cond_stage_model"), "cond_stage_model"))
  unet = UNet(**config["unet"], dtype=dtype, device=device, seed=seed,
              context_dim=hidden,
              weights=_load_weights(ck.get("unet"), "unet"))
  if kind == "kl":
    autoencoder = AutoencoderKL(**config["autoencoder_kl"], dtype=dtype, device=device, seed=seed,
                                weights=_load_weights(ck.get("autoencoder"), "autoencoder"),
                                with_encoder=with_encoder or None)
  elif kind == "vq":
    autoencoder = AutoencoderVQ(**config["autoencoder_vq"], dtype=dtype, device=device, seed=seed,
                                latent_size=latent_size,
                                weights=_load_weights(ck.get("autoencoder"), "autoencoder"),
                                with_encoder=with_encoder or None)
  return LatentDiffusionModelSampler(unet=unet, autoencoder=autoencoder, cond_stage_model=transformer,
                                     use_graph=use_graph, verbose=verbose, sampler=sampler_name(config),
                                     noise_source=noise_source_name(config),
                                     step_spacing=step_spacing_name(config),
                                     **config["ldm"])


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--config_path", required=True)
  ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
  ap.add_argument("--seed", type=int, default=0,
                  help="seed of every draw: x_T, the noise when eta > 0, img2img's encode and q_sample noise")
  ap.add_argument("--out", default="images.npy")
  args = ap.parse_args(argv)
  with open(args.config_path) as f:
    config = yaml.safe_load(f)
  dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
  sampler = build_from_config(config, dtype=dtype)
  samp = config["ldm_sampling"]
  token_ids = get_token_ids(samp["text_prompt"], samp["latent_shape"][0], samp["vocab_dir"],
                            config["cond_stage_model"]["max_seq_len"])
  source_ids = None
  if samp.get("source_prompt") is not None:
    source_ids = get_token_ids(samp["source_prompt"], samp["latent_shape"][0], samp["vocab_dir"],
                               config["cond_stage_model"]["max_seq_len"])
  method, args_, kwargs = sampling_call(config, token_ids, args.seed, source_ids=source_ids)
  if method == "ddim_p_sample_loop_progressive":
    # run_ldm_sampler.py:89-94 (with the reference's unpacking bug fixed: three results)
    _, sample_prog, pred_x0_prog = sampler.ddim_p_sample_loop_progressive(*args_, **kwargs)
    for name, t in (("sample_prog.npy", sample_prog), ("pred_x0_prog.npy", pred_x0_prog)):
      print(f"[INFO] Save progressive images to '{name}'...")
      b, r = t.shape[0], t.shape[1]
      # tensor_to_image normalises inputs[i] over everything but the batch axis (:19-22)
      u8 = tensor_to_image(t.reshape(b, r * t.shape[2], t.shape[3], t.shape[4]))
      np.save(name, u8.reshape(tuple(t.shape)))
    return
  setup_preview(sampler, config, args.seed)
  images = getattr(sampler, method)(*args_, **kwargs)
  print(f"[INFO] Save generated images to '{args.out}'...")
  np.save(args.out, tensor_to_image(images))
  if "preview_freq" in kwargs:
    strips = sampler.last_previews()
    for name, key in (("preview_sample.npy", "sample"), ("preview_x0.npy", "pred_x0")):
      path = os.path.join(os.path.dirname(os.path.abspath(args.out)), name)
      print(f"[INFO] Save latent previews to '{path}'...")
      np.save(path, strips[key])
  am = attention_map_settings(config)
  if am is not None:
    import json
    from .tokenizer import BertWordPieceTokenizer
    maps = sampler.last_attention_maps(size=am["size"])
    spans = BertWordPieceTokenizer(samp["vocab_dir"]).word_spans(samp["text_prompt"],
                                                                 config["cond_stage_model"]["max_seq_len"])
    out_dir = os.path.dirname(os.path.abspath(args.out))
    print(f"[INFO] Save cross-attention maps to '{os.path.join(out_dir, 'attention_maps.npy')}'...")
    np.save(os.path.join(out_dir, "attention_maps.npy"), maps["heat"])
    with open(os.path.join(out_dir, "attention_words.json"), "w") as f:
      json.dump([dict(word=w, positions=pos) for w, pos in spans], f)


if __name__ == "__main__":
  main()
