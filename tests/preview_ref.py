"""Restatement of the latent previews, NumPy, no GPU.

A preview of latents lat [B,h,w,c] through proj [c+1,3] (c weight rows, then the bias row), an integer upscale s and
an 8-bit quantisation:
  p[b,y,x,k] = bias[k] + sum_j lat[b,y,x,j] proj[j][k]
  v = p enlarged s times: "nearest" or "bilinear" by the rules of tests/hires_ref.py at Lo = s L
  t = 127.5 v + 127.5;  byte = floor(min(max(t, 0), 255) + 0.5), a NaN giving 0.
`preview64` is that in float64 from the rules as written (project, then upscale).  `preview32` is a float32 emulation in
the order the device kernel documents (include/ldm_hip.h: upscale each channel, then project; both are the same affine
map): its error against `preview64` is what float32 costs, the tests' gate.

The slot rule of a strip of R frames recorded every `freq` DDIM indices: idx < 0, idx % freq != 0 or idx // freq >= R
write nothing; any other idx writes slot idx // freq."""
import numpy as np

from hires_ref import _axis_taps32, resize64

MODES = ("nearest", "bilinear")


def preview64(lat, proj, scale, mode):
  """float64 t [B,s*h,s*w,3]: project -> upscale -> 127.5 v + 127.5."""
  lat = np.asarray(lat, dtype=np.float64)
  proj = np.asarray(proj, dtype=np.float64)
  c = lat.shape[-1]
  assert proj.shape == (c + 1, 3) and mode in MODES
  with np.errstate(invalid="ignore"):
    p = lat @ proj[:c] + proj[c]
    v = resize64(p, (scale * lat.shape[1], scale * lat.shape[2]), mode)
    return 127.5 * v + 127.5


def quantise(t):
  """uint8 floor(min(max(t, 0), 255) + 0.5); a NaN gives 0 (the max drops it)."""
  t = np.asarray(t, dtype=np.float64)
  t = np.where(np.isnan(t), 0., t)
  return np.floor(np.clip(t, 0., 255.) + 0.5).astype(np.uint8)


def preview32(lat, proj, scale, mode):
  """The float32 emulation, every product and sum rounded to float32: per channel j the upscaled latent (nearest: a
  copy; bilinear: the sum over the 2 x 2 taps of (wy wx) x from 0, rows outermost), v_k accumulated over ascending j
  from the bias, t = 127.5 v + 127.5.  Returns float32 t [B,s*h,s*w,3]."""
  f32 = np.float32
  lat = np.asarray(lat, dtype=f32)
  proj = np.asarray(proj, dtype=f32)
  B, h, w, c = lat.shape
  sh, sw = scale * h, scale * w
  if mode == "nearest" or scale == 1:
    up = lat[:, np.arange(sh) // scale][:, :, np.arange(sw) // scale]
  else:
    (iy, wy), (ix, wx) = _axis_taps32(h, sh, mode), _axis_taps32(w, sw, mode)
    up = np.zeros((B, sh, sw, c), dtype=f32)
    for a in range(2):
      for b in range(2):
        wt = (wy[:, a, None] * wx[None, :, b]).astype(f32)
        up = (up + (wt[None, :, :, None] * lat[:, iy[:, a]][:, :, ix[:, b]]).astype(f32)).astype(f32)
  v = np.broadcast_to(proj[c], (B, sh, sw, 3)).astype(f32)
  for j in range(c):
    v = (v + (up[..., j, None] * proj[j]).astype(f32)).astype(f32)
  return ((f32(127.5) * v).astype(f32) + f32(127.5)).astype(f32)


def slot_of(idx, freq, R):
  """The slot a launch at DDIM index `idx` writes, None when it writes nothing."""
  if idx < 0 or idx % freq != 0 or idx // freq >= R:
    return None
  return idx // freq
