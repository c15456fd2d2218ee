"""Push-pull hole filling restated in NumPy (include/ldm_hip.h): the reference of
ldm_pushpull_fill, in the kernel's order of operations, in float64 or float32.

  Level 0: a_0 = x, w_0 = clamp(m, 0, 1), a NaN in m counting as 0.
  Pull l -> l+1 until 1 x 1: H_{l+1} = ceil(H_l / 2), W_{l+1} = ceil(W_l / 2); the in-bounds children (2i+dy, 2j+dx)
    in the order (0,0), (0,1), (1,0), (1,1): s += w, v = fma(w, a, v), a child of weight 0 contributing nothing
    whatever its value (a select); a_{l+1} = s > 0 ? v / s : 0; w_{l+1} = min(s, 1).
  Push from f_L = a_L (a 1 x 1 image: x where w_0 > 0, else 0): cy = y >> 1, ny = clamp(cy + (y & 1 ? 1 : -1)),
    columns alike; top = fma(.25, f[cy,nx], .75 f[cy,cx]), bot = fma(.25, f[ny,nx], .75 f[ny,cx]),
    u = fma(.25, bot, .75 top); f_l = a_l where w_l == 1, u where w_l == 0, fma(w_l, a_l - u, u) otherwise.

NumPy has no fused multiply-add.  In float32 the product of two float32 values is exact in float64, so
fma(a, b, c) is float32(float64(a) * float64(b) + float64(c)): one rounding to float64 before the one to float32, which
differs from the fused result only where the float64 sum lands within 2^-29 ulp of a float32 tie.  In float64 the
multiply and the add round separately (an error of 1e-16, nothing beside float32's 6e-8).
"""
import numpy as np


def pyramid_extents(H, W):
  """[(H_0, W_0), ..., (H_L, W_L)] with (H_L, W_L) = (1, 1)."""
  out = [(int(H), int(W))]
  while out[-1] != (1, 1):
    h, w = out[-1]
    out.append(((h + 1) // 2, (w + 1) // 2))
  return out


def _fma(a, b, c, dtype):
  if dtype == np.float32:
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
  return a * b + c


def keep_weight(m, dtype):
  m = np.asarray(m, dtype=dtype)
  with np.errstate(invalid="ignore"):
    return np.where(m > 0, np.where(m < 1, m, dtype(1)), dtype(0)).astype(dtype)


def _pull(a, w, dtype):
  B, H, W, c = a.shape
  Hc, Wc = (H + 1) // 2, (W + 1) // 2
  s = np.zeros((B, Hc, Wc), dtype)
  v = np.zeros((B, Hc, Wc, c), dtype)
  for dy in (0, 1):
    for dx in (0, 1):
      ac, wc = a[:, dy::2, dx::2], w[:, dy::2, dx::2]        # (the children that exist: the in-bounds ones)
      h, ww = ac.shape[1:3]
      on = wc > 0
      sel = np.where(on[..., None], ac, dtype(0))            # the select: a hole's value is never multiplied
      s[:, :h, :ww] = s[:, :h, :ww] + wc
      v[:, :h, :ww] = _fma(np.broadcast_to(wc[..., None], sel.shape).astype(dtype), sel, v[:, :h, :ww], dtype)
  pos = s > 0
  with np.errstate(invalid="ignore", divide="ignore"):
    an = np.where(pos[..., None], v / np.where(pos, s, dtype(1))[..., None], dtype(0)).astype(dtype)
  return an, np.minimum(s, dtype(1)).astype(dtype)


def _push(fc, a, w, dtype):
  B, H, W, c = a.shape
  Hc, Wc = fc.shape[1:3]
  y, x = np.arange(H), np.arange(W)
  cy, cx = y >> 1, x >> 1
  ny = np.clip(cy + np.where(y & 1, 1, -1), 0, Hc - 1)
  nx = np.clip(cx + np.where(x & 1, 1, -1), 0, Wc - 1)
  q, t = dtype(0.25), dtype(0.75)
  f00, f01 = fc[:, cy][:, :, cx], fc[:, cy][:, :, nx]
  f10, f11 = fc[:, ny][:, :, cx], fc[:, ny][:, :, nx]
  top = _fma(f01, q, t * f00, dtype)
  bot = _fma(f11, q, t * f10, dtype)
  u = _fma(bot, q, t * top, dtype)
  wb = np.broadcast_to(w[..., None], a.shape)
  hole = wb == 0
  a_safe = np.where(hole, dtype(0), a)                       # (a hole's value is selected away, never used)
  with np.errstate(invalid="ignore"):
    mid = _fma(wb.astype(dtype), (a_safe - u).astype(dtype), u, dtype)
  return np.where(wb == 1, a, np.where(hole, u, mid)).astype(dtype)


def pushpull_ref(x, m, dtype=np.float64):
  """x [B,H,W,c], m [B,H,W] -> [B,H,W,c] in `dtype` (np.float64 or np.float32), the kernel's order of operations."""
  dtype = np.dtype(dtype).type
  a = [np.asarray(x, dtype=dtype)]
  w = [keep_weight(m, dtype)]
  if a[0].ndim != 4 or w[0].shape != a[0].shape[:3]:
    raise ValueError(f"x {a[0].shape} must be [B,H,W,c] and m {w[0].shape} [B,H,W]")
  while a[-1].shape[1:3] != (1, 1):
    an, wn = _pull(a[-1], w[-1], dtype)
    a.append(an)
    w.append(wn)
  if len(a) == 1:
    return np.where(w[0][..., None] > 0, a[0], dtype(0)).astype(dtype)
  f = a[-1]
  for l in range(len(a) - 2, -1, -1):
    f = _push(f, a[l], w[l], dtype)
  return f
