"""The paste-back's arithmetic restated in NumPy: ldm_mask_feather, ldm_keep_stats and
ldm_paste_back in the kernels' order of operations, in float64 or float32.

An fma is one rounding of g v + acc.  In float64 the restatement writes acc + g * v (two roundings, 1e-16 apart from one:
far below anything a float32 result is compared at).  In float32 the product of two float32 values is exact in float64,
so the sum is formed there and rounded to float32: an fma but for the rare double rounding.  In the row blur v is 0 or 1
and the product is exact in either type.
"""
import numpy as np

from ldm_tf2_amd.feather import feather_radius, feather_taps  # noqa: F401  (the taps are the host's, float32)


def kept(m):
  """P: 1 where m >= 1, a NaN counting as a hole."""
  with np.errstate(invalid="ignore"):
    return np.asarray(m) >= 1


def erode(P, r):
  """e = 1 iff every in-bounds pixel within Chebyshev distance r is kept: rows, then columns; [..., H, W] bool."""
  H, W = P.shape[-2:]
  rows = np.empty_like(P)
  for x in range(W):
    rows[..., x] = P[..., max(0, x - r):x + r + 1].all(axis=-1)
  e = np.empty_like(P)
  for y in range(H):
    e[..., y, :] = rows[..., max(0, y - r):y + r + 1, :].all(axis=-2)
  return e


def _fma(g, v, acc, dtype):
  if dtype == np.float64:
    return acc + np.asarray(g, dtype=np.float64) * v
  return (acc.astype(np.float64) + np.asarray(g, dtype=np.float64) * v.astype(np.float64)).astype(np.float32)


def _blur_last(q, taps, dtype):
  """sum_t taps[t] q[..., x + t - r], taps outside contributing nothing, ascending t from 0."""
  r = (len(taps) - 1) // 2
  W = q.shape[-1]
  acc = np.zeros(q.shape, dtype=dtype)
  for t, g in enumerate(taps):
    lo, hi = max(0, r - t), min(W, W + r - t)          # the outputs x whose tap x + t - r lies inside
    if lo < hi:
      acc[..., lo:hi] = _fma(g, q[..., lo + t - r:hi + t - r], acc[..., lo:hi], dtype)
  return acc


def feather_ref(m, sigma, dtype=np.float64, taps=None):
  """w = P ? clamp(1 - blur(1 - erode(P)), 0, 1) : 0; m [..., H, W]."""
  taps = feather_taps(sigma) if taps is None else taps
  r = (len(taps) - 1) // 2
  P = kept(m)
  q = (~erode(P, r)).astype(dtype)
  hq = _blur_last(q, taps, dtype)
  v = np.swapaxes(_blur_last(np.swapaxes(hq, -1, -2), taps, dtype), -1, -2)
  w = np.clip(dtype(1) - v, dtype(0), dtype(1)).astype(dtype)
  return np.where(P, w, dtype(0))


def keep_stats_ref(o, d, m):
  """stats [B,c,5] float64 = n, sum o, sum o^2, sum d, sum d^2 over the kept pixels (selected, so a NaN in a hole does
  not leak); m [B,H,W] or [1,H,W]."""
  B, H, W, c = o.shape
  P = np.broadcast_to(kept(m), (B, H, W))
  stats = np.zeros((B, c, 5), dtype=np.float64)
  for b in range(B):
    ob, db = o[b][P[b]].astype(np.float64), d[b][P[b]].astype(np.float64)       # [n, c]
    stats[b, :, 0] = ob.shape[0]
    stats[b, :, 1], stats[b, :, 2] = ob.sum(axis=0), (ob * ob).sum(axis=0)
    stats[b, :, 3], stats[b, :, 4] = db.sum(axis=0), (db * db).sum(axis=0)
  return stats


def gain_offset_ref(stats):
  """(a, b) [B,c] float64 from the statistics, by the finalise launch's formulas."""
  a = np.ones(stats.shape[:2], dtype=np.float64)
  b = np.zeros(stats.shape[:2], dtype=np.float64)
  for i in np.ndindex(*stats.shape[:2]):
    n, so, so2, sd, sd2 = stats[i]
    if n < 1:
      continue
    vo, vd = (so2 - so * so / n) / n, (sd2 - sd * sd / n) / n
    if n >= 2 and vd > 1e-12:
      a[i] = min(max(np.sqrt(max(vo, 0.) / vd), 0.5), 2.)
    b[i] = so / n - a[i] * (sd / n)
  return a, b


def paste_ref(o, d, w, gain=None, offset=None, dtype=np.float64):
  """out = w >= 1 ? o : (w <= 0 ? d' : fma(w, o - d', d')), d' = fma(a, d, b) or d; w [B,H,W] or [1,H,W]."""
  o, d = np.asarray(o).astype(dtype), np.asarray(d).astype(dtype)
  w = np.broadcast_to(np.asarray(w).astype(dtype), o.shape[:3])[..., None]
  if gain is not None:
    a = np.asarray(gain).astype(dtype)[:, None, None, :]
    b = np.asarray(offset).astype(dtype)[:, None, None, :]
    d = _fma(a, d, np.broadcast_to(b, d.shape), dtype) if dtype == np.float32 else a * d + b
  with np.errstate(invalid="ignore"):
    mid = d + w * (o - d) if dtype == np.float64 else _fma(w, (o - d).astype(np.float32), d, dtype)
    return np.where(w >= 1, o, np.where(w <= 0, d, mid)).astype(dtype)
