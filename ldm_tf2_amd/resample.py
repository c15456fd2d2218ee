"""The antialiased resampling rule -- host side.

One rule per axis, the one of PIL's Image.resize and of torch.nn.functional.interpolate(antialias=True): the filter is
stretched by the shrink factor, so an output sample averages everything its footprint covers.  With source extent L,
output extent Lo, output index i and a filter of half-width r, all in float64:

    scale = L / Lo            fs = max(scale, 1)       support = r * fs
    center = scale * (i + 0.5)
    xmin = max(0, int(center - support + 0.5))
    xmax = min(L, int(center + support + 0.5))
    w_j = filter((j - center + 0.5) / fs)   for j in [xmin, xmax),   normalised to sum 1

`resample_taps` lays an axis out as the table ldm_resample_nhwc reads (include/ldm_hip.h): every output index reads the
same number T of consecutive source indices, rows near the far edge are shifted back inside [0, L) and zero-filled.
The tables are built here, like the DEIS weight table, and cached per (L, Lo, filter, device).
"""
from __future__ import annotations

import numpy as np

from ._lib import RESAMPLE_FILTERS


def _triangle(x):
  return np.maximum(0., 1. - np.abs(x))


def _cubic(x):
  """Keys' cubic convolution kernel with a = -0.5 (PIL's BICUBIC, torch's antialiased bicubic; ldm_resize_nhwc uses
  -0.75, as torch's non-antialiased one does)."""
  a = -0.5
  x = np.abs(x)
  near = ((a + 2.) * x - (a + 3.)) * x * x + 1.
  far = (((x - 5.) * x + 8.) * x - 4.) * a
  return np.where(x < 1., near, np.where(x < 2., far, 0.))


def _lanczos3(x):
  return np.where(np.abs(x) < 3., np.sinc(x) * np.sinc(x / 3.), 0.)


FILTERS = {"triangle": (1., _triangle), "cubic": (2., _cubic), "lanczos3": (3., _lanczos3)}
assert tuple(FILTERS) == RESAMPLE_FILTERS


def check_filter(name, what="filter"):
  if name not in FILTERS:
    raise ValueError(f"{what} must be one of {RESAMPLE_FILTERS}, got {name!r}")
  return name


def axis_weights(L, Lo, filter):
  """The rule as written: per output index i the pair (xmin_i, float64 weights of the source indices xmin_i ..
  xmax_i - 1, normalised to sum 1).  Lo == L: the identity, (i, [1.]) for every filter (np.sinc(1.0) is 3.9e-17, not
  0, and a same-size resample must stay a copy)."""
  L, Lo = int(L), int(Lo)
  if L < 1 or Lo < 1:
    raise ValueError(f"resample extents must be positive, got {L} -> {Lo}")
  r, fn = FILTERS[check_filter(filter)]
  if Lo == L:
    return [(i, np.ones(1, dtype=np.float64)) for i in range(L)]
  scale = L / Lo
  fs = max(scale, 1.)
  support = r * fs
  rows = []
  for i in range(Lo):
    center = scale * (i + 0.5)
    xmin = max(0, int(center - support + 0.5))
    xmax = min(L, int(center + support + 0.5))
    w = fn((np.arange(xmin, xmax, dtype=np.float64) - center + 0.5) / fs)
    rows.append((xmin, w / w.sum()))
  return rows


def resample_taps(L, Lo, filter):
  """(start int32 [Lo], weights float32 [Lo, T], T): T = the largest xmax - xmin over i; row i covers the source
  indices start_i .. start_i + T - 1 with start_i = min(xmin_i, L - T), its weights shifted accordingly and
  zero-filled, so no row reaches outside [0, L) (T <= L always).  Normalised in float64, rounded once to float32."""
  rows = axis_weights(L, Lo, filter)
  T = max(len(w) for _, w in rows)
  start = np.empty(len(rows), dtype=np.int32)
  weights = np.zeros((len(rows), T), dtype=np.float64)
  for i, (xmin, w) in enumerate(rows):
    start[i] = min(xmin, int(L) - T)
    off = xmin - int(start[i])
    weights[i, off:off + len(w)] = w
  assert T <= int(L) and start.min() >= 0
  return start, weights.astype(np.float32), T


_DEVICE_TABLES = {}


def device_taps(L, Lo, filter, device):
  """resample_taps on `device`, (start, weights, T), built once per (L, Lo, filter, device)."""
  import torch
  device = torch.device(device)
  key = (int(L), int(Lo), filter, device)
  tab = _DEVICE_TABLES.get(key)
  if tab is None:
    start, weights, T = resample_taps(L, Lo, filter)
    tab = (torch.from_numpy(start).to(device), torch.from_numpy(weights).to(device).contiguous(), T)
    _DEVICE_TABLES[key] = tab
  return tab


def crop_box(src, dst):
  """The centred box of the source (Hs, Ws) with the aspect ratio of the target (H, W), in integer arithmetic:
  (y0, x0, hc, wc).  A source wider than the target loses columns, a taller one rows; at least one pixel stays."""
  (Hs, Ws), (H, W) = (int(v) for v in src), (int(v) for v in dst)
  if min(Hs, Ws, H, W) < 1:
    raise ValueError(f"crop_box: extents must be positive, got {(Hs, Ws)} -> {(H, W)}")
  if Ws * H > Hs * W:
    wc = min(max((Hs * W + H // 2) // H, 1), Ws)
    return 0, (Ws - wc) // 2, Hs, wc
  hc = min(max((Ws * H + W // 2) // W, 1), Hs)
  return (Hs - hc) // 2, 0, hc, Ws
