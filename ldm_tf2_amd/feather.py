"""The feather's tap table -- host side.

ldm_mask_feather blurs the complement of the eroded keep mask with a Gaussian of `sigma` pixels cut at r = ceil(3 sigma):
g[i] = exp(-(i - r)^2 / (2 sigma^2)) for i = 0 .. 2r, normalised to sum 1 in float64 and rounded once to float32;
sigma = 0 gives the single tap 1.  The table is built here, like the resample tables (resample.py), and cached per
(sigma, device).
"""
from __future__ import annotations

import math

import numpy as np

MAX_SIGMA = 16.                  # r = ceil(3 sigma) <= 48, the launcher's bound


def feather_radius(sigma):
  """r = ceil(3 sigma) for a finite sigma in [0, MAX_SIGMA]; ValueError otherwise."""
  number = isinstance(sigma, (int, float, np.integer, np.floating)) and not isinstance(sigma, (bool, np.bool_))
  if not number or not 0. <= float(sigma) <= MAX_SIGMA:            # (a NaN fails both comparisons)
    raise ValueError(f"mask_feather must be a number of pixels in [0, {MAX_SIGMA:g}], got {sigma!r}")
  return int(math.ceil(3. * float(sigma)))


def feather_taps(sigma):
  """float32 [2r + 1]: the normalised Gaussian taps of `sigma`, symmetric about index r."""
  r = feather_radius(sigma)
  if r == 0:
    return np.ones(1, dtype=np.float32)
  i = np.arange(2 * r + 1, dtype=np.float64) - r
  g = np.exp(-(i * i) / (2. * float(sigma) ** 2))
  return (g / g.sum()).astype(np.float32)


_DEVICE_TAPS = {}


def device_taps(sigma, device):
  """(feather_taps on `device`, r), built once per (sigma, device)."""
  import torch
  device = torch.device(device)
  key = (float(sigma), device)
  tab = _DEVICE_TAPS.get(key)
  if tab is None:
    taps = feather_taps(sigma)
    tab = (torch.from_numpy(taps).to(device), (len(taps) - 1) // 2)
    _DEVICE_TAPS[key] = tab
  return tab
