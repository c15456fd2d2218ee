"""Panorama sampling restated in NumPy.  Nothing here comes from the product; the tests compare
the product's window grid, kernels and loop with these.

Grid.  An axis of extent L, window l, stride s (1 <= l <= L, 1 <= s <= l): n = ceil((L - l) / s) + 1 windows at
origin_i = min(i * s, L - l).  A canvas [B,H,W,c] with window (h, w) and stride (sy, sx) has nW = nY * nX windows,
window k = ky * nX + kx at (oy[ky], ox[kx]).
gather: [B,H,W,c] -> [2,B,nW,h,w,c], both halves the crops.
fold:   [halves,B,nW,h,w,c] -> [halves,B,H,W,c]; every canvas element = (sum over the covering windows, float32, in
        ascending k, starting from the first covering value) / float32(count), one float32 division.
Loop.   Per DDIM index: crop the canvas, the oracle's U-Net on the rows [uncond ; cond] x B x nW, fold, CFG and the
        solver's update on the canvas (O.ddim_update, plms_ref's constants or deis_ref's table through
        deis_ref.ms_update).
"""
import math

import numpy as np


def origins(L, l, s):
  if not (1 <= l <= L and 1 <= s <= l):
    raise ValueError((L, l, s))
  n = math.ceil((L - l) / s) + 1
  return [min(i * s, L - l) for i in range(n)]


def windows(H, W, window, stride):
  """[(oy, ox)] in window order k = ky * nX + kx."""
  return [(oy, ox) for oy in origins(H, window[0], stride[0]) for ox in origins(W, window[1], stride[1])]


def counts(H, W, window, stride):
  """int [H,W]: how many windows cover each canvas cell."""
  n = np.zeros((H, W), dtype=np.int64)
  for oy, ox in windows(H, W, window, stride):
    n[oy:oy + window[0], ox:ox + window[1]] += 1
  return n


def gather(canvas, window, stride):
  canvas = np.asarray(canvas)
  B, H, W, c = canvas.shape
  h, w = window
  crops = np.stack([canvas[:, oy:oy + h, ox:ox + w] for oy, ox in windows(H, W, window, stride)], axis=1)
  return np.stack([crops, crops])


def _fold(eps_win, H, W, window, stride, dtype):
  eps_win = np.asarray(eps_win)
  halves, B, n_win, h, w, c = eps_win.shape
  wins = windows(H, W, window, stride)
  assert n_win == len(wins) and (h, w) == tuple(window)
  acc = np.zeros((halves, B, H, W, c), dtype=dtype)
  seen = np.zeros((H, W), dtype=bool)
  for k, (oy, ox) in enumerate(wins):
    v = eps_win[:, :, k].astype(dtype)
    first = ~seen[oy:oy + h, ox:ox + w][None, None, :, :, None]
    region = acc[:, :, oy:oy + h, ox:ox + w]
    # (the first covering value starts the sum: 0 + v would turn -0 into +0)
    acc[:, :, oy:oy + h, ox:ox + w] = np.where(first, v, region + v)
    seen[oy:oy + h, ox:ox + w] = True
  assert seen.all()
  return acc / counts(H, W, window, stride).astype(dtype)[None, None, :, :, None]


def fold(eps_win, H, W, window, stride):
  """float32, the summation order and the single division of the specification."""
  out = _fold(np.asarray(eps_win, dtype=np.float32), H, W, window, stride, np.float32)
  assert out.dtype == np.float32
  return out


def fold64(eps_win, H, W, window, stride):
  return _fold(eps_win, H, W, window, stride, np.float64)


def fold_abs(eps_win, H, W, window, stride):
  """float64 sum_k |v_k| / count per canvas element: the scale of fold's rounding-error bound."""
  return _fold(np.abs(np.asarray(eps_win, dtype=np.float64)), H, W, window, stride, np.float64)


def loop(O, context, w_unet, x_T, window, stride, sched, gs, sampler="ddim", noises=None, weights=None, ms_update=None,
         plms_weights=None):
  """The canvas loop over DDIM indices N-1 .. 0 in float32 torch.  O = oracle.ldm_oracle; context [2B,T,D];
  sched = O.make_schedule's dictionary (any step table); sampler "ddim" (noises [N,B,H,W,c] or None), "plms"
  (`plms_weights` = plms_ref.WEIGHTS) or "deis" (`weights` float32 [N,4,4]); `ms_update` = deis_ref.ms_update.
  Returns the final canvas."""
  import torch
  x = torch.as_tensor(np.asarray(x_T), dtype=torch.float32)
  B, H, W, c = x.shape
  n_win = len(windows(H, W, window, stride))
  context = torch.as_tensor(context)
  ctx = torch.cat([context[:B].repeat_interleave(n_win, 0), context[B:].repeat_interleave(n_win, 0)])
  f = lambda key: np.asarray(sched[key]).astype(np.float32)
  c1, c2, a_prev = f("ddim_sqrt_recip_alphas_cumprod"), f("ddim_sqrt_recipm1_alphas_cumprod"), f("ddim_alphas_cumprod_prev")
  steps = sched["ddim_steps"]
  n = len(steps)
  hist = []
  for i in range(n - 1, -1, -1):
    rows = torch.from_numpy(gather(x.numpy(), window, stride).reshape(2 * B * n_win, window[0], window[1], c))
    t = np.full([2 * B * n_win], steps[i], dtype=np.int32)
    eps_win = O.unet_forward(rows, t, ctx, w_unet, torch.float32)
    eps = torch.from_numpy(fold(eps_win.numpy().reshape(2, B, n_win, window[0], window[1], c), H, W, window, stride))
    eu, ec = eps[0], eps[1]
    if sampler == "ddim":
      nz = torch.zeros_like(x) if noises is None else torch.as_tensor(noises[i])
      x, _ = O.ddim_update(x, eu, ec, sched, i, gs, nz)
    else:
      hist.insert(0, eu + np.float32(gs) * (ec - eu))
      del hist[4:]
      j = min(n - 1 - i, 3)
      wrow = np.array(plms_weights[j], dtype=np.float32) if sampler == "plms" else weights[i, j]
      x, _ = ms_update(x, hist, i, j, wrow, c1, c2, a_prev)
    assert x.dtype == torch.float32
  return x
