"""Seamless panoramas restated in NumPy.  Nothing here comes from the product; the tests compare
the product's wrapped grid, kernels, profiles and loop with these.  The unwrapped grid is tests/panorama_ref.py's.

Grid.   A wrapped axis of extent L, window l, stride s (1 <= l <= L, 1 <= s <= l): n = ceil(L / s) windows at origin_i
        = i * s, window i covering the cells (origin_i + j) mod L, j = 0 .. l - 1.  An unwrapped axis is
        panorama_ref.origins.  Window k = ky * nX + kx.
gather: [B,H,W,c] -> [2,B,nW,h,w,c], both halves the (circular) crops.
fold:   [halves,B,nW,h,w,c] -> [halves,B,H,W,c] with the profile tables wy [h], wx [w] (None: uniform).  Per canvas
        element over the covering windows in ascending k, starting from the first covering term:
        ww = wy[jy] * wx[jx], num += ww * v, den += ww, out = num / den, every operation in `dtype`, rounded once.
        Uniform: num += v, den = count.
pad:    np.pad(mode="wrap") along H and W.
Loop.   panorama_ref.loop with these gather and fold.
"""
import math

import numpy as np

import panorama_ref as P


def origins(L, l, s, wrap):
  if not wrap:
    return P.origins(L, l, s)
  if not (1 <= l <= L and 1 <= s <= l):
    raise ValueError((L, l, s))
  return [i * s for i in range(math.ceil(L / s))]


def windows(H, W, window, stride, wrap):
  """[(oy, ox)] in window order k = ky * nX + kx."""
  return [(oy, ox) for oy in origins(H, window[0], stride[0], wrap[0])
          for ox in origins(W, window[1], stride[1], wrap[1])]


def cells(o, l, L):
  """The cells window elements 0 .. l - 1 lie on, for a window at origin o (o + l <= L on an unwrapped axis)."""
  return (o + np.arange(l)) % L


def counts(H, W, window, stride, wrap):
  n = np.zeros((H, W), dtype=np.int64)
  for oy, ox in windows(H, W, window, stride, wrap):
    n[np.ix_(cells(oy, window[0], H), cells(ox, window[1], W))] += 1
  return n


def covering_ranges(L, l, s, p):
  """The two index ranges of the windows covering cell p of a wrapped axis, as lists: the i < n with
  i s <= p < i s + l, and the i < n with i s <= p + L < i s + l."""
  n = math.ceil(L / s)
  first = [i for i in range(n) if i * s <= p < i * s + l]
  second = [i for i in range(n) if i * s <= p + L < i * s + l]
  return first, second


def gather(canvas, window, stride, wrap):
  canvas = np.asarray(canvas)
  B, H, W, c = canvas.shape
  h, w = window
  crops = np.stack([canvas[:, cells(oy, h, H)][:, :, cells(ox, w, W)]
                    for oy, ox in windows(H, W, window, stride, wrap)], axis=1)
  return np.stack([crops, crops])


def tent(l):
  return np.array([min(j + 1, l - j) for j in range(l)], dtype=np.float32)


def gaussian(l):
  j = np.arange(l, dtype=np.float64)
  return np.exp(-(j - (l - 1) / 2) ** 2 / (2 * (l / 4) ** 2)).astype(np.float32)


def _fold(eps_win, H, W, window, stride, wrap, wy, wx, dtype, absolute=False):
  """-> (out, num, den, count); the tables are float32 values whatever `dtype` is."""
  eps_win = np.asarray(eps_win)
  halves, B, n_win, h, w, c = eps_win.shape
  wins = windows(H, W, window, stride, wrap)
  assert n_win == len(wins) and (h, w) == tuple(window) and (wy is None) == (wx is None)
  num = np.zeros((halves, B, H, W, c), dtype=dtype)
  den = np.zeros((H, W), dtype=dtype)
  seen = np.zeros((H, W), dtype=bool)
  count = np.zeros((H, W), dtype=np.int64)
  ww = None
  if wy is not None:
    wy, wx = np.asarray(wy, dtype=np.float32), np.asarray(wx, dtype=np.float32)
    assert wy.shape == (h,) and wx.shape == (w,)
    ww = wy.astype(dtype)[:, None] * wx.astype(dtype)[None, :]        # one rounding in `dtype`
    assert ww.dtype == dtype
  for k, (oy, ox) in enumerate(wins):
    ix = np.ix_(cells(oy, h, H), cells(ox, w, W))
    sel = (slice(None), slice(None)) + ix
    v = eps_win[:, :, k].astype(dtype)
    if absolute:
      v = np.abs(v)
    first = ~seen[ix]
    if ww is not None:
      v = ww[None, None, :, :, None] * v
      den[ix] = np.where(first, ww, den[ix] + ww)
    assert v.dtype == dtype
    # (the first covering term starts the sum: 0 + v would turn -0 into +0)
    num[sel] = np.where(first[None, None, :, :, None], v, num[sel] + v)
    seen[ix] = True
    count[ix] += 1
  assert seen.all()
  if ww is None:
    den = count.astype(dtype)
  out = num / den[None, None, :, :, None]
  assert out.dtype == dtype
  return out, num, den, count


def fold(eps_win, H, W, window, stride, wrap, wy=None, wx=None):
  """float32, the order and the roundings of the specification."""
  return _fold(np.asarray(eps_win, dtype=np.float32), H, W, window, stride, wrap, wy, wx, np.float32)[0]


def fold64(eps_win, H, W, window, stride, wrap, wy=None, wx=None):
  """float64 from the same float32 tables."""
  return _fold(eps_win, H, W, window, stride, wrap, wy, wx, np.float64)[0]


def fold_abs(eps_win, H, W, window, stride, wrap, wy=None, wx=None):
  """float64 sum_k |w_k v_k| / sum_k w_k per canvas element: the scale of fold's rounding-error bound."""
  return _fold(eps_win, H, W, window, stride, wrap, wy, wx, np.float64, absolute=True)[0]


def fold_den(H, W, window, stride, wrap, wy=None, wx=None):
  """float32 [H,W]: the denominator of every cell, summed as fold sums it."""
  z = np.zeros((1, 1, len(windows(H, W, window, stride, wrap)), window[0], window[1], 1), dtype=np.float32)
  return _fold(z, H, W, window, stride, wrap, wy, wx, np.float32)[2]


def wrap_pad(x, pad):
  py, px = pad
  return np.pad(np.asarray(x), ((0, 0), (py, py), (px, px), (0, 0)), mode="wrap")


def loop(O, context, w_unet, x_T, window, stride, wrap, wy, wx, sched, gs, sampler="ddim", noises=None, weights=None,
         ms_update=None, plms_weights=None):
  """panorama_ref.loop with the wrapped gather and the weighted fold; arguments as there."""
  import torch
  x = torch.as_tensor(np.asarray(x_T), dtype=torch.float32)
  B, H, W, c = x.shape
  n_win = len(windows(H, W, window, stride, wrap))
  context = torch.as_tensor(context)
  ctx = torch.cat([context[:B].repeat_interleave(n_win, 0), context[B:].repeat_interleave(n_win, 0)])
  f = lambda key: np.asarray(sched[key]).astype(np.float32)
  c1, c2, a_prev = f("ddim_sqrt_recip_alphas_cumprod"), f("ddim_sqrt_recipm1_alphas_cumprod"), f("ddim_alphas_cumprod_prev")
  steps = sched["ddim_steps"]
  n = len(steps)
  hist = []
  for i in range(n - 1, -1, -1):
    rows = torch.from_numpy(np.ascontiguousarray(gather(x.numpy(), window, stride, wrap)).reshape(
        2 * B * n_win, window[0], window[1], c))
    t = np.full([2 * B * n_win], steps[i], dtype=np.int32)
    eps_win = O.unet_forward(rows, t, ctx, w_unet, torch.float32)
    eps = torch.from_numpy(fold(eps_win.numpy().reshape(2, B, n_win, window[0], window[1], c), H, W, window, stride,
                                wrap, wy, wx))
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
