"""DiffEdit restated in NumPy from DESIGN.md section 19.  Nothing here comes from the product.

Contrast map: for each noise draw r, in the order given, the model's eps under the source and the target prompt at one
level of x_r = q_sample(z0, t_m, M[r]); acc[b,p] += sum_j |e_tgt[b,p,j] - e_src[b,p,j]| -- in float32 exactly
  s = |d_0|; s = s + |d_j| for j = 1 .. c-1; acc = acc + s.
Mask: mean_b = sum_p acc[b,p] / (h w) (the sum in float64 here), thr_b = tau mean_b, edit = acc > thr_b written exactly
so (a NaN keeps the cell, an all-zero sample edits nothing), dilated by the OR over the (2 r + 1)^2 neighbourhood clipped
to the image; mask = 1 - edit.
Edit: inversion indices 0 .. k-1 from z0 keep traj[j], the latents on the level of steps[j]; sampling starts from
traj[k-1], and before the step at every index i < k-1, x <- m traj[i] + (1 - m) x (nothing is blended at index 0).
"""
import numpy as np

import inversion_ref as I


def contrast_accum(acc, e_src, e_tgt):
  """acc [B,...] + the contrast of e_src, e_tgt [B,...,c], float32 in the stated order; returns a new array."""
  e_src, e_tgt = np.asarray(e_src, dtype=np.float32), np.asarray(e_tgt, dtype=np.float32)
  acc = np.asarray(acc, dtype=np.float32)
  s = np.abs(e_tgt[..., 0] - e_src[..., 0])
  for j in range(1, e_src.shape[-1]):
    s = s + np.abs(e_tgt[..., j] - e_src[..., j])
  out = acc + s.reshape(acc.shape)
  assert out.dtype == np.float32
  return out


def dilate(edit, r):
  """edit bool [B,h,w] -> the OR over the (2 r + 1)^2 neighbourhood clipped to the image."""
  edit = np.asarray(edit, dtype=bool)
  B, h, w = edit.shape
  out = np.zeros_like(edit)
  for dy in range(-r, r + 1):
    for dx in range(-r, r + 1):
      ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
      xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
      out[:, yd, xd] |= edit[:, ys, xs]
  return out


def contrast_mask(acc, tau, r=0):
  """acc float32 [B,h,w] -> dict(mask float32 [B,h,w] (1 = keep), mean64, thr64 float64 [B], mean, thr float32 [B] (the
  float64 mean rounded once, and float32(tau) times it in float32), edited int [B]).  The comparison is float32 acc
  against the float32 threshold, as the device makes it."""
  acc = np.asarray(acc, dtype=np.float32)
  B, h, w = acc.shape
  mean64 = acc.astype(np.float64).reshape(B, -1).sum(axis=1) / (h * w)
  mean = mean64.astype(np.float32)
  thr = (np.float32(tau) * mean).astype(np.float32)
  edit = dilate(acc > thr[:, None, None], r)
  return dict(mask=(1 - edit).astype(np.float32), mean64=mean64, thr64=np.float64(np.float32(tau)) * mean64, mean=mean,
              thr=thr, edited=edit.reshape(B, -1).sum(axis=1).astype(np.int32))


def band(acc, tau):
  """bool [B,h,w]: the cells with |acc - tau mean64| <= 2 h w 2^-24 tau mean64, whose side of the threshold a legal
  summation order (within h w 2^-24 relative of the float64 sum, then two float32 roundings) may change."""
  acc = np.asarray(acc, dtype=np.float32)
  B, h, w = acc.shape
  mean64 = acc.astype(np.float64).reshape(B, -1).sum(axis=1) / (h * w)
  thr = np.float64(np.float32(tau)) * mean64
  return np.abs(acc.astype(np.float64) - thr[:, None, None]) <= (2. * h * w * 2. ** -24 * thr)[:, None, None]


# the random mask cases of the GPU test: (h, w, dilation, seed), B = 3 with sample 1 all zeros, tau = 1.5
MASK_CASES = ((1, 1, 0, 40), (5, 7, 1, 41), (16, 16, 3, 42), (64, 64, 1, 43), (8, 8192, 0, 44), (8, 8192, 3, 45))
MASK_TAU = 1.5


def mask_case_acc(case):
  """The input of one of MASK_CASES: fewer raised cells the wider the dilation, so that kept cells remain."""
  h, w, r, seed = case
  return random_acc(3, h, w, seed, zero_sample=1, frac=0.2 / (2 * r + 1) ** 2)


def random_acc(B, h, w, seed, zero_sample=None, frac=0.2):
  """Random positive maps float32 [B,h,w] whose threshold at tau = 1.5 falls into a gap of the values, so that band()
  is empty whatever h w: a fraction `frac` of the cells is uniform in [4.5, 5), the others in [0.5, 1) -- with a mean
  between 2 / 3 and 8 / 3 the threshold lies in [1, 4), where no value is, while band() reaches 2^-7 of it at most
  (tests/test_diffedit_cpu.py asserts the empty band for the shapes and seeds the GPU test uses).  The four corners are
  raised so that every dilation meets an edge.  `zero_sample`: that sample is all zeros."""
  g = np.random.default_rng(seed)
  acc = np.float32(0.5) + np.float32(0.5) * g.random((B, h, w), dtype=np.float32)
  acc = np.where(g.random((B, h, w)) < frac, acc + np.float32(4.), acc).astype(np.float32)
  for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
    acc[:, y, x] = np.float32(4.5)
  if zero_sample is not None:
    acc[zero_sample] = 0.
  return acc


def blend(m, traj_i, x):
  """m [B,h,w] over the channels: m traj_i + (1 - m) x in the dtype of x."""
  m = np.asarray(m, dtype=x.dtype)[..., None]
  return m * np.asarray(traj_i, dtype=x.dtype) + (1 - m) * x


def diffedit_loop(eps_src, eps_tgt, z0, mask, g_inv, g, k, steps, tables, record=None, dtype=np.float64):
  """The masked edit composed from inversion_ref's loops: eps_src / eps_tgt(x, t) -> (e_u, e_c) under the source /
  target prompt.  Returns (x after index 0, traj [k,...])."""
  traj = []
  I.invert_loop(eps_src, z0, g_inv, k, steps, tables, record=traj, dtype=dtype)
  x = traj[k - 1]
  for i in range(k - 1, -1, -1):
    e_u, e_c = eps_tgt(x, int(steps[i]))
    e_u = None if e_u is None else np.asarray(e_u, dtype=dtype)
    x, _ = I.forward_update(x, I.guided(e_u, np.asarray(e_c, dtype=dtype), g), i, tables)
    if i >= 1:
      x = blend(mask, traj[i - 1], x)
    assert x.dtype == dtype
    if record is not None:
      record.append(x.copy())
  return x, np.stack(traj)
