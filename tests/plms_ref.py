"""PLMS (pseudo linear multistep, Liu et al. 2022) restated in float64 NumPy from DESIGN.md section 8.

A loop runs indices start, start-1, .., 0.  At index i, with j = min(start - i, 3) earlier steps in this loop
and e_k the model's eps at index k:
  j=0: e' = e_i                        j=1: e' = (3 e_i - e_{i+1}) / 2
  j=2: e' = (23 e_i - 16 e_{i+1} + 5 e_{i+2}) / 12
  j=3: e' = (55 e_i - 59 e_{i+1} + 37 e_{i+2} - 9 e_{i+3}) / 24
  x0 = c1[i] x - c2[i] e'        x' = sqrt(a_prev[i]) x0 + sqrt(1 - a_prev[i]) e'
with c1 = sqrt(1 / abar), c2 = sqrt(1 / abar - 1).  A step without history is the DDIM step at sigma = 0.

Nothing here comes from the product; WEIGHTS is this file's own literal copy (tests compare it with
model_runners.PLMS_WEIGHTS).  The arithmetic uses only + - * and sqrt, so `plms_update` also runs on torch
tensors (the GPU tests compose it with the oracle's U-Net in float32).
"""
import numpy as np

WEIGHTS = (
    (1.,),
    (3. / 2., -1. / 2.),
    (23. / 12., -16. / 12., 5. / 12.),
    (55. / 24., -59. / 24., 37. / 24., -9. / 24.),
)
ABS_WEIGHT_SUMS = (1., 2., 11. / 3., 20. / 3.)          # sum_k |w_jk|: what row j does to a rounding error in eps


def plms_eps(eps_hist, j):
  """e' of order j: eps_hist[0] = e_i, eps_hist[k] = e_{i+k}; entries beyond j are not touched."""
  e = WEIGHTS[j][0] * eps_hist[0]
  for k in range(1, j + 1):
    e = e + WEIGHTS[j][k] * eps_hist[k]
  return e


def plms_update(x, eps_hist, i, j, c1, c2, a_prev):
  """One step at index i: returns (x', x0).  c1, c2, a_prev are tables indexed by i (any float type; the
  square roots are taken in the type of the entries)."""
  e = plms_eps(eps_hist, j)
  x0 = c1[i] * x - c2[i] * e
  a = a_prev[i]
  return np.sqrt(a) * x0 + np.sqrt(1 - a) * e, x0


def plms_loop(eps_fn, x, ab, ab_prev, start, max_order=3):
  """Indices start .. 0 from x.  ab[i] = abar at index i's timestep, ab_prev[i] = abar the step lands on;
  eps_fn(x, i) = the model's eps at index i.  max_order = 0 is the DDIM loop at sigma = 0.  float64."""
  ab = np.asarray(ab, dtype=np.float64)
  ab_prev = np.asarray(ab_prev, dtype=np.float64)
  c1 = np.sqrt(1. / ab)
  c2 = np.sqrt(1. / ab - 1.)
  x = np.asarray(x, dtype=np.float64)
  hist = []
  for i in range(start, -1, -1):
    hist.insert(0, eps_fn(x, i))
    del hist[4:]
    x, _ = plms_update(x, hist, i, min(start - i, max_order), c1, c2, ab_prev)
  return x


# ---- a data distribution whose eps is known in closed form ---------------------------------------------
GM_MEANS = np.array([-1.5, 0.7, 2.0])
GM_STDS = np.array([0.3, 0.5, 0.2])
GM_WEIGHTS = np.array([0.3, 0.5, 0.2])


def mixture_eps(x, abar):
  """Exact eps of the 1-D Gaussian mixture above diffused to abar (alpha = sqrt(abar), sigma = sqrt(1 - abar)):
  p_t = sum_c w_c N(alpha mu_c, alpha^2 s_c^2 + sigma^2); eps* = -sigma * d/dx log p_t, per element."""
  x = np.asarray(x, dtype=np.float64)[..., None]
  alpha, sigma = np.sqrt(abar), np.sqrt(1. - abar)
  var = alpha * alpha * GM_STDS ** 2 + sigma * sigma
  d = x - alpha * GM_MEANS
  logp = np.log(GM_WEIGHTS) - 0.5 * np.log(2 * np.pi * var) - 0.5 * d * d / var
  logp -= logp.max(axis=-1, keepdims=True)
  post = np.exp(logp)
  post /= post.sum(axis=-1, keepdims=True)
  score = (post * (-d / var)).sum(axis=-1)
  return -sigma * score
