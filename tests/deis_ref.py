"""Non-uniform step tables and the table-weighted multistep update ("deis"), restated in
float64 NumPy.  Nothing here comes from the product; the tests compare the product's tables, weights and loop with
these.

Schedule: betas = linspace(sqrt(b0), sqrt(b1), T)^2 formed in float32, abar = cumprod(1 - betas) in float64.
lambda(t) = 0.5 * ln(abar[t] / (1 - abar[t])) (half the log signal-to-noise ratio; it falls as t rises).

Step tables for N steps, top = the last entry of the uniform table arange(0, T, T // N) + 1:
  logsnr: targets linspace(lambda(0), lambda(top), N + 1)[1:]
  karras: sigma(t) = sqrt((1 - abar) / abar), rho = 7,
          targets -ln(linspace(sigma(0)^(1/rho), sigma(top)^(1/rho), N + 1)[1:] ** rho)
  each target -> the integer timestep with the nearest lambda, at least 1; walking upward
  t_j = max(t_j, t_{j-1} + 1); the last entry is set to top.

Weights.  A loop runs DDIM indices start .. 0.  At index i with j = min(start - i, 3) earlier steps, nodes
l_0 = lambda(steps[i]), l_m = lambda(steps[i + m]) and target l' = lambda of a_prev[i]:
  w[m] = int_{l_0}^{l'} e^{-l} L_m(l) dl / int_{l_0}^{l'} e^{-l} dl,   L_m the Lagrange basis on l_0 .. l_j
  e' = sum_m w[m] e_{i+m};   x0 = c1 x - c2 e';   x' = sqrt(a_prev) x0 + sqrt(1 - a_prev) e'
With l = l_0 + h s, h = l' - l_0 > 0, the ratio is int_0^1 e^{-h s} L_m(s) ds / int_0^1 e^{-h s} ds, L_m on the nodes
s_k = (l_k - l_0) / h.  Two evaluations: `weights_closed` expands L_m in powers of s and uses the moments
M_k = int_0^1 s^k e^{-h s} ds in closed form; `weights_gauss` is Gauss-Legendre quadrature.
"""
import math

import numpy as np

SPACINGS = ("uniform", "logsnr", "karras")
RHO = 7.


def alphas_cumprod(num_steps=1000, beta_start=0.00085, beta_end=0.012):
  a, b = np.float32(beta_start ** 0.5), np.float32(beta_end ** 0.5)
  delta = np.float32((b - a) / np.float32(num_steps - 1))
  ls = np.concatenate([[a], (a + delta * np.arange(1, num_steps - 1, dtype=np.float32)).astype(np.float32), [b]])
  ls = ls.astype(np.float32)
  betas = (ls * ls).astype(np.float32).astype(np.float64)
  return np.cumprod(1. - betas)


def lam(abar):
  abar = np.asarray(abar, dtype=np.float64)
  return 0.5 * np.log(abar / (1. - abar))


def uniform_table(n, num_steps=1000):
  steps = np.arange(0, num_steps, num_steps // n, dtype=np.int64)
  return steps + 1 if n < num_steps else steps


def step_table(abar, n, spacing):
  """The N ascending integer timesteps of `spacing` on the schedule `abar`."""
  num_steps = len(abar)
  uni = uniform_table(n, num_steps)
  if spacing == "uniform":
    return uni
  top = int(uni[-1])
  lm = lam(abar)
  if spacing == "logsnr":
    targets = np.linspace(lm[0], lm[top], n + 1)[1:]
  elif spacing == "karras":
    sig = np.sqrt((1. - abar) / abar)
    targets = -np.log(np.linspace(sig[0] ** (1. / RHO), sig[top] ** (1. / RHO), n + 1)[1:] ** RHO)
  else:
    raise ValueError(spacing)
  out = []
  for tg in targets:
    t = max(int(np.argmin(np.abs(lm - tg))), 1)
    if out:
      t = max(t, out[-1] + 1)
    out.append(t)
  out[-1] = top
  return np.array(out, dtype=np.int64)


def derived_tables(abar, steps):
  """(abar at the steps, a_prev) as the sampler defines them: a_prev[0] = abar[0]."""
  steps = np.asarray(steps)
  return abar[steps], np.concatenate([[abar[0]], abar[steps[:-1]]])


# ---- weights ---------------------------------------------------------------------------------------------------
def _lagrange_coeffs(nodes):
  """Row m = coefficients (ascending powers) of the Lagrange basis polynomial L_m on `nodes`."""
  n = len(nodes)
  out = np.zeros((n, n))
  for m in range(n):
    p = np.array([1.])
    for k in range(n):
      if k != m:
        p = np.convolve(p, np.array([-nodes[k], 1.])) / (nodes[m] - nodes[k])
    out[m, :len(p)] = p
  return out


def _moments(h, kmax):
  """M_k = int_0^1 s^k e^{-h s} ds, k = 0 .. kmax.  h >= 1: M_0 = (1 - e^{-h}) / h, M_k = (k M_{k-1} - e^{-h}) / h.
  h < 1 (where that recurrence cancels): the same integral as the series e^{-h} sum_n h^n k! / (k + n + 1)!,
  all terms positive."""
  if h >= 1.:
    m = [(1. - math.exp(-h)) / h]
    for k in range(1, kmax + 1):
      m.append((k * m[-1] - math.exp(-h)) / h)
    return np.array(m)
  out = []
  for k in range(kmax + 1):
    term, total, n = 1. / (k + 1), 0., 0           # k! / (k + 1)!
    while term > 1e-20 * max(total, 1e-300):
      total += term
      n += 1
      term *= h / (k + n + 1)
    out.append(math.exp(-h) * total)
  return np.array(out)


def weights_closed(lams, lam_target):
  """lams = (l_0, .., l_j) -> the j + 1 weights, closed form."""
  lams = np.asarray(lams, dtype=np.float64)
  h = float(lam_target - lams[0])
  coeffs = _lagrange_coeffs((lams - lams[0]) / h)
  mom = _moments(h, len(lams) - 1)
  return coeffs @ mom / mom[0]


def weights_gauss(lams, lam_target, points=32):
  """The same weights by `points`-point Gauss-Legendre quadrature on s in [0, 1]."""
  lams = np.asarray(lams, dtype=np.float64)
  h = float(lam_target - lams[0])
  nodes = (lams - lams[0]) / h
  x, wq = np.polynomial.legendre.leggauss(points)
  s = 0.5 * (x + 1.)
  ex = np.exp(-h * s)
  den = float(np.sum(wq * ex))
  out = []
  for m in range(len(nodes)):
    L = np.ones_like(s)
    for k in range(len(nodes)):
      if k != m:
        L = L * (s - nodes[k]) / (nodes[m] - nodes[k])
    out.append(float(np.sum(wq * ex * L)) / den)
  return np.array(out)


def weight_table(abar, steps, fn=weights_closed):
  """[N][4][4] float64: row [i][j] = the weights of the step at DDIM index i with j earlier steps (j + 1 entries, the
  rest zero); rows with i + j >= N (no such history exists) stay zero."""
  ab, ab_prev = derived_tables(abar, steps)
  l, lp = lam(ab), lam(ab_prev)
  n = len(steps)
  w = np.zeros((n, 4, 4))
  for i in range(n):
    for j in range(min(3, n - 1 - i) + 1):
      w[i, j, :j + 1] = fn(l[i:i + j + 1], lp[i])
  return w


def ms_eps(eps_hist, w, j):
  """e' = sum_{m <= j} w[m] e_{i+m}, accumulated m = 0 .. j; entries beyond j are not touched."""
  e = w[0] * eps_hist[0]
  for m in range(1, j + 1):
    e = e + w[m] * eps_hist[m]
  return e


def ms_update(x, eps_hist, i, j, w, c1, c2, a_prev):
  """One step at index i with the weight row w (j + 1 entries used): returns (x', x0).  Runs on NumPy arrays and on
  torch tensors (only + - * and the square roots of table entries)."""
  e = ms_eps(eps_hist, w, j)
  x0 = c1[i] * x - c2[i] * e
  a = a_prev[i]
  return np.sqrt(a) * x0 + np.sqrt(1 - a) * e, x0


def ms_loop(eps_fn, x, ab, ab_prev, start, wtab, max_order=3):
  """Indices start .. 0 from x with the weight table wtab [N][4][4]; eps_fn(x, i) = the model's eps at index i."""
  ab = np.asarray(ab, dtype=np.float64)
  ab_prev = np.asarray(ab_prev, dtype=np.float64)
  c1, c2 = np.sqrt(1. / ab), np.sqrt(1. / ab - 1.)
  x = np.asarray(x, dtype=np.float64)
  hist = []
  for i in range(start, -1, -1):
    hist.insert(0, eps_fn(x, i))
    del hist[4:]
    j = min(start - i, max_order)
    x, _ = ms_update(x, hist, i, j, wtab[i][j], c1, c2, ab_prev)
  return x


# ---- the golden step tables (tests/golden/step_tables.json): `python tests/deis_ref.py` rewrites the file --------
GOLDEN_SCHEDULE = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012)
GOLDEN_N = (8, 10, 20, 25, 50)


def golden_tables():
  ab = alphas_cumprod(**GOLDEN_SCHEDULE)
  return dict(schedule=GOLDEN_SCHEDULE,
              tables={sp: {str(n): step_table(ab, n, sp).tolist() for n in GOLDEN_N} for sp in ("logsnr", "karras")})


if __name__ == "__main__":
  import json
  import os
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_tables.json")
  with open(path, "w") as f:
    json.dump(golden_tables(), f, indent=1)
    f.write("\n")
  print("wrote", path)
