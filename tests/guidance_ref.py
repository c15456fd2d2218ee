"""Guidance schedules restated in float64 NumPy.  Nothing here comes from the product; the
tests compare the product's table builder, its update kernel and its loops with these.

A loop has N DDIM indices with timesteps steps[N] and a guidance table g[N] (float32 values), indexed by DDIM index.
  table:  a float s and no interval: g = s everywhere; with an interval (t_lo, t_hi) in training timesteps:
          g[i] = s where t_lo <= steps[i] <= t_hi (both ends inclusive), 1 elsewhere; a sequence of N floats: itself.
  step i: guided (g[i] != 1):   e_i = eps_u + g[i] * (eps_c - eps_u)
          unguided (g[i] == 1): e_i = eps_c      (a definition; eps_u is neither computed nor read)
  e_i then enters the solver's update exactly as a guided eps does: e' = sum_{m <= j} w[m] e_{i+m} with the history
  ring shared by both kinds of step, x0 = c1 x - c2 e', x' = sqrt(a_prev) x0 + sqrt(1 - a_prev) e'
  (tests/deis_ref.py ms_update; DDIM at sigma = 0 is j = 0 with w = (1,); PLMS is tests/plms_ref.py's WEIGHTS).
"""
import numpy as np

import deis_ref as D
import plms_ref as P


def table(steps, scale, interval=None):
  """g[N] float32 from a float (with or without an interval) or a sequence of N floats."""
  steps = np.asarray(steps, dtype=np.int64)
  if np.ndim(scale) > 0:
    g = [float(v) for v in scale]
    assert len(g) == len(steps) and interval is None
  elif interval is None:
    g = [float(scale)] * len(steps)
  else:
    lo, hi = interval
    g = [float(scale) if lo <= int(t) <= hi else 1. for t in steps]
  return np.array(g, dtype=np.float64).astype(np.float32)


def guided(g):
  """Which indices run the guided form."""
  return [float(v) != 1. for v in np.asarray(g)]


def step_eps(eps_u, eps_c, gi):
  """e_i of one step; eps_u may be None for an unguided step."""
  if float(gi) == 1.:
    return eps_c
  return eps_u + gi * (eps_c - eps_u)


def plms_weight_table(n):
  """[N][4][4]: the Adams-Bashforth rows as a table (row [i][j] = plms_ref.WEIGHTS[j] for every i)."""
  w = np.zeros((n, 4, 4))
  for j in range(4):
    w[:, j, :j + 1] = P.WEIGHTS[j]
  return w


def sched_step(x, eps_u, eps_c, hist, g, i, j, w, c1, c2, a_prev):
  """One scheduled step at index i with j earlier eps in `hist` (hist[0] = e_{i+1}, ..): returns (x', x0, e_i).
  w = the weight row (j + 1 entries used), (1,) for DDIM.  Runs on NumPy arrays and torch tensors."""
  e_i = step_eps(eps_u, eps_c, g[i])
  x1, x0 = D.ms_update(x, [e_i] + list(hist[:j]), i, j, w, c1, c2, a_prev)
  return x1, x0, e_i
