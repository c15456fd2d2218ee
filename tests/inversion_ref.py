"""DDIM inversion restated in NumPy from DESIGN.md section 13 (float64 unless a caller asks for float32).

N DDIM steps walk the table steps[0] < .. < steps[N-1].  The sampling step at index i maps x on level steps[i] to x' on
the level below it, training timestep t_in[i] (t_in[0] = 0, t_in[i] = steps[i-1]; abar[t_in[i]] = a_prev[i]):
  x0 = c1[i] x - c2[i] e          x' = sqrt(a_prev[i]) x0 + sqrt(1 - a_prev[i]) e
with c1 = sqrt(1 / abar[steps[i]]), c2 = sqrt(1 / abar[steps[i]] - 1).  The inversion step at index i maps x' back:
  e  = eps(x', t_in[i])            (the model is asked at the level its input is on)
  e  = e_c when g == 1, else e_u + g (e_c - e_u)
  x0 = (x' - sqrt(1 - a_prev[i]) e) / sqrt(a_prev[i])
  x  = (x0 + c2[i] e) / c1[i]
An inversion of depth k runs indices 0 .. k-1 from z0; no noise, no clip, first order.

Nothing here comes from the product.  The arithmetic uses + - * / and sqrt on arrays of the dtype the caller chose, so
the same functions give the float32 emulation the tests take their margins from.
"""
import numpy as np


def t_in(steps):
  """The training timestep of the level below each DDIM index."""
  steps = np.asarray(steps)
  return np.concatenate([[0], steps[:-1]]).astype(steps.dtype)


def make_tables(alphas_cumprod, steps, dtype=np.float64):
  """c1, c2, a_prev [N] as the device holds them: float64 values cast to float32 (the product's `_extract`), then
  widened to `dtype`."""
  ac = np.asarray(alphas_cumprod, dtype=np.float64)
  steps = np.asarray(steps)
  f = lambda a: a.astype(np.float32).astype(dtype)
  return dict(c1=f(np.sqrt(1. / ac)[steps]), c2=f(np.sqrt(1. / ac - 1.)[steps]), a_prev=f(ac[t_in(steps)]))


def guided(e_u, e_c, g):
  """g == 1: the conditional eps by definition (e_u is not touched and may be None)."""
  if g == 1:
    return e_c
  return e_u + e_u.dtype.type(g) * (e_c - e_u)


def forward_update(x, e, i, tables):
  """The sigma = 0 sampling step at index i given e: returns (x', x0)."""
  a = tables["a_prev"][i]
  x0 = tables["c1"][i] * x - tables["c2"][i] * e
  return np.sqrt(a) * x0 + np.sqrt(1 - a) * e, x0


def invert_update(x, e_u, e_c, g, i, tables):
  """The inversion step at index i given the two halves of eps: returns (x on level steps[i], x0)."""
  e = guided(e_u, e_c, g)
  a = tables["a_prev"][i]
  x0 = (x - np.sqrt(1 - a) * e) / np.sqrt(a)
  return (x0 + tables["c2"][i] * e) / tables["c1"][i], x0


def invert_loop(eps_fn, z0, g, k, steps, tables, record=None, dtype=np.float64):
  """Inversion indices 0 .. k-1 from z0.  eps_fn(x, t) -> (e_u, e_c): the model's two eps halves for x at training
  timestep t (e_u may be None when g == 1).  Returns x on the level of steps[k-1]."""
  x = np.asarray(z0, dtype=dtype)
  tin = t_in(steps)
  for i in range(k):
    e_u, e_c = eps_fn(x, int(tin[i]))
    e_u = None if e_u is None else np.asarray(e_u, dtype=dtype)
    x, _ = invert_update(x, e_u, np.asarray(e_c, dtype=dtype), g, i, tables)
    if record is not None:
      record.append(x.copy())
  return x


def sample_loop(eps_fn, x, g, k, steps, tables, record=None, dtype=np.float64):
  """Sampling indices k-1 .. 0 (sigma = 0, first order) from x on the level of steps[k-1]; eps_fn as above, asked at
  steps[i]."""
  x = np.asarray(x, dtype=dtype)
  for i in range(k - 1, -1, -1):
    e_u, e_c = eps_fn(x, int(steps[i]))
    e_u = None if e_u is None else np.asarray(e_u, dtype=dtype)
    x, _ = forward_update(x, guided(e_u, np.asarray(e_c, dtype=dtype), g), i, tables)
    if record is not None:
      record.append(x.copy())
  return x
