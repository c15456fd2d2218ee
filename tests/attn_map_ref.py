"""Restatements of ldm_xattn_map (include/ldm_hip.h) for the tests: `maps64`, the definition in
float64, and `maps32`, the kernel's own float32 operation order (fma chain over the head dims in ascending order, the
scale, the maximum, exp2, the ascending sum, one reciprocal, the product, the ascending head sum, 1 / heads, fma with
the weight).  Both take q [R,T,>=heads*sp] and k [R,Tk,>=heads*sp] as the exact float32 values handed to the kernel (a
bf16 tensor converted to float32) and return acc0 [R,T,Tk] plus the launch's increment."""
import numpy as np


def maps64(q, k, heads, S, sp, log2_scale, w, acc0):
  q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
  out = np.zeros((q.shape[0], q.shape[1], k.shape[1]), np.float64)
  for h in range(heads):
    qh, kh = q[..., h * sp:h * sp + S], k[..., h * sp:h * sp + S]
    l = float(log2_scale) * np.einsum("rtd,rjd->rtj", qh, kh)
    e = np.exp2(l - l.max(-1, keepdims=True))
    out += e / e.sum(-1, keepdims=True)
  return np.asarray(acc0, np.float64) + float(w) * out / heads


def maps32(q, k, heads, S, sp, log2_scale, w, acc0):
  f32 = np.float32
  q, k = np.asarray(q, f32), np.asarray(k, f32)
  R, T, Tk = q.shape[0], q.shape[1], k.shape[1]
  hs = np.zeros((R, T, Tk), f32)
  for h in range(heads):
    l = np.zeros((R, T, Tk), f32)
    for d in range(S):
      # fma: the product of two float32 is exact in float64, the sum is rounded once to float64 and once to float32
      prod = q[:, :, None, h * sp + d].astype(np.float64) * k[:, None, :, h * sp + d].astype(np.float64)
      l = (prod + l.astype(np.float64)).astype(f32)
    l = l * f32(log2_scale)
    e = np.exp2((l - l.max(-1, keepdims=True)).astype(np.float64)).astype(f32)
    s = np.zeros((R, T), f32)
    for j in range(Tk):
      s = s + e[..., j]
    inv = f32(1.) / s
    hs = hs + e * inv[..., None]
  v = hs * (f32(1.) / f32(heads))
  return (f32(w).astype(np.float64) * v.astype(np.float64) + np.asarray(acc0, f32).astype(np.float64)).astype(f32)


def gate(q, k, heads, S, sp, log2_scale, w, acc0):
  """(want float64, e32, delta): delta = max(2 e32, 8 * 2^-24 * w), the project's "twice the float32 emulation's
  error" rule with a floor of eight half-ulps of the largest possible increment w, one per rounding between a logit
  and the store (exp2, denominator, reciprocal, product, head sum, 1 / heads, w, accumulate)."""
  want = maps64(q, k, heads, S, sp, log2_scale, w, acc0)
  e32 = float(np.abs(maps32(q, k, heads, S, sp, log2_scale, w, acc0).astype(np.float64) - want).max())
  return want, e32, max(2. * e32, 8. * 2. ** -24 * abs(float(w)))
