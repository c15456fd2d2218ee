"""NumPy restatement of the antialiased resample, written from the rule and not from the product
code (ldm_tf2_amd/resample.py, csrc/resample.hip), shared by tests/test_resample_cpu.py and
tests/test_varsize_resample_gpu.py.

Per axis, with source extent L, output extent Lo, output index i and a filter of half-width r, in float64:
  scale = L / Lo, fs = max(scale, 1), support = r * fs, center = scale * (i + 0.5),
  xmin = max(0, int(center - support + 0.5)), xmax = min(L, int(center + support + 0.5)),
  w_j = filter((j - center + 0.5) / fs) for j in [xmin, xmax), normalised to sum 1.
Lo == L is the identity.  The image is resampled along W first, then along H.

`resample64` is that as two dense float64 matrices and einsum.  `tables32` lays an axis out the way the device reads it
(T taps per row, rows shifted inside [0, L), float32 weights rounded once from the float64 ones); `resample32` is a
float32 emulation on those tables in the order the kernel documents, acc = acc + w_j * x_j for ascending j from 0 with
the product and the sum rounded separately: its error against `resample64` is what float32 costs, the tests' gate.
"""
import numpy as np

FILTERS = ("triangle", "cubic", "lanczos3")
HALF_WIDTH = {"triangle": 1., "cubic": 2., "lanczos3": 3.}
# (H, W) -> (Ho, Wo): shrinking, enlarging, non-integer ratios, everything into one pixel, the identity, mixed axes
SHAPES = [((64, 64), (32, 32)), ((37, 53), (16, 24)), ((16, 16), (32, 32)), ((100, 60), (32, 32)), ((9, 7), (8, 8)),
          ((33, 33), (32, 32)), ((512, 384), (256, 256)), ((5, 5), (1, 1)), ((8, 8), (8, 8)), ((3, 200), (16, 16))]


def filter64(name, x):
  x = np.abs(np.asarray(x, dtype=np.float64))
  if name == "triangle":
    return np.maximum(0., 1. - x)
  if name == "cubic":                            # Keys, a = -0.5
    return np.where(x < 1., 1.5 * x ** 3 - 2.5 * x ** 2 + 1.,
                    np.where(x < 2., -0.5 * x ** 3 + 2.5 * x ** 2 - 4. * x + 2., 0.))
  if name == "lanczos3":
    return np.where(x < 3., np.sinc(x) * np.sinc(x / 3.), 0.)
  raise ValueError(name)


def axis_rows(L, Lo, name):
  """[(xmin_i, float64 weights over xmin_i .. xmax_i - 1)] for i < Lo."""
  if Lo == L:
    return [(i, np.ones(1)) for i in range(L)]
  scale = L / Lo
  fs = max(scale, 1.)
  support = HALF_WIDTH[name] * fs
  rows = []
  for i in range(Lo):
    center = scale * (i + 0.5)
    xmin = max(0, int(center - support + 0.5))
    xmax = min(L, int(center + support + 0.5))
    w = filter64(name, (np.arange(xmin, xmax) - center + 0.5) / fs)
    rows.append((xmin, w / w.sum()))
  return rows


def matrix64(L, Lo, name):
  m = np.zeros((Lo, L), dtype=np.float64)
  for i, (xmin, w) in enumerate(axis_rows(L, Lo, name)):
    m[i, xmin:xmin + len(w)] = w
  return m


def resample64(x, size, name):
  """x [B,H,W,c] -> float64 [B,Ho,Wo,c]."""
  x = np.asarray(x, dtype=np.float64)
  tmp = np.einsum("bhwc,ow->bhoc", x, matrix64(x.shape[2], size[1], name))
  return np.einsum("bhwc,oh->bowc", tmp, matrix64(x.shape[1], size[0], name))


def tables32(L, Lo, name):
  """(start int32 [Lo], weights float32 [Lo, T], T)."""
  rows = axis_rows(L, Lo, name)
  T = max(len(w) for _, w in rows)
  start = np.array([min(xmin, L - T) for xmin, _ in rows], dtype=np.int32)
  w64 = np.zeros((Lo, T), dtype=np.float64)
  for i, (xmin, w) in enumerate(rows):
    w64[i, xmin - start[i]:xmin - start[i] + len(w)] = w
  return start, w64.astype(np.float32), T


def _axis32(x, axis, L, Lo, name):
  start, w, T = tables32(L, Lo, name)
  x = np.moveaxis(x, axis, 0)                    # [L, ...]
  g = x[start[:, None] + np.arange(T)[None]]     # [Lo, T, ...]
  if T == 1:                                     # (a copy of the source bits)
    return np.moveaxis(g[:, 0], 0, axis)
  acc = np.zeros((Lo,) + x.shape[1:], dtype=np.float32)
  wb = w.reshape((Lo, T) + (1,) * (x.ndim - 1))
  for j in range(T):
    acc = (acc + (wb[:, j] * g[:, j]).astype(np.float32)).astype(np.float32)
  return np.moveaxis(acc, 0, axis)


def resample32(x, size, name):
  """x float32 [B,H,W,c] -> float32 [B,Ho,Wo,c], the float32 emulation."""
  x = np.asarray(x, dtype=np.float32)
  tmp = _axis32(x, 2, x.shape[2], size[1], name)
  return _axis32(tmp, 1, x.shape[1], size[0], name)


def crop_box(src, dst):
  """(y0, x0, hc, wc): the centred box of the source (Hs, Ws) with the aspect ratio of the target (H, W)."""
  (Hs, Ws), (H, W) = src, dst
  if Ws * H > Hs * W:
    wc = min(max((Hs * W + H // 2) // H, 1), Ws)
    return 0, (Ws - wc) // 2, Hs, wc
  hc = min(max((Ws * H + W // 2) // W, 1), Hs)
  return (Hs - hc) // 2, 0, hc, Ws
