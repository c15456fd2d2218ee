"""ldm_resample_nhwc on the GPU against the float64 restatement (tests/resample_ref.py): every
output element written once and nothing outside, every tap of every output pixel accounted for with exact one-hot
probes, the two paths bit for bit, the identity size a copy.

Gates.
  Random data: max |got - float64 restatement| <= max(2 * e32, 2^-23 * max|x|), where e32 is the same error of the
    float32 NumPy emulation (resample_ref.resample32: the same table layout, acc = acc + w_j * x_j for ascending j) on
    the same inputs, computed in the test; the factor 2 covers fused against separately rounded multiply-adds, as in
    tests/test_hires_gpu.py.  Never against the kernel's own output.
  Probes: a one-hot input of value 1 at source pixel (ys, xs) gives out[yo, xo] == float32(yw[yo, ys - ystart[yo]] *
    xw[xo, xs - xstart[xo]]), the product of the two float32 table entries rounded once (0 where a row does not reach
    the pixel): the W pass yields the weight itself and the H pass one product; adding zeros is exact.
  The identity size: the source bits.  A constant image: within 4 ulp of the constant, the bound DESIGN.md section 15
    states (a float64 emulation of the fused chain on these shapes and values stays within 3).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_ref as R  # noqa: E402
from ldm_tf2_amd import _lib, ops  # noqa: E402
from ldm_tf2_amd.resample import resample_taps  # noqa: E402

B = 2
SHAPES = [((37, 53), (16, 24)), ((9, 7), (8, 8)), ((16, 16), (32, 32)), ((5, 5), (1, 1)), ((33, 33), (32, 32))]
SHAPE_IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SHAPES]
CHANNELS = (3, 4, 5, 8)
FLOOR = 2.0 ** -23
CANARY = -12288.
PAD = 64                                         # floats around every output (a multiple of 4: the view stays aligned)


def _x(shape, seed=0):
  return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _offset_view(dev, numel, shape, offset, fill=CANARY):
  """A view `offset` floats into a canary-filled buffer, PAD floats of canary on both sides."""
  buf = torch.full((numel + 2 * PAD + offset,), fill, dtype=torch.float32, device=dev)
  view = buf[PAD + offset:PAD + offset + numel].view(shape)
  assert view.data_ptr() % 16 == (4 * offset) % 16
  return buf, view


def _resample_padded(dev, x, size, name, offset=0, in_offset=0):
  """The entry on `x` (itself a view `in_offset` floats off alignment) into a view `offset` floats into a canary-filled
  buffer -> the result (CPU); the pads are checked, and every element inside was written."""
  b, c = x.shape[0], x.shape[3]
  shape = (b, size[0], size[1], c)
  numel = int(np.prod(shape))
  buf, out = _offset_view(dev, numel, shape, offset)
  _, xin = _offset_view(dev, x.size, x.shape, in_offset)
  xin.copy_(torch.from_numpy(x))
  ops.resample_nhwc(xin, size, name, out=out)
  assert (buf[:PAD + offset] == CANARY).all() and (buf[PAD + offset + numel:] == CANARY).all()   # nothing outside
  got = out.cpu().numpy()
  if np.isfinite(x).all():
    assert np.isfinite(got).all() and not (got == CANARY).any()                                  # everything inside
  return got


# ---- 1. random data against the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("src,dst", SHAPES, ids=SHAPE_IDS)
def test_kernel_against_restatement(dev, src, dst, name):
  """c = 3, 5: the element path; c = 4, 8: channel quads; c = 4 and 8 once more on an output one float off alignment
  (the element path again).  The ratios err / e32 are printed."""
  for c, offset in [(c, 0) for c in CHANNELS] + [(4, 1), (8, 1)]:
    x = _x((B,) + src + (c,), seed=c)
    got = _resample_padded(dev, x, dst, name, offset)
    want = R.resample64(x, dst, name)
    e32 = np.abs(R.resample32(x, dst, name).astype(np.float64) - want).max()
    gate = max(2 * e32, FLOOR * np.abs(x).max())
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"{name} c={c} {src}->{dst} offset={offset}: err {err:.3e}, emulation {e32:.3e}, ratio "
          f"{err / e32 if e32 else float('nan'):.2f}, gate {gate:.3e}")
    assert err <= gate, (c, offset, err, gate)


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("src,dst", SHAPES, ids=SHAPE_IDS)
def test_both_paths_give_the_same_bits(dev, src, dst, name):
  """c % 4 == 0: 16-byte accesses on aligned pointers; the element-wise path when the output, or the input, is a view
  one float off."""
  for c in (4, 8):
    x = _x((B,) + src + (c,), seed=3)
    quad = _resample_padded(dev, x, dst, name)
    for offset, in_offset in ((1, 0), (0, 1)):
      elem = _resample_padded(dev, x, dst, name, offset, in_offset)
      assert np.array_equal(quad.view(np.uint32), elem.view(np.uint32)), (c, offset, in_offset)
    again = _resample_padded(dev, x, dst, name)                         # deterministic
    assert np.array_equal(quad.view(np.uint32), again.view(np.uint32))


# ---- 2. exact probes --------------------------------------------------------------------------------------
def _probe_want(src, dst, name):
  """want[p = ys * W + xs][yo][xo] = float32(yw * xw) of the table entries that reach (ys, xs), float32."""
  (H, W), (Ho, Wo) = src, dst
  ys_, yw, yt = resample_taps(H, Ho, name)
  xs_, xw, xt = resample_taps(W, Wo, name)
  wy = np.zeros((Ho, H), dtype=np.float32)       # dense float32 matrices of the two tables
  wx = np.zeros((Wo, W), dtype=np.float32)
  for i in range(Ho):
    wy[i, ys_[i]:ys_[i] + yt] = yw[i]
  for i in range(Wo):
    wx[i, xs_[i]:xs_[i] + xt] = xw[i]
  want = wy.T[:, None, :, None] * wx.T[None, :, None, :]       # [ys][xs][yo][xo]: one float32 product each
  assert want.dtype == np.float32
  return want.reshape(H * W, Ho, Wo)


@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("c,src,dst,offset", [(4, (9, 7), (8, 8), 0), (3, (9, 7), (8, 8), 0), (4, (5, 5), (1, 1), 0),
                                              (5, (5, 7), (16, 9), 0), (8, (6, 4), (3, 9), 1), (4, (8, 8), (8, 4), 0)])
def test_one_hot_probes(dev, c, src, dst, offset, name):
  """Image p of the batch is 1 at source pixel p (all channels) and 0 elsewhere: every output position of every probe
  must be the one product of the two table entries, bit for bit, and zero where no tap reaches the pixel.  One call
  per case: the probes are the batch."""
  n = src[0] * src[1]
  x = np.zeros((n,) + src + (c,), dtype=np.float32)
  x.reshape(n, n, c)[np.arange(n), np.arange(n)] = 1.
  got = _resample_padded(dev, x, dst, name, offset)
  want = _probe_want(src, dst, name)
  for ch in range(c):
    g = got[..., ch]
    assert np.array_equal(g, want), (ch, np.abs(g.astype(np.float64) - want).max())
    nz = want != 0
    assert np.array_equal(g[nz].view(np.uint32), want[nz].view(np.uint32))
  # the tables themselves are the rule: the total weight every source pixel receives, against the restatement
  ref = R.resample64(x[..., :1], dst, name)[..., 0]
  assert np.abs(want.astype(np.float64) - ref).max() <= 2.0 ** -22
  assert np.abs(ref.sum(axis=0) - 1.).max() <= 1e-12            # (every output's weights sum to 1)


# ---- 3. the identity size, a constant image, bad arguments ------------------------------------------------
@pytest.mark.parametrize("name", R.FILTERS)
@pytest.mark.parametrize("c", [3, 4])
def test_same_size_is_a_copy(dev, c, name):
  x = _x((B, 9, 7, c), seed=5)
  bits = x.view(np.uint32)
  x.flat[0] = -0.0
  bits.flat[1] = 0x7fc12345                       # a NaN with a payload
  bits.flat[2] = 0xff800000                       # -inf
  bits.flat[3] = 0x00000001                       # the smallest denormal
  for offset in (0, 1):
    got = _resample_padded(dev, x, (9, 7), name, offset)
    assert np.array_equal(got.view(np.uint32), bits)
  # one axis the same, the other not: the copied axis leaves the other's sums alone
  y = _x((B, 9, 7, c), seed=6)
  got = _resample_padded(dev, y, (9, 4), name)
  want = R.resample64(y, (9, 4), name)
  e32 = np.abs(R.resample32(y, (9, 4), name).astype(np.float64) - want).max()
  assert np.abs(got.astype(np.float64) - want).max() <= max(2 * e32, FLOOR * np.abs(y).max())


@pytest.mark.parametrize("name", R.FILTERS)
def test_constant_image_stays_constant(dev, name):
  for value in (0.7, 1e-3):
    v = np.float32(value)
    ulp = np.spacing(np.abs(v))
    for (src, dst), c in zip(SHAPES, (3, 4, 5, 8, 4)):
      x = np.full((B,) + src + (c,), v, dtype=np.float32)
      got = _resample_padded(dev, x, dst, name)
      dev_ulps = np.abs(got.astype(np.float64) - np.float64(v)).max() / ulp
      print(f"{name} {src}->{dst} c={c} value {value}: {dev_ulps:.2f} ulp")
      assert dev_ulps <= 4., (src, dst, c, value, dev_ulps)


def test_bad_arguments(dev):
  x = torch.zeros(2, 6, 5, 4, device=dev)
  tmp = torch.full((2, 6, 8, 4), CANARY, device=dev)
  out = torch.full((2, 8, 8, 4), CANARY, device=dev)
  ys, yw, yt = (torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in resample_taps(6, 8, "cubic"))
  xs, xw, xt = (torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in resample_taps(5, 8, "cubic"))
  s = torch.cuda.current_stream().cuda_stream
  lib = _lib.lib
  good = [x.data_ptr(), tmp.data_ptr(), out.data_ptr(), 2, 6, 5, 4, 8, 8, xs.data_ptr(), xw.data_ptr(), xt,
          ys.data_ptr(), yw.data_ptr(), yt, s]
  for k in (0, 1, 2, 9, 10, 12, 13):               # each pointer
    args = list(good)
    args[k] = None
    assert lib.ldm_resample_nhwc(*args) == _lib.ERR_ARG and "null pointer" in _lib.last_error(), k
  for k in (3, 4, 5, 6, 7, 8):                     # B, H, W, c, Ho, Wo
    for v in (0, -1):
      args = list(good)
      args[k] = v
      assert lib.ldm_resample_nhwc(*args) == _lib.ERR_ARG and "bad args" in _lib.last_error(), (k, v)
  for k, vals in ((11, (0, -1, 6)), (14, (0, -1, 7))):     # taps below 1, or above the axis's source extent (W = 5, H = 6)
    for v in vals:
      args = list(good)
      args[k] = v
      assert lib.ldm_resample_nhwc(*args) == _lib.ERR_ARG and "bad taps" in _lib.last_error(), (k, v)
  with pytest.raises(ValueError, match="resample filter"):
    ops.resample_nhwc(x, (8, 8), "bicubic", out=out)
  with pytest.raises(ValueError, match="positive"):
    ops.resample_nhwc(x, (8, 0), "cubic")
  torch.cuda.synchronize()
  assert (out == CANARY).all() and (tmp == CANARY).all()                     # nothing was launched
  assert lib.ldm_resample_nhwc(*good) == _lib.OK                            # (and the good call is good)
  torch.cuda.synchronize()
  assert not (out == CANARY).any() and (out == 0).all()
  assert _lib.RESAMPLE_FILTERS == R.FILTERS
