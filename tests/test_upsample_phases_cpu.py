"""layout.upsample_phase_kernel: the 3x3 convolution over the nearest-2x upsampled image equals four padded 2x2
convolutions over the image itself, interleaved into the output (float64, against the oracle), and the returned
matrix has the documented shape, phase order (p = 2a + b) and K order (tap (dy, dx) outer, ci inner)."""
import numpy as np
import torch

from ldm_tf2_amd import layout as L
from oracle import ldm_oracle as O


def apply_phases(x, w4):
  """x [B,H,W,Cin], w4 [4][Cout][4 Cin] -> [B,2H,2W,Cout]: output pixel (2i + a, 2j + b) = sum over the taps
  (dy, dx) of x[i - 1 + a + dy, j - 1 + b + dx] (zero outside the image) . w4[2a + b][:, (dy, dx, :)]."""
  B, H, W, Cin = x.shape
  Cout = w4.shape[1]
  xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=x.dtype)
  xp[:, 1:-1, 1:-1] = x
  out = torch.zeros(B, 2 * H, 2 * W, Cout, dtype=x.dtype)
  for a in range(2):
    for b in range(2):
      acc = torch.zeros(B, H, W, Cout, dtype=x.dtype)
      for dy in range(2):
        for dx in range(2):
          t = dy * 2 + dx
          wt = w4[2 * a + b][:, t * Cin:(t + 1) * Cin]                 # [Cout, Cin]
          src = xp[:, a + dy:a + dy + H, b + dx:b + dx + W]            # padded index = image index + 1
          acc += src @ wt.t()
      out[:, a::2, b::2] = acc
  return out


def test_phase_convolutions_equal_the_upsampled_convolution():
  g = np.random.default_rng(11)
  B, H, W, Cin, Cout = 2, 3, 5, 8, 6
  for _ in range(3):
    k = g.standard_normal((3, 3, Cin, Cout))
    x = torch.from_numpy(g.standard_normal((B, H, W, Cin)))
    w4 = L.upsample_phase_kernel(k, torch.float64, "cpu")
    assert tuple(w4.shape) == (4, Cout, 4 * Cin) and w4.dtype == torch.float64 and w4.is_contiguous()
    ref = O.conv2d(O.upsample_nearest2x(x), torch.from_numpy(k), None)
    got = apply_phases(x, w4)
    assert tuple(got.shape) == tuple(ref.shape) == (B, 2 * H, 2 * W, Cout)
    err = (got - ref).abs().max().item()
    print(f"max |phases - conv(upsample)| = {err:.3e}")
    assert err <= 1e-12


def test_shape_phase_order_and_tap_order():
  """A kernel whose entries encode (kh, kw, ci, co) in separate decimal digits: every element of the phase matrix
  is the sum of known entries, so a swapped phase, tap or channel order shows up exactly."""
  Cin, Cout = 3, 2
  k = np.zeros((3, 3, Cin, Cout))
  for kh in range(3):
    for kw in range(3):
      for ci in range(Cin):
        for co in range(Cout):
          k[kh, kw, ci, co] = 1000 * (kh + 1) + 100 * (kw + 1) + 10 * (ci + 1) + (co + 1)
  w4 = L.upsample_phase_kernel(k.astype(np.float32), torch.float32, "cpu")
  assert tuple(w4.shape) == (4, Cout, 4 * Cin) and w4.dtype == torch.float32
  rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}          # a (or b) -> per dy (or dx): the 3x3 rows (columns) summed
  for a in range(2):
    for b in range(2):
      for dy in range(2):
        for dx in range(2):
          for ci in range(Cin):
            for co in range(Cout):
              want = sum(k[kh, kw, ci, co] for kh in rows[a][dy] for kw in rows[b][dx])
              assert w4[2 * a + b, co, (dy * 2 + dx) * Cin + ci].item() == want, (a, b, dy, dx, ci, co)


def test_rounded_once_from_the_unrounded_sum():
  """bf16: the tap groups are summed before rounding (one rounding per phase weight, not one per tap)."""
  g = np.random.default_rng(5)
  k = g.standard_normal((3, 3, 4, 4)).astype(np.float32)
  w4 = L.upsample_phase_kernel(k, torch.bfloat16, "cpu")
  kk = torch.from_numpy(k).double()
  want = (kk[1, 1] + kk[1, 2] + kk[2, 1] + kk[2, 2]).t().to(torch.bfloat16)      # phase (0, 0), tap (1, 1)
  assert torch.equal(w4[0][:, 3 * 4:4 * 4], want)
