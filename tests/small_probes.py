"""Probes for the small kernels of the sampling path (csrc/misc.hip and softmax_rows_kernel of csrc/norms.hip): case lists
placed on each kernel's own edges, expected outputs, float64 references and plain models of each kernel's WORK
DECOMPOSITION with switchable faults (a plain module, imported by test_small_probes_cpu.py and
test_small_kernels_gpu.py; torch on the CPU only).

Exact probes (gate: torch.equal, no tolerance)
  convs, census        all-ones image, every weight 2^-3, bias u * {-2..2} with u = Cin 2^-3: each output is
                       u * (number of in-image taps: 9 / 6 / 4, fewer on one-line images) + bias.
  convs, selection     one hot pixel in every 3 x 3 window (the lattice y % 3 = ry, x % 3 = rx), hot at ONE channel
                       ci = (b + y + 2 x) % Cin; weight (kh, kw, ci, co) = wcode(n), n = ((3 kh + kw) Cin + ci) Cout + co,
                       all distinct, each with an 8-bit mantissa (exact in bf16).  Every output is ONE weight or 0.
  gemv (no activation) integer x, w and bias: every partial sum is an integer below 2^24.
  vq_nearest           integer z and codebook; planted duplicates of the nearest row (vq_plants); expected index = the
                       first minimum of the float64 distances.
  minmax_u8            integer images with ONE 0 and ONE 255 placed at the first / last element or in the slice of
                       reduction block 63; every other byte value is one for which trunc((v / 255) * 255) = v in
                       float32 (u8_safe: the CPU test shows that all 256 are), so out = x.
  cast                 bit equality with Tensor.to on the CPU (NaN stays NaN); special values first (ties between two
                       bf16 neighbours with both parities of the lower one, -0, +-inf, NaN, denormals, the largest
                       finite float), then random bit patterns.
  embedding            ids with -1, vocab, vocab + 5: the clamped lookup; float32 is one add (bit-exact), bf16 is that
                       sum rounded once.
All operands are views of NaN-filled buffers (channel offset, row pitch > C): a read outside the operand poisons the
result; the GPU test asserts that the output buffer is still NaN outside the region the launch owns.

Float64 references (gemv with SiLU, softmax_rows, post_quant, gaussian_sample, time_embedding, random-data convs)
  Computed from the exact values the kernel is given (bf16 / float32 widened to float64).  A case's FIGURE is
      max |kernel - ref64|  /  max(max |oracle - ref64|, u max |ref64|)
  where `oracle` is oracle/ldm_oracle.py's float32 computation on the CPU rounded to the output type and u is the unit
  roundoff of the output type: 2^-24 (float32) or 2^-8 (bf16, 8 significant bits).  With float32 output the floor only
  keeps a case in which the oracle happens to be exact (one softmax column) from dividing by 0.  With bf16 output it
  usually IS the denominator: the oracle's error there is one bf16 rounding of some output, which u max |ref64| bounds
  from above, so a bf16 figure reads "kernel error in units of one bf16 rounding of the largest output" (about 0.5
  for a kernel that rounds once), not a ratio to the oracle's own error.
  GATES holds, per entry point and type, twice the largest figure of the first run on an MI355X rounded up to one
  significant digit (the factor 2 is for input seeds; the inputs are seeded).  Besides its gate every case must meet
  the CEILING: the rtol / atol the older test of the same op applies (test_ops_gpu.py, test_encoder_gpu.py), now
  against float64.  Where no older test exists the ceiling is derived from the number format (post_quant bf16 out:
  one bf16 rounding, at most 2^-8 relative with 8 significant bits, on top of the float32 ceiling).

  Bounds chosen here, with their reasoning
    softmax row sum    |sum of a float32 output row - 1| <= 28 * 2^-24.  The row sum s is accumulated in at most 16
                       serial adds per thread, 6 shuffle levels and 3 adds (25 roundings of 2^-24 relative), 1 / s and
                       the product add 2 more and the outputs' own rounding 1; both passes evaluate the same __expf
                       of the same argument.  28 is that count: every rounding at its worst and all of one sign.
    frequencies        with t = 1 the sine half is sin(f); for k >= half / 2, f <= 0.01 and f = asin(out) to rounding
                       level.  f = expf(e), e = -logf(1e4) k / half: |e| <= 9.2104 carries the rounding of logf(1e4)
                       (representation + 1 ulp), of the product and of the quotient, 4 * 2^-24 * 9.2104 = 2.2e-6
                       relative in f; expf and sinf add 2 ulp each (2.4e-7 each).  Bound: 3e-6 relative.  A wrong
                       constant in the 6th digit is an error of 1e-5.

MEASURED (MI355X, first run; figure = kernel error / oracle error as defined above, largest over the cases)
  entry point, input / weight type, output type: the largest figure, its gate, and the largest share of the ceiling
  (worst |kernel - ref64| / (atol + rtol |ref64|)) any case used.  289 cases passed on that run; every exact probe
  (convs census + selection, gemv, vq_nearest, minmax_u8, cast, embedding) was equal; the largest softmax row-sum
  error was 1.5e-7 and the largest frequency error 5.7e-7 (the oracle's own: 5.7e-7).  No kernel needed a change
  beyond the vq_nearest index fix made with this module.
  conv_in bf16 bf16            figure 0.568    gate 2      share of the ceiling used 0.156
  conv_in f32 f32              figure 1.706    gate 4      share of the ceiling used 0.005
  conv_lds bf16 bf16           figure 0.498    gate 1      share of the ceiling used 0.114
  conv_lds bf16 f32            figure 2.318    gate 5      share of the ceiling used 0.000
  conv_lds f32 bf16            figure 0.509    gate 2      share of the ceiling used 0.156
  conv_lds f32 f32             figure 1.732    gate 4      share of the ceiling used 0.005
  conv_out bf16 bf16           figure 0.577    gate 2      share of the ceiling used 0.156
  conv_out bf16 f32            figure 1.048    gate 3      share of the ceiling used 0.000
  conv_out f32 bf16            figure 0.602    gate 2      share of the ceiling used 0.109
  conv_out f32 f32             figure 0.645    gate 2      share of the ceiling used 0.009
  gaussian_sample f32          figure 0.874    gate 2      share of the ceiling used 0.059
  gemv bf16                    figure 1.325    gate 3      share of the ceiling used 0.002
  gemv f32                     figure 1.925    gate 4      share of the ceiling used 0.003
  post_quant bf16              figure 0.891    gate 2      share of the ceiling used 0.983
  post_quant f32               figure 1.272    gate 3      share of the ceiling used 0.125
  softmax_rows bf16 bf16       figure 0.468    gate 1      share of the ceiling used 0.060
  softmax_rows bf16 f32        figure 1.247    gate 3      share of the ceiling used 0.000
  softmax_rows f32 bf16        figure 0.435    gate 0.9    share of the ceiling used 0.050
  softmax_rows f32 f32         figure 1.815    gate 4      share of the ceiling used 0.000
  time_embedding f32           figure 2.040    gate 5      share of the ceiling used 0.293
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

F32, BF, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
NAN = float("nan")
DTN = {F32: "f32", BF: "bf16"}

# ---- the numbers of csrc/misc.hip (the CPU test reads them back from the source text) ----------------------
LDS_CAP, IN_CAP, OUT_CAP = 768, 8192, 4096          # workgroups: conv_in_lds / conv_small_in / conv_small_out
LDS_BYTES = 64 * 1024
OUT_PIX_PER_WG = 32
DEFAULT_CAP = 4096                                   # grid_for's default: cast, embedding, post_quant, gaussian_sample
MINMAX_BLOCKS = 64
GEMV_RT = 4


def u_of(dtype):
  return 2.0 ** -8 if dtype == BF else 2.0 ** -24


def rnd(shape, seed, scale=1.0):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F32) * scale


def ints(shape, seed, lo, hi):
  return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed), dtype=I64)


def representable(ref, dtype):
  """True if every value of the float64 tensor `ref` survives the round trip through `dtype`."""
  return bool((ref.to(dtype).to(F64) == ref).all())


def strided(rows, cols, off, pad, dtype, data=None, device="cpu", tail=64):
  """(flat, view): a [rows, cols] view with row pitch off + cols + pad, starting `off` elements into a NaN-filled flat
  buffer that ends with `tail` more NaNs.  `data` (anything [rows, cols]-shaped) is rounded to `dtype` on the CPU."""
  ld = off + cols + pad
  flat = torch.full((rows * ld + tail,), NAN, dtype=dtype)
  if data is not None:
    flat[:rows * ld].view(rows, ld)[:, off:off + cols] = data.reshape(rows, cols).to(dtype)
  flat = flat.to(device)
  return flat, flat[:rows * ld].view(rows, ld)[:, off:off + cols]


def figure(got, orc, ref, odt):
  """(kernel error, oracle error, figure) of the module docstring; all float64 on the CPU.  A non-finite kernel value
  gives an infinite error."""
  kerr = (got - ref).abs()
  kerr = float(torch.where(torch.isfinite(got), kerr, torch.full_like(kerr, math.inf)).max())
  oerr = max(float((orc - ref).abs().max()), u_of(odt) * float(ref.abs().max()))
  return kerr, oerr, kerr / oerr


def within(got, ref, rtol, atol):
  """The older tests' allclose, against float64: the worst |got - ref| / (atol + rtol |ref|), <= 1 passes."""
  r = (got - ref).abs() / (atol + rtol * ref.abs())
  return float(torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf)).max())


# ============================================================================================================
# ldm_conv3x3_small
# ============================================================================================================
def conv_kernel_of(c):
  """The dispatch of ldm_conv3x3_small restated: 'lds' (conv_in_lds_kernel), 'in' (conv_small_in_kernel) or 'out'
  (conv_small_out_kernel).  Buffers start 16-byte aligned, so a view's alignment is that of its channel offset."""
  isz, osz = (2 if c.idt == BF else 4), (2 if c.odt == BF else 4)
  ldx, ldo = c.xoff + c.Cin + c.xpad, c.ooff + c.Cout + c.opad
  x16, o16 = (c.xoff * isz) % 16 == 0, (c.ooff * osz) % 16 == 0
  if (c.Cin == 4 and c.Cout % 8 == 0 and 9 * c.Cin * c.Cout * 4 <= LDS_BYTES and ldo % 8 == 0 and o16 and
      (c.idt != F32 or (ldx % 4 == 0 and x16))):
    return "lds"
  if c.Cin <= 8:
    assert c.Cout % 4 == 0
    return "in"
  epc = 8 if c.idt == BF else 4
  assert c.Cout <= 4 and c.Cin % epc == 0 and ldx % epc == 0 and x16 and 9 * c.Cin * c.Cout * 4 <= LDS_BYTES
  return "out"


def _conv(B, H, W, Cin, Cout, idt, odt, xoff=0, xpad=0, ooff=0, opad=0, bias=1, rand=0, phases=((0, 0), (1, 2)), tag=""):
  c = NS(B=B, H=H, W=W, Cin=Cin, Cout=Cout, idt=idt, odt=odt, xoff=xoff, xpad=xpad, ooff=ooff, opad=opad, bias=bias,
         rand=rand, phases=phases, tag=tag)
  c.kernel = conv_kernel_of(c)
  c.id = (f"{c.kernel}-{DTN[idt]}-{DTN[odt]}-{B}x{H}x{W}-c{Cin}-{Cout}" + ("" if bias else "-nobias") +
          (f"-x{xoff}+{xpad}" if xoff or xpad else "") + (f"-o{ooff}+{opad}" if ooff or opad else "") +
          (f"-{tag}" if tag else ""))
  return c


def conv_cases():
  one = ((1, 2),)
  return [
      # conv_in_lds_kernel: W % 4 in {3, 1, 2, 0}, both input types, the LDS edge (Cout = 448), one pixel
      _conv(2, 5, 7, 4, 16, F32, F32, xoff=4, xpad=4, ooff=8, opad=8, rand=1),
      _conv(1, 3, 5, 4, 8, BF, BF, xoff=3, xpad=2, ooff=8, opad=16, rand=1),            # (odd input pitch: scalar loads)
      _conv(3, 4, 6, 4, 24, BF, F32, bias=0, xoff=8, xpad=4, ooff=4, opad=4, rand=1),
      _conv(1, 2, 4, 4, 448, F32, BF, xoff=4, xpad=0, ooff=0, opad=8, tag="lds-edge"),
      _conv(1, 1, 1, 4, 8, F32, F32),
      _conv(5, 64, 66, 4, 320, F32, BF, rand=1, phases=one, tag="past-cap"),            # 217,600 items > 196,608
      _conv(5, 64, 66, 4, 320, F32, F32, rand=1, phases=(), xoff=4, xpad=4, tag="past-cap"),
      _conv(2, 16, 18, 4, 448, BF, F32, xoff=4, xpad=8, ooff=8, opad=0, rand=1, phases=one),
      # conv_small_in_kernel: Cin = 3 and 8, the first Cout beyond the LDS, a pitch the LDS kernel cannot store to
      _conv(1, 9, 7, 3, 12, F32, F32, xoff=1, xpad=2, ooff=3, opad=2, rand=1),
      _conv(2, 4, 5, 8, 4, BF, BF, xoff=2, xpad=1, ooff=1, opad=0, rand=1),
      _conv(1, 2, 3, 4, 456, F32, BF, xoff=4, xpad=0, ooff=8, opad=0, tag="beyond-lds"),
      _conv(1, 3, 6, 4, 16, F32, F32, ooff=0, opad=4, rand=1, tag="ldo20"),
      _conv(1, 130, 130, 4, 512, F32, F32, rand=1, phases=one, tag="past-cap"),         # 2,163,200 items > 2,097,152
      _conv(1, 130, 131, 4, 512, BF, BF, rand=1, phases=(), tag="past-cap"),
      # conv_small_out_kernel: Cout 1..4, chunk counts 6 / 3 / 18 / 8 over the 8 lanes of a pixel, 63 and 60 pixels
      _conv(1, 9, 7, 24, 1, F32, F32, xoff=4, xpad=4, ooff=1, opad=2, rand=1),
      _conv(1, 9, 7, 24, 2, BF, BF, xoff=8, xpad=8, ooff=0, opad=1, rand=1),
      _conv(1, 9, 7, 24, 2, F32, BF, rand=1, bias=0),
      _conv(1, 9, 7, 24, 1, BF, F32, rand=1),
      _conv(2, 5, 6, 72, 3, F32, BF, xoff=8, xpad=8, ooff=2, opad=3, rand=1),
      _conv(1, 4, 4, 64, 4, BF, F32, bias=0, xoff=8, xpad=0, rand=1),
      _conv(1, 384, 384, 128, 3, BF, BF, rand=1, phases=one, tag="past-cap"),           # 147,456 pixels > 131,072
      _conv(2, 64, 64, 320, 4, F32, F32, rand=1, phases=one, xoff=0, xpad=8),
      _conv(1, 32, 33, 320, 4, BF, F32, rand=1, phases=()),
  ]


def conv_items(c):
  """(work items, items per workgroup, workgroup cap, the count the host sizes the grid from) of the kernel that runs
  case `c`.  The LDS kernel's items are groups of 4 pixels of ONE line, B H ceil(W / 4) (Cout / 8), but the host sizes
  its grid from ceil(B H W / 4) (Cout / 8): with W % 4 != 0 the grid is smaller than the items need, and the
  grid-stride loop makes a second pass even below the cap."""
  npix = c.B * c.H * c.W
  if c.kernel == "lds":
    return c.B * c.H * ((c.W + 3) // 4) * (c.Cout // 8), 256, LDS_CAP, ((npix + 3) // 4) * (c.Cout // 8)
  if c.kernel == "in":
    return npix * (c.Cout // 4), 256, IN_CAP, npix * (c.Cout // 4)
  return npix, OUT_PIX_PER_WG, OUT_CAP, npix


def passes(total, per_wg, cap, sized=None):
  """(grid-stride passes, workgroups): the grid is ceil(sized / per_wg) clamped to [1, cap] (common.h grid_for)."""
  grid = max(1, min(cap, -(-(total if sized is None else sized) // per_wg)))
  return -(-total // (grid * per_wg)), grid


def wcode(n):
  """Distinct values with 8-bit mantissas: (128 + n % 128) 2^(n // 128 - 40)."""
  n = torch.as_tensor(n, dtype=I64)
  return (128 + n % 128).to(F64) * torch.pow(torch.tensor(2.0, dtype=F64), (n // 128 - 40).to(F64))


def conv_census(c):
  """x [B,H,W,Cin], w [3,3,Cin,Cout], bias [Cout] or None, expected [B,H,W,Cout]; all float64."""
  s = 2.0 ** -3
  u = c.Cin * s
  x = torch.ones(c.B, c.H, c.W, c.Cin, dtype=F64)
  w = torch.full((3, 3, c.Cin, c.Cout), s, dtype=F64)
  bias = (ints((c.Cout,), 11 + c.Cout, -2, 2).to(F64) * u) if c.bias else None
  y, xx = torch.arange(c.H), torch.arange(c.W)
  ty = torch.minimum(y + 1, torch.tensor(c.H - 1)) - torch.clamp(y - 1, min=0) + 1
  tx = torch.minimum(xx + 1, torch.tensor(c.W - 1)) - torch.clamp(xx - 1, min=0) + 1
  taps = (ty[:, None] * tx[None, :]).to(F64)
  exp = (u * taps)[None, :, :, None].expand(c.B, c.H, c.W, c.Cout).clone()
  if bias is not None:
    exp += bias
  return x, w, bias, exp


def _hot_channel(c, b, y, x):
  return (b + y + 2 * x) % c.Cin


def conv_selection(c, phase):
  """One hot pixel per 3 x 3 window: x, w, None, expected (float64)."""
  ry, rx = phase
  b, y, xx = torch.meshgrid(torch.arange(c.B), torch.arange(c.H), torch.arange(c.W), indexing="ij")
  hot = (y % 3 == ry % 3) & (xx % 3 == rx % 3)
  x = torch.zeros(c.B, c.H, c.W, c.Cin, dtype=F64)
  x[b[hot], y[hot], xx[hot], _hot_channel(c, b, y, xx)[hot]] = 1.0
  n = torch.arange(9 * c.Cin * c.Cout).view(3, 3, c.Cin, c.Cout)
  w = wcode(n)
  exp = torch.zeros(c.B, c.H, c.W, c.Cout, dtype=F64)
  for kh in range(3):
    for kw in range(3):
      iy, ix = y + kh - 1, xx + kw - 1
      ok = (iy >= 0) & (iy < c.H) & (ix >= 0) & (ix < c.W) & (iy % 3 == ry % 3) & (ix % 3 == rx % 3)
      ci = _hot_channel(c, b, iy, ix)
      exp[ok] += w[kh, kw][ci[ok]]
  return x, w, None, exp


def conv_random(c):
  """x in the input type's values, w, bias float32 values; all widened to float64."""
  seed = 1000 + c.B * 7 + c.H * 13 + c.W * 17 + c.Cin * 19 + c.Cout * 23
  x = rnd((c.B, c.H, c.W, c.Cin), seed).to(c.idt).to(F64)
  w = rnd((3, 3, c.Cin, c.Cout), seed + 1, (9 * c.Cin) ** -0.5).to(F64)
  bias = rnd((c.Cout,), seed + 2).to(F64) if c.bias else None
  return x, w, bias


def conv_ref64(x, w, bias, swap=False):
  """3 x 3 'same' convolution in float64, nine shifted products (no call into conv2d)."""
  B, H, W, Cin = x.shape
  xp = F.pad(x, (0, 0, 1, 1, 1, 1))
  out = torch.zeros(B, H, W, w.shape[-1], dtype=F64)
  for kh in range(3):
    for kw in range(3):
      out += xp[:, kh:kh + H, kw:kw + W, :] @ (w[kw, kh] if swap else w[kh, kw])
  return out if bias is None else out + bias


def conv_ceiling(c):
  """test_conv3x3_small / test_conv3x3_small_in_paths: 2e-4 in float32, 2e-2 once the input or the output is bf16."""
  t = 2e-2 if BF in (c.idt, c.odt) else 2e-4
  return t, t


CONV_FAULTS = ("drop_ragged_group", "skip_second_pass", "swap_kh_kw", "pitch_as_contiguous", "one_chunk_pass")


def conv_model(c, xflat, w, bias, fault=None):
  """The output of case `c` as the kernel's decomposition produces it: float64 [B,H,W,Cout], NaN where no work item
  stores.  xflat: the NaN-filled flat input buffer (float64 copy), read at pixel * ldx + xoff + ci."""
  npix = c.B * c.H * c.W
  ldx = c.Cin if fault == "pitch_as_contiguous" else c.xoff + c.Cin + c.xpad
  idx = torch.arange(npix)[:, None] * ldx + c.xoff + torch.arange(c.Cin)[None, :]
  x = xflat[idx].view(c.B, c.H, c.W, c.Cin)
  if fault == "one_chunk_pass" and c.kernel == "out":             # `v += 8` lost: a lane takes its first chunk only
    epc = 8 if c.idt == BF else 4
    x = x.clone()
    x[..., 8 * epc:] = 0
  out = conv_ref64(x, w, bias, swap=fault == "swap_kh_kw")
  total, per_wg, cap, sized = conv_items(c)
  _, grid = passes(total, per_wg, cap, sized)
  b, y, xx, co = torch.meshgrid(torch.arange(c.B), torch.arange(c.H), torch.arange(c.W), torch.arange(c.Cout), indexing="ij")
  pix = (b * c.H + y) * c.W + xx
  if c.kernel == "lds":
    wg4 = (c.W + 3) // 4
    item = ((b * c.H + y) * wg4 + xx // 4) * (c.Cout // 8) + co // 8
    if fault == "drop_ragged_group" and c.W % 4:
      out[xx // 4 == wg4 - 1] = NAN
  elif c.kernel == "in":
    item = pix * (c.Cout // 4) + co // 4
  else:
    item = pix
  if fault == "skip_second_pass":
    out[item // (grid * per_wg) == 1] = NAN
  return out


# ============================================================================================================
# ldm_gemv
# ============================================================================================================
GEMV_ACTS = {"none": (0, 0), "act_out": (0, 1), "act_in": (1, 0)}       # (act_in, act_out) is SiLU: unet.py:614-618


def gemv_cases():
  out = []
  for wdt in (F32, BF):
    for rows in (1, 3, 5, 64):
      for N in (1, 6, 1280):
        for K in (8, 320, 1280, 2048):
          c = NS(rows=rows, N=N, K=K, wdt=wdt, xpad=(0, 8, 3)[(rows + N + K // 8) % 3], ypad=(5, 0, 2)[(rows + N) % 3])
          c.id = f"{DTN[wdt]}-r{rows}-N{N}-K{K}-ldx+{c.xpad}-ldy+{c.ypad}"
          out.append(c)
  return out


def gemv_exact(c):
  s = c.rows * 31 + c.N * 7 + c.K
  return (ints((c.rows, c.K), s, -4, 4).to(F64), ints((c.N, c.K), s + 1, -3, 3).to(F64), ints((c.N,), s + 2, -9, 9).to(F64))


def gemv_random(c):
  s = 5000 + c.rows * 31 + c.N * 7 + c.K
  return (rnd((c.rows, c.K), s).to(F64), rnd((c.N, c.K), s + 1, c.K ** -0.5).to(c.wdt).to(F64), rnd((c.N,), s + 2).to(F64))


def silu64(x):
  return x / (1.0 + torch.exp(-x))


def gemv_ref64(x, w, b, act_in, act_out):
  y = (silu64(x) if act_in else x) @ w.t() + b
  return silu64(y) if act_out else y


def gemv_oracle(x, w, b, act_in, act_out, O):
  x, w, b = x.to(F32), w.to(F32), b.to(F32)
  y = (O.silu(x) if act_in else x) @ w.t() + b
  return (O.silu(y) if act_out else y).to(F64)


GEMV_FAULTS = ("drop_second_row_block", "drop_n_tail", "pitch_as_contiguous", "one_k_pass")


def gemv_model(c, xflat, w, b, fault=None):
  """y [rows, N] float64 (no activation) by the kernel's decomposition: workgroup (bx, by) = columns 4 bx .. + 3, rows
  4 by .. + 3; lane l takes the 16-byte chunks l, l + 64, ... of a weight row.  NaN where nothing is stored."""
  epc = 8 if c.wdt == BF else 4
  ldx = c.K if fault == "pitch_as_contiguous" else c.K + c.xpad
  x = xflat[torch.arange(c.rows)[:, None] * ldx + torch.arange(c.K)[None, :]]
  if fault == "one_k_pass":
    x = x.clone()
    x[:, 64 * epc:] = 0
  y = x @ w.t() + b
  if fault == "drop_second_row_block":
    y[GEMV_RT:2 * GEMV_RT] = NAN
  if fault == "drop_n_tail" and c.N % 4:
    y[:, c.N // 4 * 4:] = NAN
  return y


# ============================================================================================================
# ldm_vq_nearest
# ============================================================================================================
def vq_cases():
  out = []
  for V in (1, 63, 64, 65, 1000, 16384):
    for Cc in (1, 3, 4, 8):
      out.append(NS(V=V, C=Cc, rows=37, id=f"V{V}-C{Cc}-r37"))
  out.append(NS(V=1000, C=4, rows=64, id="V1000-C4-r64"))
  out.append(NS(V=200, C=3, rows=6, id="V200-C3-r6"))
  return out


def vq_plants(V, Cc):
  """Index sets that hold the same codebook row (the nearest of the z rows aimed at it): (a) v and v + 64, one lane;
  (b) 63 (the highest lane) and 64 (lane 0); (c) 2 and V - 1 (even C), V - 1 alone (odd C: the last row is read at
  all); 134 and 7 (a later pass of a higher lane against the first pass of a lower one)."""
  sets = [[5, 69], [63, 64], [2, V - 1] if Cc % 2 == 0 else [V - 1], [134, 7]]
  keep, used = [], set()
  for s in sets:
    if all(0 <= v < V for v in s) and len(set(s)) == len(s) and not (set(s) & used):
      keep.append(s)
      used |= set(s)
  return keep


def vq_data(c):
  """z [rows, C], codebook [V, C] (integers as float64), expected indices [rows] and rows of the codebook."""
  cb = ints((c.V, c.C), 77 + c.V + c.C, -6, 6)
  plants = vq_plants(c.V, c.C)
  special = []
  for j, s in enumerate(plants):
    row = torch.full((c.C,), 9, dtype=I64)
    row[0] = 9 + j                                        # outside [-6, 6]: no other row equals it
    cb[s] = row
    special.append(row)
  z = ints((c.rows, c.C), 78 + c.V + c.C, -6, 6)
  for r in range(min(c.rows, 2 * len(special))):          # the first rows aim at the planted rows (twice over)
    z[r] = special[r % len(special)]
  z, cb = z.to(F64), cb.to(F64)
  idx = first_min((z[:, None, :] - cb[None, :, :]).pow(2).sum(-1))
  return z, cb, idx, cb[idx]


def first_min(d):
  V = d.shape[1]
  return torch.where(d == d.min(1, keepdim=True).values, torch.arange(V)[None, :], torch.tensor(V)).min(1).values


VQ_FAULTS = ("tie_le", "no_index_compare", "drop_row_tail", "drop_last_codebook_row")
VQ_OVERFLOW_FAULTS = ("unseeded",)


def vq_distances_f32(z, cb):
  """[rows, V] float64: the kernel's |z|^2 + |e|^2 - 2 z.e evaluated in float32 (+inf where |z|^2 overflows)."""
  z, cb = z.to(F32), cb.to(F32)
  return ((z * z).sum(1)[:, None] + (cb * cb).sum(1)[None, :] - 2.0 * (z @ cb.t())).to(F64)


def vq_model(c, z, cb, fault=None, d=None):
  """indices [rows] by the kernel's decomposition: lane l < V takes row l whatever its distance, then scans rows
  l + 64, ... keeping the first minimum (a lane beyond V keeps (inf, no row)); a butterfly (xor 32 .. 1) in which a
  lane takes its partner's (distance, index) if it is smaller, or equal with a lower index; lane 0 stores.  -1 where
  no wave stores.  `d`: the distances [rows, V], when they are not the exact integer ones.  Fault `unseeded`: a lane
  whose distances are all +inf holds no row (the kernel before it seeded its lanes)."""
  V = c.V - 1 if fault == "drop_last_codebook_row" and c.V > 1 else c.V
  d = (z[:, None, :] - cb[None, :V, :]).pow(2).sum(-1) if d is None else d[:, :V]                 # [rows, V]
  pad = -(-V // 64) * 64
  dl = torch.full((c.rows, pad), math.inf, dtype=F64)
  dl[:, :V] = d
  dl = dl.view(c.rows, pad // 64, 64)                                   # [rows, pass, lane]
  best = dl.min(1).values                                               # [rows, lane]
  hit = dl == best[:, None, :]
  p = torch.arange(pad // 64)[None, :, None]
  ps = torch.where(hit, p, torch.tensor(-1)).max(1).values if fault == "tie_le" else \
      torch.where(hit, p, torch.tensor(pad)).min(1).values
  bidx = ps * 64 + torch.arange(64)[None, :]
  lane = torch.arange(64)
  empty = torch.isinf(best) if fault == "unseeded" else (lane >= V)[None, :].expand_as(best)
  bidx = torch.where(empty, torch.tensor(0x7fffffff), bidx)
  for o in (32, 16, 8, 4, 2, 1):
    ob, oi = best[:, lane ^ o], bidx[:, lane ^ o]
    take = (ob < best) if fault == "no_index_compare" else (ob < best) | ((ob == best) & (oi < bidx))
    best, bidx = torch.where(take, ob, best), torch.where(take, oi, bidx)
  idx = bidx[:, 0].clone()
  if fault == "drop_row_tail" and c.rows % 4:
    idx[c.rows // 4 * 4:] = -1
  return idx


def vq_overflow_data():
  """Finite z whose squared norm overflows float32 (rows 1, 4, 9): every distance of such a row is +inf.  The other
  rows and the codebook are integers, so their distances are exact in any order.  float32 tensors (z, codebook)."""
  z = ints((10, 4), 90, -6, 6).to(F32)
  z[1] = torch.tensor([2e19, 1.0, -3.0, 0.5])
  z[4] = torch.tensor([-1.5e19, 1.5e19, 0.0, 1.0])
  z[9] = torch.tensor([0.0, 0.0, 0.0, -3e19])
  return z, ints((130, 4), 91, -6, 6).to(F32)


# ============================================================================================================
# ldm_minmax_u8
# ============================================================================================================
def u8_safe():
  """Byte values v with trunc(float32(float32(v / 255) * 255)) == v (minimum 0, range 255)."""
  v = np.arange(256, dtype=np.float32)
  r = (v / np.float32(255.0)) * np.float32(255.0)
  return [int(i) for i in range(256) if int(r[i]) == i]


def minmax_positions(n):
  """{name: element}: first, last, one element of reduction block 63's slice (when n reaches it)."""
  pos = {"first": 0, "last": n - 1}
  b63 = (MINMAX_BLOCKS - 1) * 256 + 17
  if n > b63 and b63 not in (0, n - 1):
    pos["blk63"] = b63
  return pos


def minmax_cases():
  out = []
  for dt in (F32, BF):
    for n in (2, 255, 256, 257, 64 * 256 - 1, 64 * 256 + 1, 3 * 250 * 250):
      names = list(minmax_positions(n))
      pairs = [(a, b) for a in names for b in names if a != b]
      for i in range(len(pairs)):                          # two images per launch: every placement at b = 0 and b = 1
        grp = [pairs[i], pairs[(i + 1) % len(pairs)]]
        c = NS(n=n, dt=dt, places=grp, B=len(grp))
        c.id = f"{DTN[dt]}-n{n}-" + "+".join(f"{a}.{b}" for a, b in grp)
        out.append(c)
  return out


def minmax_data(c):
  """x [B, n] integer image (int64): ONE 0 at the first name's element, ONE 255 at the second's, the rest in
  U8_SAFE \\ {0, 255}.  Expected output: x itself."""
  safe = torch.tensor([v for v in u8_safe() if 0 < v < 255])
  x = safe[ints((c.B, c.n), 300 + c.n, 0, len(safe) - 1)]
  for b, (mn, mx) in enumerate(c.places):
    pos = minmax_positions(c.n)
    x[b, pos[mn]], x[b, pos[mx]] = 0, 255
  return x


MINMAX_FAULTS = ("ignore_last_block", "ignore_first_block")


def minmax_model(c, x, fault=None):
  """uint8-valued [B, n] by the decomposition: block j of 64 reduces elements i with (i // 256) % 64 == j of its image,
  the second kernel folds the 64 (min, max) pairs."""
  blk = (torch.arange(c.n) // 256) % MINMAX_BLOCKS
  use = torch.ones(c.n, dtype=torch.bool)
  if fault == "ignore_last_block":
    use = blk != MINMAX_BLOCKS - 1
  if fault == "ignore_first_block":
    use = blk != 0
  out = torch.empty_like(x)
  for b in range(c.B):
    v = x[b][use].numpy().astype(np.float32)
    mn, mx = (v.min(), v.max()) if v.size else (np.float32(np.inf), np.float32(-np.inf))
    with np.errstate(invalid="ignore", divide="ignore"):
      r = (x[b].numpy().astype(np.float32) - mn) / (mx - mn)
      r = r * np.float32(255.0)
      out[b] = torch.from_numpy(np.nan_to_num(r, nan=0.0, posinf=255.0, neginf=0.0).clip(0, 255).astype(np.uint8).astype(np.int64))
  return out


# ============================================================================================================
# ldm_cast
# ============================================================================================================
def cast_cases():
  out = []
  for idt in (F32, BF):
    for odt in (F32, BF):
      out.append(NS(idt=idt, odt=odt, rows=5, cols=37, xoff=3, xpad=4, ooff=2, opad=1))
      out.append(NS(idt=idt, odt=odt, rows=1030, cols=1031, xoff=0, xpad=1031, ooff=1, opad=6))     # strided halves
  for c in out:
    c.id = f"{DTN[c.idt]}-{DTN[c.odt]}-{c.rows}x{c.cols}"
  return out


CAST_SPECIAL = [0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,     # ties: lower neighbour even / odd, both signs
                0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,     # one float32 ulp beside a tie
                0x80000000, 0x00000000, 0x7f800000, 0xff800000,     # -0, +0, +-inf
                0x7fc00000, 0xffc00000, 0x7f800001, 0x7fa00000,     # NaNs (quiet, negative, signalling, payload)
                0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff,     # the largest finite values: round to inf / stay
                0x00000001, 0x00008000, 0x00018000, 0x007fffff,     # denormals
                0x00800000, 0x3f800000, 0x477fe000, 0x33800000]


def cast_data(c):
  """[rows, cols] of type idt: the special patterns first, then random bit patterns."""
  n = c.rows * c.cols
  bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=torch.Generator().manual_seed(n), dtype=I64)
  sp = torch.tensor(CAST_SPECIAL, dtype=I64)
  sp = torch.where(sp >= 2 ** 31, sp - 2 ** 32, sp)
  bits[:len(sp)] = sp
  if c.idt == F32:
    return bits.to(torch.int32).view(F32).view(c.rows, c.cols)
  return (bits >> 16).to(torch.int16).view(BF).view(c.rows, c.cols)


def bits_of(t):
  return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(got, want):
  """Bit equality where `want` is a number; NaN where it is NaN."""
  nan = torch.isnan(want)
  return bool(torch.isnan(got)[nan].all()) and bool((bits_of(got)[~nan] == bits_of(want)[~nan]).all())


CAST_FAULTS = ("truncate", "pitch_as_contiguous", "skip_second_pass")


def cast_model(c, xflat, fault=None):
  """[rows, cols] of type odt; element i = (r, col) is owned by pass i // (grid * 256).  Dropped elements: NaN."""
  ldx = c.cols if fault == "pitch_as_contiguous" else c.xoff + c.cols + c.xpad
  x = xflat[torch.arange(c.rows)[:, None] * ldx + c.xoff + torch.arange(c.cols)[None, :]]
  if fault == "truncate" and c.idt == F32 and c.odt == BF:
    out = ((x.contiguous().view(torch.int32) >> 16).to(torch.int16)).view(BF)
  else:
    out = x.to(c.odt)
  if fault == "skip_second_pass":
    _, grid = passes(c.rows * c.cols, 256, DEFAULT_CAP)
    i = torch.arange(c.rows * c.cols).view(c.rows, c.cols)
    out = torch.where(i // (grid * 256) == 1, torch.tensor(NAN, dtype=c.odt), out)
  return out


# ============================================================================================================
# ldm_embedding
# ============================================================================================================
def embedding_cases():
  out = []
  for odt in (F32, BF):
    out.append(NS(rows=3, T=7, D=8, vocab=11, odt=odt))
    out.append(NS(rows=16, T=77, D=1280, vocab=500, odt=odt))       # 1,576,960 elements > 4096 x 256
  for c in out:
    c.id = f"{DTN[c.odt]}-{c.rows}x{c.T}x{c.D}-v{c.vocab}"
  return out


def embedding_data(c):
  ids = ints((c.rows, c.T), 400 + c.D, 0, c.vocab - 1)
  flat = ids.view(-1)
  flat[0], flat[3], flat[-1], flat[-2], flat[5] = -1, c.vocab, c.vocab + 5, -7, c.vocab - 1
  flat[c.T] = 0
  return ids, rnd((c.vocab, c.D), 401), rnd((c.T, c.D), 402)


EMB_FAULTS = ("no_clamp", "skip_second_pass", "position_of_row")


def embedding_model(c, ids, tok, pos, fault=None):
  """[rows, T, D] of type odt: the float32 sum tok[clamp(id)] + pos[t], rounded once.  Without the clamp a stray id
  reads outside the table: modelled as NaN."""
  cl = ids.clamp(0, c.vocab - 1)
  e = tok[cl] + (pos[torch.arange(c.rows) % c.T][:, None, :] if fault == "position_of_row" else pos[None])
  if fault == "no_clamp":
    e[cl != ids] = NAN
  if fault == "skip_second_pass":
    _, grid = passes(e.numel(), 256, DEFAULT_CAP)
    i = torch.arange(e.numel()).view(e.shape)
    e[i // (grid * 256) == 1] = NAN
  return e.to(c.odt)


# ============================================================================================================
# ldm_post_quant, ldm_gaussian_sample
# ============================================================================================================
def post_quant_cases():
  out = []
  for Cc in (3, 4, 8):
    for sf in (0.18215, 1.0):
      for bias in (1, 0):
        for odt in (F32, BF):
          out.append(NS(C=Cc, sf=sf, bias=bias, odt=odt, shape=(2, 9, 7)))
  out.append(NS(C=4, sf=1.0, bias=1, odt=F32, shape=(1, 1030, 1031)))            # 1,061,930 pixels > 4096 x 256
  for c in out:
    c.id = f"C{c.C}-sf{c.sf}-{'bias' if c.bias else 'nobias'}-{DTN[c.odt]}-" + "x".join(map(str, c.shape))
  return out


def post_quant_data(c):
  s = 500 + c.C + int(c.sf * 10)
  return rnd(c.shape + (c.C,), s), rnd((c.C, c.C), s + 1), (rnd((c.C,), s + 2) if c.bias else None)


def post_quant_ref64(c, z, k, b):
  sf = float(torch.tensor(c.sf, dtype=F32))                             # the kernel's parameter is a float
  y = (z.to(F64) / sf) @ k.to(F64)
  return y if b is None else y + b.to(F64)


def post_quant_ceiling(c):
  """test_post_quant_vq_embedding_minmax_cast: rtol = atol = 1e-5 (float32).  bf16 out has no older test: one bf16
  rounding (8 significant bits: at most 2^-8 relative) on top of it."""
  return (1e-5, 1e-5) if c.odt == F32 else (2.0 ** -8 + 2e-5, 1e-5)


def gaussian_cases():
  out = [NS(C=4, noise=1, scale=0.18215, shape=(2, 9, 7), wide=1), NS(C=4, noise=0, scale=0.18215, shape=(2, 9, 7), wide=1),
         NS(C=3, noise=1, scale=1.0, shape=(1, 5, 5), wide=1), NS(C=4, noise=1, scale=0.18215, shape=(1, 1030, 257), wide=0)]
  for c in out:
    c.id = f"C{c.C}-{'noise' if c.noise else 'mode'}-s{c.scale}-" + "x".join(map(str, c.shape))
  return out


def gaussian_data(c):
  """moments [.., 2C]: mean ~ N(0, 1); log-variance ~ N(0, 3^2) in the small cases (as test_gaussian_sample_kernel),
  N(-2, 0.5^2) in the large one (where a float32 ceiling of 1e-6 absolute holds against float64 only while
  std * noise stays of order 1)."""
  s = 600 + c.C + c.shape[1]
  mean = rnd(c.shape + (c.C,), s)
  logvar = rnd(c.shape + (c.C,), s + 1, 3.0) if c.wide else rnd(c.shape + (c.C,), s + 1, 0.5) - 2.0
  return torch.cat([mean, logvar], -1).contiguous(), (rnd(c.shape + (c.C,), s + 2) if c.noise else None)


def gaussian_ref64(c, mom, noise):
  mean, logvar = torch.chunk(mom.to(F64), 2, dim=-1)
  scale = float(torch.tensor(c.scale, dtype=F32))
  return (mean if noise is None else mean + torch.exp(0.5 * logvar) * noise.to(F64)) * scale


GAUSSIAN_CEILING = (2e-6, 1e-6)                                             # test_gaussian_sample_kernel


# ============================================================================================================
# ldm_softmax_rows
# ============================================================================================================
SOFTMAX_COLS = (1, 63, 64, 65, 255, 256, 257, 1000, 4096)


def softmax_cases():
  out = []
  for idt in (F32, BF):
    for odt in (F32, BF):
      for cols in SOFTMAX_COLS:
        c = NS(cols=cols, idt=idt, odt=odt, rows=7, scale=(0.3, 1.0)[cols % 2], xpad=9 + cols % 3, opad=5)
        c.id = f"{DTN[idt]}-{DTN[odt]}-c{cols}-s{c.scale}"
        out.append(c)
  return out


def softmax_data(c):
  """x [rows, cols] in the input type's values (float64): random rows, one row with a dominant logit, one with a large
  common offset, one constant."""
  x = rnd((c.rows, c.cols), 700 + c.cols, 4.0)
  x[2, c.cols // 2] += 60.0
  x[3] += 1000.0
  x[4] = -3.0
  return x.to(c.idt).to(F64)


def softmax_ref64(c, x):
  return torch.softmax(x * float(torch.tensor(c.scale, dtype=F32)), dim=-1)


def softmax_ceiling(c):
  t = 2e-2 if c.odt == BF else 2e-4                                      # test_softmax_rows
  return t, t


ROW_SUM_BOUND = 28 * 2.0 ** -24


# ============================================================================================================
# ldm_time_embedding
# ============================================================================================================
TIME_CHANNELS = (320, 321, 2)
TIME_CEILING = (0.0, 2e-4)                                                  # test_time_embedding_gemv: atol 2e-4
FREQ_BOUND = 3e-6


def step_table():
  return torch.arange(1, 1000, 20, dtype=torch.int32)                       # the 50-step table of the sampler tests


def freqs64(channels):
  half = channels // 2
  return torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64) / half)


def time_ref64(t, channels):
  """[len(t), channels]: cos(t f) | sin(t f) | 0 for an odd channel count."""
  a = torch.as_tensor(t).to(F64)[:, None] * freqs64(channels)[None, :]
  e = torch.cat([torch.cos(a), torch.sin(a)], -1)
  return torch.cat([e, torch.zeros(len(t), 1, dtype=F64)], -1) if channels % 2 else e


def freqs_from_sines(emb_t1, channels):
  """(f [half / 2 ..], k): the frequencies of the upper half of k recovered from the row of t = 1: asin(sin f) = f."""
  half = channels // 2
  k = torch.arange((half + 1) // 2, half)
  return torch.asin(emb_t1[half + k].to(F64)), k


TIME_FAULTS = ("no_odd_tail", "index_is_row", "sin_first")


def time_model(t_rows, steps, index, rows, channels, fault=None):
  """[rows, channels] float64 by the kernel's indexing: element i of rows * half is (row i // half, k = i % half);
  t = steps[index] for every row when an index is given; the odd tail column is stored by k = 0."""
  half = channels // 2
  out = torch.full((rows, channels), NAN, dtype=F64)
  if index is not None:
    t = steps[torch.arange(rows) % len(steps)] if fault == "index_is_row" else steps[index].expand(rows)
  else:
    t = t_rows
  a = t.to(F64)[:, None] * freqs64(channels)[None, :]
  c_, s_ = (torch.sin(a), torch.cos(a)) if fault == "sin_first" else (torch.cos(a), torch.sin(a))
  out[:, :half], out[:, half:2 * half] = c_, s_
  if channels % 2 and fault != "no_odd_tail":
    out[:, -1] = 0.0
  return out


# ============================================================================================================
# gates: twice the largest figure of the first run, rounded up to one significant digit (module docstring)
# ============================================================================================================
GATES = {
    ('conv_in', 'bf16', 'bf16'): 2.0,
    ('conv_in', 'f32', 'f32'): 4.0,
    ('conv_lds', 'bf16', 'bf16'): 1.0,
    ('conv_lds', 'bf16', 'f32'): 5.0,
    ('conv_lds', 'f32', 'bf16'): 2.0,
    ('conv_lds', 'f32', 'f32'): 4.0,
    ('conv_out', 'bf16', 'bf16'): 2.0,
    ('conv_out', 'bf16', 'f32'): 3.0,
    ('conv_out', 'f32', 'bf16'): 2.0,
    ('conv_out', 'f32', 'f32'): 2.0,
    ('gaussian_sample', 'f32'): 2.0,
    ('gemv', 'bf16'): 3.0,
    ('gemv', 'f32'): 4.0,
    ('post_quant', 'bf16'): 2.0,
    ('post_quant', 'f32'): 3.0,
    ('softmax_rows', 'bf16', 'bf16'): 1.0,
    ('softmax_rows', 'bf16', 'f32'): 3.0,
    ('softmax_rows', 'f32', 'bf16'): 0.9,
    ('softmax_rows', 'f32', 'f32'): 4.0,
    ('time_embedding', 'f32'): 5.0,
}


def gate(entry, *types):
  return GATES[(entry,) + tuple(DTN.get(t, t) for t in types)]


def one_digit_up(v):
  """v rounded up to one significant digit."""
  if v <= 0:
    return 0.0
  e = math.floor(math.log10(v))
  m = math.ceil(v / 10 ** e - 1e-9)
  return float(f"{m * 10.0 ** e:.1g}")
