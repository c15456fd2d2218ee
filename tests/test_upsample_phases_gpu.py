"""The upsample convolution as four 2x2 phase convolutions (ops.conv3x3_up2, ldm_gemm's upsample = 2) against the
nine-tap oracle conv2d(upsample_nearest2x(x), k) and against the existing conv3x3(upsample=True) launch.

Tiles: the ones the phase form is instantiated for (bf16: 2, 9, 11; f32: 1, 2) and 0 (the cost model's pick).

Exact case: x in {-1, 0, 1}, kernel entries in {-1, 1} on one input channel in eight (the channel set moves with the
output channel and the tap, so every input channel and every tap is multiplied somewhere) and zero elsewhere, integer
bias in [-8, 8].  A phase weight is a sum of at most four kernel entries (|w| <= 4) and an output is a sum of at most
9 Cin / 8 <= 144 terms of magnitude 1 plus the bias: |out| <= 152 < 256, an integer that bf16 (8 significant bits) and
float32 hold exactly, as they hold every partial sum.  The gate is torch.equal: a wrong tap, phase, border or output row
is a whole-number error.

Random case: tolerances are TOL of tests/test_ops_gpu.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ldm_oracle as O  # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TOL = {F32: dict(rtol=2e-4, atol=2e-4), BF: dict(rtol=2e-2, atol=2e-2)}      # tests/test_ops_gpu.py
TILES = {BF: (0, 2, 9, 11), F32: (0, 1, 2)}
KTILE = {BF: 64, F32: 32}                                                      # elements per 128-byte K-tile


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


def layout():
  from ldm_tf2_amd import layout as _l
  return _l


def exact_problem(B, H, W, Cin, Cout, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randint(-1, 2, (B, H, W, Cin), generator=g).to(F64)
  sign = torch.randint(0, 2, (3, 3, Cin, Cout), generator=g).to(F64) * 2 - 1
  kh, kw, ci, co = torch.meshgrid(torch.arange(3), torch.arange(3), torch.arange(Cin), torch.arange(Cout), indexing="ij")
  k = sign * ((ci + co + 3 * kh + kw) % 8 == 0)
  bias = torch.randint(-8, 9, (Cout,), generator=g).to(F64)
  ref = O.conv2d(O.upsample_nearest2x(x), k, bias)
  assert ref.abs().max().item() <= 152
  return x, k, bias, ref


def random_problem(B, H, W, Cin, Cout, dtype, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(B, H, W, Cin, generator=g).to(dtype)                        # the activations as the device holds them
  k = torch.randn(3, 3, Cin, Cout, generator=g) * (9 * Cin) ** -0.5            # unrounded float32 master kernel
  bias = torch.randn(Cout, generator=g)
  ref = O.conv2d(O.upsample_nearest2x(x.to(F64)), k.to(F64), bias.to(F64))
  return x, k, bias, ref


_CACHE = {}


def problem(kind, *args):
  key = (kind,) + args
  if key not in _CACHE:
    _CACHE[key] = (exact_problem if kind == "exact" else random_problem)(*args)
  return _CACHE[key]


def close(got, ref, dtype, what):
  got, ref = got.detach().to(F64).cpu(), ref.to(F64).cpu()
  err = (got - ref).abs().max().item()
  print(f"{what}: max err {err:.3e}")
  assert torch.allclose(got, ref, **TOL[dtype]), f"{what}: max err {err}"


def shapes(dtype):
  kt = KTILE[dtype]
  # B, H, W, Cin, Cout: M / N tails, an image boundary inside a tile, a non-square image, one and two channel chunks;
  # 270 rows per phase: one full 256-row tile and a partial second one
  return [(2, 3, 5, kt, 72), (2, 3, 5, 2 * kt, 72), (3, 10, 9, kt, 72)]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_exact(dev, dtype, case):
  o, L = ops(), layout()
  B, H, W, Cin, Cout = shapes(dtype)[case]
  x, k, bias, ref = problem("exact", B, H, W, Cin, Cout, 7 + case)
  w4 = L.upsample_phase_kernel(k.numpy(), dtype, dev)
  assert torch.equal(w4.cpu().to(F64), L.upsample_phase_kernel(k.numpy(), F64, "cpu"))     # the sums are exact
  xd, bd = x.to(dtype).to(dev), bias.to(F32).to(dev)
  for tile in TILES[dtype]:
    out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=dtype, device=dev)
    o.conv3x3_up2(xd, w4, out, bias=bd, tile=tile)
    got = out.cpu().to(F64)
    bad = (got != ref).sum().item()
    assert torch.equal(got, ref), f"tile {tile}: {bad} of {ref.numel()} outputs differ"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("split", [2, 4])
def test_exact_split_k(dev, dtype, split):
  """4x4 -> 8x8, Cin = Cout = 128, forced split-K: the slabs carry output rows, the reduce stores them."""
  o, L = ops(), layout()
  B, H, W, Cin, Cout = 2, 4, 4, 128, 128
  x, k, bias, ref = problem("exact", B, H, W, Cin, Cout, 21)
  w4 = L.upsample_phase_kernel(k.numpy(), dtype, dev)
  xd, bd = x.to(dtype).to(dev), bias.to(F32).to(dev)
  for tile in TILES[dtype]:
    out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=dtype, device=dev)
    o.conv3x3_up2(xd, w4, out, bias=bd, tile=tile, split_k=split)
    assert torch.equal(out.cpu().to(F64), ref), f"tile {tile} split {split}"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_random(dev, dtype, case):
  """Against the float64 oracle on the UNROUNDED kernel, and against the nine-tap launch on its own rounded weights."""
  o, L = ops(), layout()
  B, H, W, Cin, Cout = (shapes(dtype) + [(2, 4, 4, 128, 128)])[case]
  x, k, bias, ref = problem("random", B, H, W, Cin, Cout, dtype, 31 + case)
  w4 = L.upsample_phase_kernel(k.numpy(), dtype, dev)
  w9 = L.conv_kernel(k.numpy(), dtype, dev)
  xd, bd = x.to(dev), bias.to(dev)
  old = torch.empty(B, 2 * H, 2 * W, Cout, dtype=dtype, device=dev)
  o.conv3x3(xd, w9, old, bias=bd, upsample=True)
  for tile in TILES[dtype]:
    for split in ((0, 2, 4) if case == 3 else (0,)):
      out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=dtype, device=dev)
      o.conv3x3_up2(xd, w4, out, bias=bd, tile=tile, split_k=split)
      close(out, ref, dtype, f"tile {tile} split {split} vs oracle")
      close(out, old, dtype, f"tile {tile} split {split} vs conv3x3(upsample=True)")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("wide", [128, 100])
@pytest.mark.parametrize("with_bias", [False, True])
def test_channel_sliced_destination(dev, dtype, wide, with_bias):
  """The destination is the first Cout channels of a wider, pre-filled buffer (the U-Net's concat buffers); pixel
  pitch 128 takes the 16-byte epilogue, 100 the element-wise one.  The other channels keep their bits."""
  o, L = ops(), layout()
  B, H, W, Cin, Cout = 2, 3, 5, 2 * KTILE[dtype], 72
  x, k, bias, ref = problem("exact", B, H, W, Cin, Cout, 8)
  if not with_bias:
    ref = ref - bias
  w4 = L.upsample_phase_kernel(k.numpy(), dtype, dev)
  xd = x.to(dtype).to(dev)
  bd = bias.to(F32).to(dev) if with_bias else None
  g = torch.Generator().manual_seed(3)
  fill = torch.randn(B, 2 * H, 2 * W, wide, generator=g).to(dtype).to(dev)
  for tile in TILES[dtype]:
    for split in (0, 2):
      buf = fill.clone()
      o.conv3x3_up2(xd, w4, buf[..., :Cout], bias=bd, tile=tile, split_k=split)
      assert torch.equal(buf[..., :Cout].cpu().to(F64), ref), f"tile {tile} split {split}"
      assert torch.equal(buf[..., Cout:], fill[..., Cout:]), f"tile {tile} split {split}: neighbouring channels"


def test_host_validation(dev):
  o = ops()
  from ldm_tf2_amd._lib import LdmHipError
  x = torch.zeros(1, 4, 4, 64, dtype=BF, device=dev)
  w4 = torch.zeros(4, 8, 256, dtype=BF, device=dev)
  out = torch.zeros(1, 8, 8, 8, dtype=BF, device=dev)
  p = o._up2_params(x, w4, out, None, 0, 0)
  p.K = 9 * 64
  with pytest.raises(LdmHipError, match="needs K == 4\\*Cin"):
    o._gemm(p, x.device)
  p = o._up2_params(x, w4, out, None, 0, 0)
  p.stride = 2
  with pytest.raises(LdmHipError, match="needs stride 1"):
    o._gemm(p, x.device)
  with pytest.raises(LdmHipError, match="has no phase form"):
    o.conv3x3_up2(x, w4, out, tile=3)
  torch.cuda.synchronize()
