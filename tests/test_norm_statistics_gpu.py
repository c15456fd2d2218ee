"""Every GroupNorm / LayerNorm code path against float64, on the inputs where norm statistics go wrong.

The kernels take their mean and variance in eight different ways (fused two-pass GroupNorm, the split-K
GroupNorm, the two-launch partial-sums + apply pair, ldm_layernorm, the GEMM's LayerNorm second output and
the row-panel kernels' LayerNorm folds).  A one-pass variance (E[x^2] - mean^2) cancels catastrophically
once a group's mean is large compared with its spread, so the input families here carry offsets of up to
10^4 sigma (float32; bfloat16 values cannot carry more than 2^8 sigma), offsets that differ between the
groups of one sample, outlier channels, nearly flat and exactly constant groups.

Inputs are built on the CPU from seeded generators and rounded to the kernel dtype; the reference is the
oracle's group_norm / layer_norm (+ silu) in float64 on those rounded values.  Where a kernel normalises a
product it has rounded to the output dtype (the split-K GroupNorm, the GEMM's LayerNorm output), the
reference is the float64 norm of the product as stored; the stored product is checked on its own against
the float64 convolution / dense.  Every case also asserts which kernel it reaches and that two runs give
identical bits.

Gates, with k the case's offset / sigma (0 for `centred` and `outliers`):
  float32:  relative L2 <= 2e-6 + 1e-6 k;  max |err| <= 2e-4 max|gamma| for k <= 256
  bfloat16: every element within 1 bf16 ulp (taken at max(|ref|, 2^-6)); relative L2 <= 3e-3
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from ldm_tf2_amd import layout as L  # noqa: E402
from norm_check import bf16_ulp, check  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

F32, BF = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF: "bf16"}
GROUPS = 32
GN_EPS = 1e-6           # the autoencoder's: a mean error is multiplied by up to 1 / sqrt(eps)
LN_EPS = 1e-5

F32_FAMILIES = ["centred", "shift32", "shift256", "shift1000", "shift10000", "mixed", "outliers", "near_flat",
                "constant"]
BF16_FAMILIES = ["centred", "shift32", "shift256", "mixed", "outliers", "constant"]
FAMILIES = {F32: F32_FAMILIES, BF: BF16_FAMILIES}
CONST = 0.75            # every partial sum of 0.75 at these sizes is exact in float32


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


def lib():
  from ldm_tf2_amd._lib import lib as _lib
  return _lib


def offset_over_sigma(family, dtype):
  if family.startswith("shift"):
    return float(family[5:])
  if family == "mixed":
    return 1000.0 if dtype == F32 else 128.0
  if family == "near_flat":
    return 1000.0
  return 0.0


def unit_offsets(family, n, dtype, g):
  """Per-unit (sample x group, or row) offset and noise scale of a family."""
  sign = torch.sign(torch.randn(n, generator=g, dtype=torch.float64))
  sign[sign == 0] = 1.0
  k = offset_over_sigma(family, dtype)
  if family.startswith("shift"):
    return k * sign, 1.0
  if family == "mixed":
    off = torch.zeros(n, dtype=torch.float64)
    half = torch.randperm(n, generator=g)[:n // 2]
    off[half] = k * sign[half]
    return off, 1.0
  if family == "near_flat":
    return torch.ones(n, dtype=torch.float64), 1e-3
  return torch.zeros(n, dtype=torch.float64), 1.0


def outlier_channels(C, g):
  idx = torch.randperm(C, generator=g)[:max(1, C // 100)]
  return idx, 60.0 * torch.sign(torch.randn(len(idx), generator=g, dtype=torch.float64))


def check_constant(label, got, want, dtype):
  """A group / row of exactly constant input has variance 0: its output is beta (or silu(beta)) up to the
  output dtype's rounding."""
  got = got.detach().cpu().double()
  want = want.double()
  assert torch.isfinite(got).all(), f"{label}: non-finite output on the constant group"
  scale = want.abs().clamp_min(2.0 ** -6)
  tol = bf16_ulp(want) if dtype == BF else scale * 2.0 ** -20
  worst = ((got - want).abs() / tol).max().item()
  assert worst <= 1.0, f"{label}: constant group off beta by {worst:.2f} x the dtype's rounding"


def norm_params(C, seed):
  g = torch.Generator().manual_seed(seed)
  gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
  beta = 0.2 * torch.randn(C, generator=g)
  return gamma, beta


# ---- GroupNorm inputs ------------------------------------------------------------------------------------------
def gn_input(shape, dtype, family, seed):
  """x [B, H, W, C] of `family`, rounded to dtype (CPU)."""
  B, H, W, C = shape
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
  off, s = unit_offsets(family, B * GROUPS, dtype, g)
  x = x * s + off.view(B, 1, 1, GROUPS).repeat_interleave(C // GROUPS, dim=3)
  if family == "outliers":
    idx, val = outlier_channels(C, g)
    x[..., idx] += val
  if family == "constant":
    x[0, :, :, :C // GROUPS] = CONST              # sample 0, group 0
  return x.to(dtype)


_REF = {}


def gn_reference(shape, dtype, family, seed):
  """(x rounded to dtype, float64 GroupNorm without activation, gamma, beta); one entry kept: cases that share
  an input are adjacent."""
  key = (shape, dtype, family, seed)
  if key not in _REF:
    _REF.clear()
    x = gn_input(shape, dtype, family, seed)
    gamma, beta = norm_params(shape[-1], seed + 1)
    y = O.group_norm(x.double(), gamma.double(), beta.double(), groups=GROUPS, eps=GN_EPS)
    _REF[key] = (x, y, gamma, beta)
  return _REF[key]


def shape_id(shape):
  return "x".join(str(s) for s in shape)


FUSED_SHAPES = [(2, 32, 32, 320), (9, 16, 16, 640), (5, 4, 4, 1280), (2, 5, 7, 320),
                (2, 64, 64, 512)]            # 64x64 at 512 channels stays on the fused kernel (gn_fused_plan)


def _gn_cases():
  cases = []
  for dtype in (F32, BF):
    fam = FAMILIES[dtype]
    for shape in FUSED_SHAPES:
      for i, f in enumerate(fam):
        cases.append(("gn_fused", dtype, f, shape, i % 2 == 0))
    # two launches.  The decoder's 256x256x128: every family, both activations
    for f in fam:
      for silu in (True, False):
        cases.append(("gn_two_launch", dtype, f, (1, 256, 256, 128), silu))
    big = "shift1000" if dtype == F32 else "shift256"
    sub = ["centred", big, "mixed", "near_flat" if dtype == F32 else "outliers"]
    for shape in [(1, 256, 256, 256), (1, 128, 128, 512)]:    # decoder 256^2, encoder 128^2
      for f in sub:
        cases.append(("gn_two_launch", dtype, f, shape, True))
    cases.append(("gn_two_launch", dtype, big, (1, 512, 512, 128), True))  # latent 64 decode: one 512^2 case
    u64 = ["centred", big, "mixed", "constant"] + (["shift10000"] if dtype == F32 else [])
    for i, f in enumerate(u64):                               # the U-Net's 64x64 level at latent 64
      cases.append(("gn_two_launch", dtype, f, (2, 64, 64, 320), i % 2 == 1))
    for i, f in enumerate(fam):                               # odd HW, one chunk
      cases.append(("gn_two_launch", dtype, f, (3, 5, 7, 320), i % 2 == 0))
    for f in ["centred", big, "mixed"]:                       # B = 16: fewer, shorter chunks
      cases.append(("gn_two_launch", dtype, f, (16, 64, 64, 128), True))
  return cases


GN_CASES = _gn_cases()


def _gn_id(c):
  path, dtype, f, shape, silu = c
  return f"{path}-{DTN[dtype]}-{f}-{shape_id(shape)}" + ("-silu" if silu else "")


@pytest.mark.parametrize("case", GN_CASES, ids=[_gn_id(c) for c in GN_CASES])
def test_groupnorm_statistics(dev, case):
  """Fused and two-launch GroupNorm (+SiLU) on channel-sliced input and output against float64."""
  path, dtype, family, shape, silu = case
  o = ops()
  B, H, W, C = shape
  HW = H * W
  fused_ok = lib().ldm_groupnorm_fused_supported(B, HW, C, GROUPS, o.code(dtype))
  x, y64, gamma, beta = gn_reference(shape, dtype, family, 7)
  if path == "gn_fused":
    assert fused_ok == 1, f"{shape} {dtype} no longer takes the fused GroupNorm"
    fused = True
  else:
    # decoder / encoder shapes reach the two-launch pair by default; the others are forced onto it
    fused = None if fused_ok == 0 else False
    if min(H, W) >= 128 or shape == (2, 64, 64, 320):
      assert fused_ok == 0, f"{shape} {dtype} now takes the fused GroupNorm"
  ref = O.silu(y64) if silu else y64
  wide = torch.zeros(B, H, W, C + 64, dtype=dtype, device=dev)
  xs = wide[..., 64:]
  xs.copy_(x)
  gd, bd = gamma.to(dev), beta.to(dev)
  outs = []
  for _ in range(2):
    ow = torch.full((B, H, W, C + 32), float("nan"), dtype=dtype, device=dev)
    o.groupnorm(xs, gd, bd, ow[..., 32:], GN_EPS, silu=silu, groups=GROUPS, fused=fused)
    outs.append(ow)
  torch.cuda.synchronize()
  assert torch.isnan(outs[0][..., :32].float()).all(), "wrote outside the output slice"
  got = outs[0][..., 32:]
  assert torch.equal(got, outs[1][..., 32:]), "two runs differ: the reductions are not fixed-order"
  k = offset_over_sigma(family, dtype)
  check(_gn_id(case), got, ref, dtype, k, gamma.abs().max().item())
  if family == "constant":
    cg = C // GROUPS
    want = beta[:cg].double().expand(H, W, cg)
    check_constant(_gn_id(case), got[0, :, :, :cg], O.silu(want) if silu else want, dtype)


# ---- split-K convolution + GroupNorm (ldm_groupnorm_splitk) ----------------------------------------------------
SK_SHAPES = [(4, 8, 128, 320, 3), (2, 16, 64, 640, 2), (3, 4, 256, 1280, 4)]   # B, H, Cin, Cout, split


def _sk_cases():
  cases = []
  for dtype in (F32, BF):
    fam = ["centred", "shift32", "shift256", "mixed"] + (["shift1000", "shift10000"] if dtype == F32 else [])
    for sh in SK_SHAPES:
      for i, f in enumerate(fam):
        cases.append((dtype, f, sh, i % 2 == 0))
  return cases


SK_CASES = _sk_cases()


def _sk_id(c):
  dtype, f, (B, H, Cin, Cout, split), silu = c
  return f"gn_splitk-{DTN[dtype]}-{f}-{B}x{H}x{H}x{Cin}to{Cout}-split{split}" + ("-silu" if silu else "")


@pytest.mark.parametrize("case", SK_CASES, ids=[_sk_id(c) for c in SK_CASES])
def test_splitk_groupnorm_statistics(dev, case):
  """conv3x3 split-K with its reduce deferred into the GroupNorm; the per-group offset rides in the bias."""
  dtype, family, (B, H, Cin, Cout, split), silu = case
  o = ops()
  assert lib().ldm_groupnorm_splitk_supported(B, H * H, Cout, GROUPS, o.code(dtype)) == 1
  g = torch.Generator().manual_seed(40)
  x = torch.randn(B, H, H, Cin, generator=g).to(dtype)
  w_hwio = torch.randn(3, 3, Cin, Cout, generator=g) * (9 * Cin) ** -0.5
  off, _ = unit_offsets(family, GROUPS, dtype, g)
  bias = (0.1 * torch.randn(Cout, generator=g, dtype=torch.float64) +
          off.repeat_interleave(Cout // GROUPS)).float()
  gamma, beta = norm_params(Cout, 41)
  wt = L.conv_kernel(w_hwio.numpy(), dtype, dev)
  xd = x.to(dev)
  prods, outs = [], []
  for _ in range(2):
    y = torch.full((B, H, H, Cout), float("nan"), dtype=dtype, device=dev)
    pend = o.conv3x3(xd, wt, y, bias=bias.to(dev), split_k=split, defer_reduce=True)
    assert isinstance(pend, o.PendingReduce) and not pend.done
    gn = torch.full_like(y, float("nan"))
    o.groupnorm(y, gamma.to(dev), beta.to(dev), gn, GN_EPS, silu=silu, groups=GROUPS, pending=pend, store_x=True)
    assert pend.done
    prods.append(y)
    outs.append(gn)
  torch.cuda.synchronize()
  assert torch.equal(prods[0], prods[1]) and torch.equal(outs[0], outs[1])
  # the stored product against the float64 convolution
  want = O.conv2d(x.double(), w_hwio.double(), bias.double())
  yc = prods[0].cpu().double()
  rp = ((yc - want).norm() / want.norm()).item()
  assert rp < (2e-5 if dtype == F32 else 6e-3), f"stored product rel-L2 {rp:.3e}"
  # the normalisation of the product as stored
  ref = O.group_norm(yc, gamma.double(), beta.double(), groups=GROUPS, eps=GN_EPS)
  if silu:
    ref = O.silu(ref)
  check(_sk_id(case), outs[0], ref, dtype, offset_over_sigma(family, dtype), gamma.abs().max().item())


# ---- row inputs for the LayerNorms -----------------------------------------------------------------------------
def row_input(M, C, dtype, family, g, noise_scale=1.0):
  """[M, C] float64 of `family` (not rounded); `constant` makes row 0 exactly CONST."""
  x = torch.randn(M, C, generator=g, dtype=torch.float64)
  off, s = unit_offsets(family, M, dtype, g)
  x = x * (s * noise_scale) + off[:, None]
  if family == "outliers":
    idx, val = outlier_channels(C, g)
    x[:, idx] += val
  if family == "constant":
    x[0] = CONST
  return x


def _row_cases(widths):
  return [(dtype, f, C) for dtype in (F32, BF) for C in widths for f in FAMILIES[dtype]]


LN_CASES = _row_cases([64, 320, 768, 1280])


@pytest.mark.parametrize("case", LN_CASES, ids=[f"layernorm-{DTN[d]}-{f}-300x{C}" for d, f, C in LN_CASES])
def test_layernorm_statistics(dev, case):
  dtype, family, C = case
  o = ops()
  M = 300
  g = torch.Generator().manual_seed(60 + C)
  x = row_input(M, C, dtype, family, g).to(dtype)
  gamma, beta = norm_params(C, 61)
  xd = x.to(dev)
  outs = []
  for _ in range(2):
    out = torch.full((M, C), float("nan"), dtype=dtype, device=dev)
    o.layernorm(xd, gamma.to(dev), beta.to(dev), out, LN_EPS)
    outs.append(out)
  torch.cuda.synchronize()
  assert torch.equal(outs[0], outs[1])
  ref = O.layer_norm(x.double(), gamma.double(), beta.double(), eps=LN_EPS)
  label = f"layernorm-{DTN[dtype]}-{family}-{M}x{C}"
  check(label, outs[0], ref, dtype, offset_over_sigma(family, dtype), gamma.abs().max().item())
  if family == "constant":
    check_constant(label, outs[0][0], beta.double(), dtype)


# ---- the GEMM's LayerNorm second output ------------------------------------------------------------------------
GL_CASES = _row_cases([320])


@pytest.mark.parametrize("case", GL_CASES, ids=[f"gemm_ln_out-{DTN[d]}-{f}-300x{C}" for d, f, C in GL_CASES])
def test_gemm_layernorm_output_statistics(dev, case):
  """linear(..., ln=...): the row offset enters through the residual; the LayerNorm is of `out` as stored."""
  dtype, family, N = case
  o = ops()
  M, K = 300, 320
  assert o.linear_ln_supported(N, dtype)
  g = torch.Generator().manual_seed(70)
  s = 1e-3 if family == "near_flat" else 1.0              # the product's spread follows the family's noise
  x = (torch.randn(M, K, generator=g) * s).to(dtype)
  if family == "constant":
    x[0] = 0
  w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
  res = row_input(M, N, dtype, family, g, noise_scale=0.5).to(dtype)
  bias = None if family == "constant" else 0.1 * s * torch.randn(N, generator=g)
  gamma, beta = norm_params(N, 71)
  xd, wd, rd = x.to(dev), w.to(dev), res.to(dev)
  bd = None if bias is None else bias.to(dev)
  outs, lns = [], []
  for _ in range(2):
    out = torch.full((M, N), float("nan"), dtype=dtype, device=dev)
    ln = torch.full((M, N), float("nan"), dtype=dtype, device=dev)
    o.linear(xd, wd, out, bias=bd, residual=rd, ln=(gamma.to(dev), beta.to(dev), ln, LN_EPS))
    outs.append(out)
    lns.append(ln)
  torch.cuda.synchronize()
  assert torch.equal(outs[0], outs[1]) and torch.equal(lns[0], lns[1])
  # the stored product against the float64 dense (test_ops_gpu's tolerances)
  want = x.double() @ w.double().t() + res.double() + (0 if bias is None else bias.double())
  tol = dict(rtol=2e-4, atol=2e-4) if dtype == F32 else dict(rtol=2e-2, atol=2e-2)
  oc = outs[0].cpu().double()
  assert torch.allclose(oc, want, **tol), f"stored product max err {(oc - want).abs().max().item():.3e}"
  ref = O.layer_norm(oc, gamma.double(), beta.double(), eps=LN_EPS)
  label = f"gemm_ln_out-{DTN[dtype]}-{family}-{M}x{N}"
  check(label, lns[0], ref, dtype, offset_over_sigma(family, dtype), gamma.abs().max().item())
  if family == "constant":
    check_constant(label, lns[0][0], beta.double(), dtype)


# ---- LayerNorm folds of the row-panel kernels (bf16) -----------------------------------------------------------
C_, H_, S_, SP_ = 320, 8, 40, 48
K0_ = H_ * SP_


def fold_rows(M, family, g):
  """The round-4 LN-fold test's rows: a common offset of 32 / 64 sigma with a sign per row, or 1 % of the
  channels at 60 sigma."""
  x = torch.randn(M, C_, generator=g)
  if family == "outliers":
    idx = torch.randperm(C_, generator=g)[:max(1, C_ // 100)]
    x[:, idx] += 60.0 * torch.sign(torch.randn(len(idx), generator=g))
  else:
    x = x + float(family[5:]) * torch.sign(torch.randn(M, 1, generator=g))
  return x.to(BF)


def ffn_weights(g):
  gamma, beta = 1.0 + 0.3 * torch.randn(C_, generator=g), 0.2 * torch.randn(C_, generator=g)
  k1 = torch.randn(C_, 8 * C_, generator=g) * C_ ** -0.5
  b1 = torch.randn(8 * C_, generator=g)
  k2 = torch.randn(4 * C_, C_, generator=g) * (4 * C_) ** -0.5
  b2 = torch.randn(C_, generator=g)
  return gamma, beta, k1, b1, k2, b2


def ffn64(h, gamma, beta, k1, b1, k2, b2):
  """float64 h + Dense(a * gelu(g)), (a | g) = Dense(LayerNorm(h))."""
  d = lambda t: t.double()
  y = O.layer_norm(h, d(gamma), d(beta), eps=LN_EPS) @ d(k1) + d(b1)
  a, gt = y[:, :4 * C_], y[:, 4 * C_:]
  return h + (a * 0.5 * gt * (1.0 + torch.erf(gt / math.sqrt(2.0)))) @ d(k2) + d(b2)


class FfnDev:
  """Device operands of the feed-forward: folded for the row-panel kernels, plain for the unfused chain."""

  def __init__(self, dev, gamma, beta, k1, b1, k2, b2):
    gw, gb = L.geglu_kernel(k1.numpy(), b1.numpy(), torch.float32, "cpu")
    self.w1, cs, bb = L.ln_fold(gw, gamma.numpy(), beta.numpy(), gb.numpy(), BF, dev)
    self.aux = L.ffn_aux(cs, bb)
    self.gw, self.gb = gw.to(BF).to(dev), gb.to(dev)
    self.w2 = L.dense_kernel(k2.numpy(), BF, dev)
    self.b2 = b2.to(dev)
    self.gamma, self.beta = gamma.to(dev), beta.to(dev)

  def unfused(self, o, hd):
    """ldm_layernorm -> bf16 rows -> GEGLU GEMM -> FF-out GEMM + residual."""
    M = hd.shape[0]
    ln = torch.empty(M, C_, dtype=BF, device=hd.device)
    o.layernorm(hd, self.gamma, self.beta, ln, LN_EPS)
    ff = torch.empty(M, 4 * C_, dtype=BF, device=hd.device)
    o.linear(ln, self.gw, ff, bias=self.gb, act=o.ACT_GEGLU)
    y = torch.empty(M, C_, dtype=BF, device=hd.device)
    o.linear(ff, self.w2, y, bias=self.b2, residual=hd)
    return y


def fold_gate(label, out, out_unfused, ref):
  rel = lambda a: ((a.detach().cpu().double() - ref).norm() / ref.norm()).item()
  r, ru = rel(out), rel(out_unfused)
  print(f"{label}: rel-L2 {r:.3e} (unfused chain {ru:.3e})")
  assert torch.isfinite(out.float()).all()
  assert r <= max(4e-3, 1.5 * ru), f"{label}: rel {r:.3e} > max(4e-3, 1.5 x {ru:.3e})"


FOLD_FAMILIES = ["shift32", "shift64", "outliers"]


@pytest.mark.parametrize("family", FOLD_FAMILIES)
def test_ffn_geglu_layernorm_fold(dev, family):
  o = ops()
  M = 1000
  g = torch.Generator().manual_seed(80)
  x = fold_rows(M, family, g)
  wts = ffn_weights(g)
  ref = ffn64(x.double(), *wts)
  F = FfnDev(dev, *wts)
  xd = x.to(dev)
  assert o.ffn_geglu_supported(xd)
  outs = []
  for _ in range(2):
    out = torch.full((M, C_), float("nan"), dtype=BF, device=dev)
    o.ffn_geglu(xd, F.w1, F.aux, F.w2, F.b2, out, LN_EPS)
    outs.append(out)
  out_u = F.unfused(o, xd)
  torch.cuda.synchronize()
  assert torch.equal(outs[0], outs[1])
  fold_gate(f"ffn_geglu-bf16-{family}-{M}x{C_}", outs[0], out_u, ref)


def tail_operands(g, M):
  ko = torch.zeros(K0_, C_)                    # rows of the padded head dims are zero (layout.merge_kernel)
  ko.view(H_, SP_, C_)[:, :S_] = torch.randn(H_, S_, C_, generator=g) * (H_ * S_) ** -0.5
  bo, bp = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
  kp = torch.randn(C_, C_, generator=g) * C_ ** -0.5
  r1 = torch.randn(M, C_, generator=g).to(BF)
  return ko, bo, kp, bp, r1


def tail64(att, r0, ko, bo, wts, kp, bp, r1):
  """float64 r1 + bp + Wp (ffn(h)), h = r0 + bo + Wo att."""
  h = r0.double() + att.double() @ ko.double() + bo.double()
  return r1.double() + ffn64(h, *wts) @ kp.double() + bp.double()


def tail_unfused(o, att, wo, bo, r0, F, wp, bp, r1):
  M = r0.shape[0]
  hd = torch.empty(M, C_, dtype=BF, device=r0.device)
  o.linear(att.reshape(M, -1), wo, hd, bias=bo, residual=r0)
  y = F.unfused(o, hd)
  out = torch.empty(M, C_, dtype=BF, device=r0.device)
  o.linear(y, wp, out, bias=bp, residual=r1)
  return out


@pytest.mark.parametrize("family", FOLD_FAMILIES)
def test_st_tail_layernorm_fold(dev, family):
  """The LayerNorm inside ldm_st_tail normalises h = r0 + bo + Wo att; the offset rides in r0."""
  o = ops()
  M = 1000
  g = torch.Generator().manual_seed(90)
  att = torch.randn(M, K0_, generator=g).to(BF)
  r0 = fold_rows(M, family, g)
  wts = ffn_weights(g)
  ko, bo, kp, bp, r1 = tail_operands(g, M)
  ref = tail64(att, r0, ko, bo, wts, kp, bp, r1)
  F = FfnDev(dev, *wts)
  wo, wp = L.dense_kernel(ko.numpy(), BF, dev), L.dense_kernel(kp.numpy(), BF, dev)
  ad, r0d, r1d, bod, bpd = att.to(dev), r0.to(dev), r1.to(dev), bo.to(dev), bp.to(dev)
  outs = []
  for _ in range(2):
    out = torch.full((M, C_), float("nan"), dtype=BF, device=dev)
    o.st_tail(ad, wo, bod, r0d, F.w1, F.aux, F.w2, F.b2, wp, bpd, r1d, out, LN_EPS)
    outs.append(out)
  out_u = tail_unfused(o, ad, wo, bod, r0d, F, wp, bpd, r1d)
  torch.cuda.synchronize()
  assert torch.equal(outs[0], outs[1])
  fold_gate(f"st_tail-bf16-{family}-{M}x{C_}", outs[0], out_u, ref)


def attention_operands(g, R, T, Tk):
  """bf16 q, k, v [R, T|Tk, H, S] and their ldm_attention_ms layouts (as test_round3_gpu builds them)."""
  kb, vb = (torch.randn(R, Tk, H_, S_, generator=g).to(BF) for _ in range(2))
  kd = torch.zeros(R, Tk, H_, SP_); kd[..., :S_] = kb.float(); kd[..., L.MS_DIM] = 1.0
  vt = torch.zeros(R, K0_, 80)
  vv = torch.zeros(R, Tk, H_, SP_); vv[..., :S_] = vb.float(); vv[..., L.MS_DIM] = 1.0
  vt[:, :, :Tk] = vv.reshape(R, Tk, K0_).permute(0, 2, 1)
  return kb, vb, kd.reshape(R, Tk, K0_).to(BF), vt.to(BF)


def attention64(q, kb, vb):
  """float64 softmax(q k^T / sqrt(S)) v, padded to the 48-wide head layout: [R * T, K0]."""
  R, T = q.shape[:2]
  logits = torch.einsum("nqhs,nchs->nhqc", q.double(), kb.double()) * S_ ** -0.5
  a = torch.einsum("nhqc,nchs->nqhs", torch.softmax(logits, dim=3), vb.double())
  ap = torch.zeros(R, T, H_, SP_, dtype=torch.float64)
  ap[..., :S_] = a
  return ap.reshape(R * T, K0_)


@pytest.mark.parametrize("family", FOLD_FAMILIES)
def test_st_xtail_layernorm_fold(dev, family):
  """ldm_st_xtail: cross-attention, then the st_tail chain; the offset rides in r0."""
  o = ops()
  R, T, Tk = 3, 256, 77
  M = R * T
  g = torch.Generator().manual_seed(100)
  qb = (torch.randn(R, T, H_, S_, generator=g) * 2.0).to(BF)
  kb, vb, kd, vt = attention_operands(g, R, T, Tk)
  qd = torch.zeros(R, T, H_, SP_); qd[..., :S_] = qb.float() * (S_ ** -0.5 * L.MS_LOG2E)
  qd = qd.reshape(R, T, K0_).to(BF)
  r0 = fold_rows(M, family, g)
  wts = ffn_weights(g)
  ko, bo, kp, bp, r1 = tail_operands(g, M)
  ref = tail64(attention64(qb, kb, vb), r0, ko, bo, wts, kp, bp, r1)
  F = FfnDev(dev, *wts)
  wo, wp = L.dense_kernel(ko.numpy(), BF, dev), L.dense_kernel(kp.numpy(), BF, dev)
  qd, kd, vt = qd.to(dev), kd.to(dev), vt.to(dev)
  r0d, r1d, bod, bpd = r0.to(dev), r1.to(dev), bo.to(dev), bp.to(dev)
  outs = []
  for _ in range(2):
    out = torch.full((M, C_), float("nan"), dtype=BF, device=dev)
    o.st_xtail(qd, kd, vt, wo, bod, r0d, F.w1, F.aux, F.w2, F.b2, wp, bpd, r1d, out, LN_EPS)
    outs.append(out)
  att = torch.empty(R, T, K0_, dtype=BF, device=dev)
  o.attention(qd, kd, vt, att, H_, SP_, S_ ** -0.5, matrix_softmax=True)
  out_u = tail_unfused(o, att, wo, bod, r0d, F, wp, bpd, r1d)
  torch.cuda.synchronize()
  assert torch.equal(outs[0], outs[1])
  fold_gate(f"st_xtail-bf16-{family}-{R}x{T}x{C_}", outs[0], out_u, ref)


@pytest.mark.parametrize("family", FOLD_FAMILIES)
def test_st_block_layernorm_folds(dev, family):
  """ldm_st_block has two folds: LayerNorm(h1) before the query projection and LayerNorm(h2) before the
  feed-forward; the offset in r0 reaches both."""
  o = ops()
  R, T, Tk = 2, 384, 77
  M = R * T
  g = torch.Generator().manual_seed(110)
  att1 = torch.randn(M, K0_, generator=g).to(BF)
  r0 = fold_rows(M, family, g)
  g2, be2 = 1.0 + 0.3 * torch.randn(C_, generator=g), 0.2 * torch.randn(C_, generator=g)
  ko1 = torch.randn(K0_, C_, generator=g) * K0_ ** -0.5
  bo1 = torch.randn(C_, generator=g)
  kq = torch.randn(C_, H_, S_, generator=g) * C_ ** -0.5    # the query projection has no bias (unet.py:262)
  kb, vb, kd, vt = attention_operands(g, R, T, Tk)
  wts = ffn_weights(g)
  ko2, bo2, kp, bp, r1 = tail_operands(g, M)
  # float64
  h1 = r0.double() + att1.double() @ ko1.double() + bo1.double()
  q = torch.einsum("mc,chs->mhs", O.layer_norm(h1, g2.double(), be2.double(), eps=LN_EPS), kq.double())
  h2 = h1 + attention64(q.reshape(R, T, H_, S_), kb, vb) @ ko2.double() + bo2.double()
  ref = r1.double() + ffn64(h2, *wts) @ kp.double() + bp.double()
  # device operands
  wq_nk = torch.zeros(H_, SP_, C_)
  wq_nk[:, :S_] = kq.permute(1, 2, 0) * (S_ ** -0.5 * L.MS_LOG2E)
  wq_nk = wq_nk.reshape(K0_, C_)
  wq, qcs, qb = L.ln_fold(wq_nk, g2.numpy(), be2.numpy(), None, BF, dev)
  F = FfnDev(dev, *wts)
  wo1, wo2, wp = (L.dense_kernel(k.numpy(), BF, dev) for k in (ko1, ko2, kp))
  ad, r0d, r1d = att1.reshape(R, T, K0_).to(dev), r0.to(dev), r1.to(dev)
  bo1d, bo2d, bpd = bo1.to(dev), bo2.to(dev), bp.to(dev)
  kd, vt = kd.to(dev), vt.to(dev)
  outs = []
  for _ in range(2):
    out = torch.full((M, C_), float("nan"), dtype=BF, device=dev)
    o.st_block(ad, wo1, bo1d, r0d, wq, qcs, qb, kd, vt, wo2, bo2d, F.w1, F.aux, F.w2, F.b2, wp, bpd, r1d, out,
               LN_EPS)
    outs.append(out)
  # unfused: per-layer launches, each LayerNorm by ldm_layernorm into bf16 rows
  h1d = torch.empty(M, C_, dtype=BF, device=dev)
  o.linear(ad.view(M, K0_), wo1, h1d, bias=bo1d, residual=r0d)
  ln1 = torch.empty(M, C_, dtype=BF, device=dev)
  o.layernorm(h1d, g2.to(dev), be2.to(dev), ln1, LN_EPS)
  qd = torch.empty(R, T, K0_, dtype=BF, device=dev)
  o.linear(ln1, wq_nk.to(BF).to(dev), qd.view(M, K0_))
  a2 = torch.empty(R, T, K0_, dtype=BF, device=dev)
  o.attention(qd, kd, vt, a2, H_, SP_, S_ ** -0.5, matrix_softmax=True)
  out_u = tail_unfused(o, a2, wo2, bo2d, h1d, F, wp, bpd, r1d)
  torch.cuda.synchronize()
  assert torch.equal(outs[0], outs[1])
  fold_gate(f"st_block-bf16-{family}-{R}x{T}x{C_}", outs[0], out_u, ref)
