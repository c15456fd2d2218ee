"""Split-K completion at the planned split counts and every form of the split-K GroupNorm.

A split-K product leaves `split` float32 slabs in the workspace; they are summed either by the plain reduce
(splitk_epilogue_vec_kernel, or splitk_epilogue_kernel when a pointer is not 16-byte aligned) or inside the
GroupNorm that consumes the product (ldm_groupnorm_splitk, gn_fused.h with SK = true).  The second path has
forms (GB groups per workgroup, S chunks per pixel, NT threads, MAXCH chunks per thread) that batch SU slabs
(SU = 4 on the one-wave form NT = 64, else 2) and KB chunks per round trip, load slab 0 for the dead slots of
the last SU batch, skip chunk batches with no pixel (k0 * P >= HW, P = NT / S pixels per pass) and park idle
threads (NT % S) on element 0 of the workspace.  Every case here names the form it targets and asserts that
`ldm_groupnorm_splitk_form` returns it, and that `ldm_gemm_splits` returns its effective split.

Cases: (a) every packaged plan-table entry with split > 1 whose output the U-Net completes inside a GroupNorm
(stride-1 and stride-2 convolutions, the ResBlock's second convolution with its shortcut as extra K columns
(" x2"), and the folded FF-out + proj_out product (conv0 " x2", B = the table's rows, HW = M / B)), run with
the table's (tile, split); the upsampling convolutions are not deferred by the U-Net and are left out.  A key
names the shape, not the epilogue: each case takes the U-Net's epilogue for its geometry, and a same-width
stride-1 key (a ResBlock's conv1, or its conv2 without a shortcut) runs with both.
(b) synthetic cases that fill the forms the plan tables do not reach, with idle lanes, HW < P, HW not a
multiple of P, B not a multiple of 8 (the grid rounds B up to 8), every split residue mod SU and splits whose
last slab has fewer K-tiles than the others.  The split-K GroupNorm has no (NT, MAXCH) = (512, 8) form with
S = 5: the 256-thread form covers 16 * floor(256 / 5) = 816 pixels, 8 * floor(512 / 5) = 816 as well; only
S = 10 (f32, C = 1280) reaches it, at HW 401 - 408.  Channel counts 320 / 640 / 1280 give S = 5 or 10, which
divide no NT: the C = 512 cases give S = 2 / 4.

Epilogues as the U-Net passes them: conv1 = bias + a column slice of the wide [B, sum Cout] time-embedding
tensor (add_ld > C), SiLU; conv2m = bias + the shortcut's channels of x2; conv2u = bias + residual (a channel
slice); down = the stride-2 convolution, bias only; fold = conv0 product with residual and x2.  The product
and the GroupNorm output are channel slices of wider NaN-filled buffers at a 16-byte channel offset, as the
skip-concat buffers are; their row strides are multiples of 8 elements.  `scalar` cases offset the addend by
one float: the plain reduce then runs splitk_epilogue_kernel; every other case asserts, from its launch
parameters, that it runs splitk_epilogue_vec_kernel.  `shift` cases carry a per-group offset in the bias (256 bf16, 1000 f32).

The workspace is exactly ldm_gemm_workspace_bytes(p) = splits x M x N x 4 bytes at the front of a larger
buffer filled with 0xFF (float32 NaN): a slab element that is read and used but was never written, or read
past the end, shows up as NaN, and the guard tail must stay 0xFF.  Three completions of one product:
(i) the plain reduce, (ii) ldm_groupnorm_splitk storing the product, (iii) the same without storing it.
(i) and (ii) store identical bits; the GroupNorm of (ii) and (iii) is bit-identical to (i) followed by the
single-launch GroupNorm; (iii) leaves its product buffer at NaN; two runs give the same bits.  The product
is checked against the float64 product on samples {0, B/2, B-1} (bf16: within 1 ulp at max(|ref|, 2^-6);
f32: within 2^-20 A with A the float64 product of the magnitudes plus |bias| + |addend| + |residual|, and
relative L2 <= 2e-6), the GroupNorm output against the float64 GroupNorm of the product as stored
(tests/norm_check.py).

Coverage (form = GB/S/NT/MAXCH; spl = effective split; %SU = split mod SU; idl = NT % S idle lanes;
P = NT // S pixels per pass):
  case                                                               form        spl %SU idl  HW vs P      epilogue
  plan-bf16-conv1-B32-8x8-C1280-t9-split4-form1.5.64.8               1/5/64/8      4   0   4  HW % P = 4   conv1
  plan-bf16-conv1-B32-16x16-C640-t15-split2-form2.5.256.8            2/5/256/8     2   0   1  HW % P = 1   conv1
  plan-bf16-conv2u-B32-16x16-C640-t15-split2-form2.5.256.8           2/5/256/8     2   0   1  HW % P = 1   conv2u
  plan-bf16-conv2u-B32-8x8-C1280-t9-split4-form1.5.64.8              1/5/64/8      4   0   4  HW % P = 4   conv2u
  plan-bf16-conv1-B32-4x4-C1280-t11-split12-form1.5.64.8             1/5/64/8     12   0   4  HW % P = 4   conv1
  plan-bf16-conv2u-B32-4x4-C1280-t11-split12-form1.5.64.8            1/5/64/8     12   0   4  HW % P = 4   conv2u
  plan-bf16-conv2m-B32-16x16-C640-t9-split2-form2.5.256.8            2/5/256/8     2   0   1  HW % P = 1   conv2m
  plan-bf16-conv2m-B32-8x8-C1280-t9-split4-form1.5.64.8              1/5/64/8      4   0   4  HW % P = 4   conv2m
  plan-bf16-conv2m-B32-4x4-C1280-t11-split12-form1.5.64.8            1/5/64/8     12   0   4  HW % P = 4   conv2m
  plan-bf16-fold-B32-16x16-C640-t9-split2-form2.5.256.8              2/5/256/8     2   0   1  HW % P = 1   fold
  plan-bf16-fold-B32-8x8-C1280-t1-split3-form1.5.64.8                1/5/64/8      3   3   4  HW % P = 4   fold
  plan-bf16-fold-B32-4x4-C1280-t18-split2-form1.5.64.8               1/5/64/8      2   2   4  HW % P = 4   fold
  plan-bf16-conv1-B16-16x16-C640-t9-split4-form2.5.256.8             2/5/256/8     4   0   1  HW % P = 1   conv1
  plan-bf16-conv1-B16-8x8-C1280-t9-split8-form1.5.64.8               1/5/64/8      8   0   4  HW % P = 4   conv1
  plan-bf16-conv1-B16-32x32-C320-t9-split2-form4.5.512.16            4/5/512/16    2   0   2  HW % P = 4   conv1
  plan-bf16-conv2u-B16-32x32-C320-t9-split2-form4.5.512.16           4/5/512/16    2   0   2  HW % P = 4   conv2u
  plan-bf16-conv1-B16-16x16-C640-t11-split3-form2.5.256.8            2/5/256/8     3   1   1  HW % P = 1   conv1
  plan-bf16-conv2u-B16-16x16-C640-t11-split3-form2.5.256.8           2/5/256/8     3   1   1  HW % P = 1   conv2u
  plan-bf16-conv1-B16-4x4-C1280-t18-split8-form1.5.64.8              1/5/64/8      8   0   4  HW % P = 4   conv1
  plan-bf16-conv2u-B16-4x4-C1280-t18-split8-form1.5.64.8             1/5/64/8      8   0   4  HW % P = 4   conv2u
  plan-bf16-conv2u-B16-8x8-C1280-t9-split8-form1.5.64.8              1/5/64/8      8   0   4  HW % P = 4   conv2u
  plan-bf16-down-B16-8x8-C640-t4-split6-form2.5.256.8                2/5/256/8     6   0   1  HW % P = 13  down
  plan-bf16-conv2m-B16-16x16-C640-t11-split3-form2.5.256.8           2/5/256/8     3   1   1  HW % P = 1   conv2m
  plan-bf16-conv2m-B16-8x8-C1280-t9-split8-form1.5.64.8              1/5/64/8      8   0   4  HW % P = 4   conv2m
  plan-bf16-conv2m-B16-4x4-C1280-t18-split8-form1.5.64.8             1/5/64/8      8   0   4  HW % P = 4   conv2m
  plan-bf16-conv2m-B16-32x32-C320-t9-split2-form4.5.512.16           4/5/512/16    2   0   2  HW % P = 4   conv2m
  plan-f32-conv1-B8-16x16-C640-t7-split8-form1.5.256.8               1/5/256/8     8   0   1  HW % P = 1   conv1
  plan-f32-conv1-B8-8x8-C1280-t3-split16-form1.10.256.8              1/10/256/8   16   0   6  HW % P = 14  conv1
  plan-f32-conv1-B8-32x32-C320-t7-split4-form2.5.512.16              2/5/512/16    4   0   2  HW % P = 4   conv1
  plan-f32-conv2u-B8-16x16-C640-t6-split8-form1.5.256.8              1/5/256/8     8   0   1  HW % P = 1   conv2u
  plan-f32-conv2u-B8-8x8-C1280-t7-split16-form1.10.256.8             1/10/256/8   16   0   6  HW % P = 14  conv2u
  plan-f32-conv1-B8-8x8-C1280-t4-split8-form1.10.256.8               1/10/256/8    8   0   6  HW % P = 14  conv1
  plan-f32-conv1-B8-32x32-C640-t7-split2-form1.5.512.16              1/5/512/16    2   0   2  HW % P = 4   conv1
  plan-f32-conv1-B8-16x16-C1280-t7-split8-form1.10.256.16            1/10/256/16   8   0   6  HW % P = 6   conv1
  plan-f32-conv1-B8-32x32-C640-t7-split4-form1.5.512.16              1/5/512/16    4   0   2  HW % P = 4   conv1
  plan-f32-conv1-B8-16x16-C1280-t8-split4-form1.10.256.16            1/10/256/16   4   0   6  HW % P = 6   conv1
  plan-f32-conv2u-B8-32x32-C640-t8-split2-form1.5.512.16             1/5/512/16    2   0   2  HW % P = 4   conv2u
  plan-f32-conv2u-B8-16x16-C1280-t6-split4-form1.10.256.16           1/10/256/16   4   0   6  HW % P = 6   conv2u
  plan-bf16-conv1-B8-16x16-C1280-t15-split4-form1.5.256.8            1/5/256/8     4   0   1  HW % P = 1   conv1
  plan-bf16-conv1-B8-32x32-C640-t9-split2-form2.5.512.16             2/5/512/16    2   0   2  HW % P = 4   conv1
  plan-bf16-conv2u-B8-32x32-C640-t15-split2-form2.5.512.16           2/5/512/16    2   0   2  HW % P = 4   conv2u
  plan-bf16-conv2u-B8-16x16-C1280-t15-split4-form1.5.256.8           1/5/256/8     4   0   1  HW % P = 1   conv2u
  plan-bf16-conv2m-B8-32x32-C640-t9-split2-form2.5.512.16            2/5/512/16    2   0   2  HW % P = 4   conv2m
  plan-bf16-conv2m-B8-16x16-C1280-t9-split4-form1.5.256.8            1/5/256/8     4   0   1  HW % P = 1   conv2m
  plan-bf16-fold-B8-32x32-C640-t9-split2-form2.5.512.16              2/5/512/16    2   0   2  HW % P = 4   fold
  plan-bf16-fold-B8-8x8-C1280-t1-split8-form1.5.256.8                1/5/256/8     8   0   1  HW % P = 13  fold
  syn-bf16-conv1-B17-4x4-C1280-t2-split13-form1.5.64.8               1/5/64/8     13   1   4  HW % P = 4   conv1
  syn-bf16-conv1-B17-4x4-C1280-t2-split13-form1.5.64.8-shift         1/5/64/8     13   1   4  HW % P = 4   conv1
  syn-bf16-conv2u-B16-2x2-C1280-t2-split7-form1.5.64.8               1/5/64/8      7   3   4  HW < P       conv2u
  syn-bf16-conv2m-B16-8x12-C1280-t2-split9-form1.5.64.8              1/5/64/8      9   1   4  HW = 8 P     conv2m
  syn-bf16-conv1-B16-10x10-C1280-t2-split6-form1.5.64.16             1/5/64/16     6   2   4  HW % P = 4   conv1
  syn-bf16-conv2u-B24-12x16-C1280-t3-split5-form1.5.64.16            1/5/64/16     5   1   4  HW = 16 P    conv2u
  syn-bf16-fold-B16-3x3-C1280-t4-split2-form1.5.64.8                 1/5/64/8      2   2   4  HW < P       fold
  syn-bf16-conv1-B8-8x8-C1280-t2-split16-form1.5.256.8               1/5/256/8    16   0   1  HW % P = 13  conv1
  syn-bf16-conv2u-B3-20x24-C1280-t2-split5-form1.5.256.16            1/5/256/16    5   1   1  HW % P = 21  conv2u
  syn-bf16-conv1-B1-29x31-C1280-t2-split3-form1.5.512.16             1/5/512/16    3   1   2  HW % P = 83  conv1
  syn-bf16-conv1-B16-4x4-C1280-t2-split8-form1.5.64.8-scalar         1/5/64/8      8   0   4  HW % P = 4   conv1
  syn-bf16-conv2u-B33-4x4-C640-t2-split3-form2.5.64.8                2/5/64/8      3   3   4  HW % P = 4   conv2u
  syn-bf16-conv2m-B32-11x11-C640-t2-split2-form2.5.64.16             2/5/64/16     2   2   4  HW % P = 1   conv2m
  syn-bf16-conv1-B3-7x9-C640-t2-split3-form2.5.256.8                 2/5/256/8     3   1   1  HW % P = 12  conv1
  syn-bf16-conv2u-B2-24x24-C640-t2-split8-form2.5.256.16             2/5/256/16    8   0   1  HW % P = 15  conv2u
  syn-bf16-conv1-B1-30x30-C640-t2-split5-form2.5.512.16              2/5/512/16    5   1   2  HW % P = 84  conv1
  syn-bf16-conv1-B65-4x4-C320-t2-split8-form4.5.64.8                 4/5/64/8      8   0   4  HW % P = 4   conv1
  syn-bf16-conv2m-B64-10x10-C320-t2-split12-form4.5.64.16            4/5/64/16    12   0   4  HW % P = 4   conv2m
  syn-bf16-conv1-B5-5x7-C320-t2-split2-form4.5.256.8                 4/5/256/8     2   0   1  HW < P       conv1
  syn-bf16-conv2u-B1-16x32-C320-t2-split5-form4.5.256.16             4/5/256/16    5   1   1  HW % P = 2   conv2u
  syn-bf16-conv2u-B16-8x8-C512-t2-split4-form1.2.64.8                1/2/64/8      4   0   0  HW = 2 P     conv2u
  syn-bf16-conv1-B16-16x20-C512-t2-split3-form1.2.64.16              1/2/64/16     3   3   0  HW = 10 P    conv1
  syn-bf16-conv1-B2-40x40-C512-t2-split2-form1.2.256.16              1/2/256/16    2   0   0  HW % P = 64  conv1
  syn-f32-conv1-B16-4x4-C1280-t2-split12-form1.10.64.8               1/10/64/8    12   0   4  HW % P = 4   conv1
  syn-f32-conv1-B16-4x4-C1280-t2-split12-form1.10.64.8-shift         1/10/64/8    12   0   4  HW % P = 4   conv1
  syn-f32-conv2u-B17-7x7-C1280-t3-split5-form1.10.64.16              1/10/64/16    5   1   4  HW % P = 1   conv2u
  syn-f32-conv2u-B2-8x51-C1280-t2-split2-form1.10.512.8              1/10/512/8    2   0   2  HW = 8 P     conv2u
  syn-f32-conv1-B2-10x20-C1280-t2-split3-form1.10.256.8              1/10/256/8    3   1   6  HW = 8 P     conv1
  syn-f32-conv2u-B1-24x24-C1280-t2-split8-form1.10.512.16            1/10/512/16   8   0   2  HW % P = 15  conv2u
  syn-f32-conv2m-B16-3x5-C1280-t2-split9-form1.10.64.8               1/10/64/8     9   1   4  HW % P = 3   conv2m
  syn-f32-fold-B16-6x6-C1280-t4-split7-form1.10.64.8                 1/10/64/8     7   3   4  HW = 6 P     fold
  syn-f32-conv1-B16-4x4-C1280-t2-split13-form1.10.64.8-scalar        1/10/64/8    13   1   4  HW % P = 4   conv1
  syn-f32-conv2u-B17-4x4-C640-t2-split9-form1.5.64.8                 1/5/64/8      9   1   4  HW % P = 4   conv2u
  syn-f32-conv1-B16-12x12-C640-t2-split3-form1.5.64.16               1/5/64/16     3   3   4  HW = 12 P    conv1
  syn-f32-conv1-B1-20x21-C640-t2-split5-form1.5.256.16               1/5/256/16    5   1   1  HW % P = 12  conv1
  syn-f32-conv1-B32-5x5-C320-t2-split7-form2.5.64.8                  2/5/64/8      7   3   4  HW % P = 1   conv1
  syn-f32-conv2u-B33-13x13-C320-t2-split2-form2.5.64.16              2/5/64/16     2   2   4  HW % P = 1   conv2u
  syn-f32-conv1-B3-9x9-C320-t2-split6-form2.5.256.8                  2/5/256/8     6   0   1  HW % P = 30  conv1
  syn-f32-conv2u-B1-20x30-C320-t2-split3-form2.5.256.16              2/5/256/16    3   1   1  HW % P = 39  conv2u
  syn-f32-conv2u-B16-8x16-C512-t2-split2-form1.4.64.8                1/4/64/8      2   2   0  HW = 8 P     conv2u
  syn-f32-conv1-B2-32x32-C512-t2-split3-form1.4.256.16               1/4/256/16    3   1   0  HW = 16 P    conv1
"""
import ctypes as C
import glob
import json
import math
import os
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd._lib import BF16, F32 as F32C, GemmParams, lib  # noqa: E402
from norm_check import bf16_ulp, check  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

F32, BF = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF: "bf16"}
GROUPS = 32
GN_EPS = 1e-5                 # the ResBlocks' (unet.py GN_EPS_RES)
SHIFT = {BF: 256.0, F32: 1000.0}
F32_GATE = 2.0 ** -20         # per element, in units of A

# one launch: output [B, H, W, C]; conv: input channels Cin (+ Cin2 shortcut channels), stride s; fold: a dense
# over 4 C (+ C as x2) columns.  form = (GB, S, NT, MAXCH) the split-K GroupNorm must run, split = effective split
Case = namedtuple("Case", "src dt B H W Cin C Cin2 s epi tile split_k split form family scalar")


def _skeleton(c):
  """ldm_gemm_params of the case's launch without pointers (what the host plan functions read)."""
  p = GemmParams()
  p.N, p.batch, p.tile, p.split_k = c.C, 1, c.tile, c.split_k
  p.dtype = p.out_dtype = BF16 if c.dt == BF else F32C
  p.M = c.B * c.H * c.W
  if c.epi == "fold":
    p.K, p.Cin2 = 5 * c.C, c.C
  else:
    p.conv, p.B, p.H, p.W, p.Cin, p.OH, p.OW, p.stride = 1, c.B, c.H * c.s, c.W * c.s, c.Cin, c.H, c.W, c.s
    p.K, p.Cin2 = 9 * c.Cin + c.Cin2, c.Cin2
  return p


def gn_form(B, HW, Cc, dtype):
  f = (C.c_int32 * 4)()
  st = lib.ldm_groupnorm_splitk_form(B, HW, Cc, GROUPS, BF16 if dtype == BF else F32C, f)
  return tuple(f) if st == 0 else None


def eff_split(c):
  return lib.ldm_gemm_splits(C.byref(_skeleton(c)))


def _fields(key):
  return dict((k.rstrip("0123456789"), int(k[len(k.rstrip("0123456789")):])) for k in key.split())


def _plan_cases():
  d = os.path.join(os.path.dirname(ops.__file__), "plans")
  out, seen = [], set()
  for path in sorted(glob.glob(os.path.join(d, "*.json"))):
    tab = json.load(open(path))
    rows = tab["config"]["rows"]
    for key, (tile, split) in tab["plans"].items():
      f = _fields(key)
      x2 = key.endswith(" x2")
      if split <= 1 or f["act"] or (f["conv"] and f["u"]) or (not f["conv"] and not x2):
        continue
      dt = BF if f["dt"] == BF16 else F32
      M, N, K = f["M"], f["N"], f["K"]
      if f["conv"]:
        s = f["s"]
        H, W = f["H"] // s, f["W"] // s
        B = M // (H * W)
        Cin, Cin2 = (N, K - 9 * N) if x2 else (K // 9, 0)
        # a key names the shape, not the epilogue: the epilogues are the U-Net's for that geometry, chosen here.
        # A same-width stride-1 key is a ResBlock's conv1 (temb addend) or its conv2 without shortcut (residual):
        # it runs as both
        epis = ["conv2m"] if x2 else ["down"] if s == 2 else ["conv1", "conv2u"] if Cin == N else ["conv1"]
      else:
        B, s, Cin, Cin2, epis = rows, 1, 4 * N, N, ["fold"]
        H = W = math.isqrt(M // rows)
        assert H * W * rows == M and K == 5 * N, key
      for epi in epis:
        c = Case("plan", dt, B, H, W, Cin, N, Cin2, s, epi, tile, split, 0, None, "plain", False)
        c = c._replace(split=eff_split(c), form=gn_form(B, H * W, N, dt))
        if c.form is None:
          continue
        k = (B, H * W, N, dt, c.split, c.form, epi)
        if k not in seen:
          seen.add(k)
          out.append(c)
  return out


def S(dt, B, H, W, Cin, Cc, split, form, epi="conv1", tile=2, split_k=None, Cin2=0, s=1, family="plain",
      scalar=False):
  if epi == "fold":
    Cin, Cin2 = 4 * Cc, Cc
  return Case("syn", dt, B, H, W, Cin, Cc, Cin2, s, epi, tile, split_k or split, split, form, family, scalar)


# synthetic cases: (dtype, B, H, W, Cin, C, effective split, form).  K-tiles: 9 Cin / 64 (bf16), 9 Cin / 32 (f32)
SYN = [
    # bf16, C = 1280 (GB 1, S 5): one-wave form from B = 16
    S(BF, 17, 4, 4, 640, 1280, 13, (1, 5, 64, 8)),                         # 90 K-tiles: 12 x 7 + 6
    S(BF, 17, 4, 4, 640, 1280, 13, (1, 5, 64, 8), family="shift"),
    S(BF, 16, 2, 2, 1280, 1280, 7, (1, 5, 64, 8), epi="conv2u"),           # HW 4 < P 12; 6 x 26 + 24
    S(BF, 16, 8, 12, 640, 1280, 9, (1, 5, 64, 8), epi="conv2m", Cin2=640),
    S(BF, 16, 10, 10, 640, 1280, 6, (1, 5, 64, 16)),
    S(BF, 24, 12, 16, 640, 1280, 5, (1, 5, 64, 16), epi="conv2u", tile=3),
    S(BF, 16, 3, 3, 640, 1280, 2, (1, 5, 64, 8), epi="fold", tile=4),
    S(BF, 8, 8, 8, 1024, 1280, 16, (1, 5, 256, 8)),                        # SU = 2
    S(BF, 3, 20, 24, 640, 1280, 5, (1, 5, 256, 16), epi="conv2u"),
    S(BF, 1, 29, 31, 640, 1280, 3, (1, 5, 512, 16)),
    S(BF, 16, 4, 4, 640, 1280, 8, (1, 5, 64, 8), scalar=True),
    # bf16, C = 640 (GB 2, S 5): one-wave from B = 32
    S(BF, 33, 4, 4, 640, 640, 3, (2, 5, 64, 8), epi="conv2u"),
    S(BF, 32, 11, 11, 640, 640, 2, (2, 5, 64, 16), epi="conv2m", Cin2=320),
    S(BF, 3, 7, 9, 640, 640, 3, (2, 5, 256, 8)),
    S(BF, 2, 24, 24, 640, 640, 8, (2, 5, 256, 16), epi="conv2u"),          # 90 K-tiles: 7 x 12 + 6
    S(BF, 1, 30, 30, 320, 640, 5, (2, 5, 512, 16)),
    # bf16, C = 320 (GB 4, S 5): one-wave from B = 64
    S(BF, 65, 4, 4, 640, 320, 8, (4, 5, 64, 8)),                           # 7 x 12 + 6
    S(BF, 64, 10, 10, 640, 320, 12, (4, 5, 64, 16), epi="conv2m", Cin2=320),
    S(BF, 5, 5, 7, 640, 320, 2, (4, 5, 256, 8)),
    S(BF, 1, 16, 32, 320, 320, 5, (4, 5, 256, 16), epi="conv2u"),
    # bf16, C = 512 (S 2 divides NT)
    S(BF, 16, 8, 8, 512, 512, 4, (1, 2, 64, 8), epi="conv2u"),
    S(BF, 16, 16, 20, 512, 512, 3, (1, 2, 64, 16)),
    S(BF, 2, 40, 40, 512, 512, 2, (1, 2, 256, 16)),
    # f32, C = 1280 (GB 1, S 10: P = 6 on the one-wave form, 4 idle lanes)
    S(F32, 16, 4, 4, 320, 1280, 12, (1, 10, 64, 8)),              # 90 K-tiles: 11 x 8 + 2
    S(F32, 16, 4, 4, 320, 1280, 12, (1, 10, 64, 8), family="shift"),
    S(F32, 17, 7, 7, 320, 1280, 5, (1, 10, 64, 16), epi="conv2u", Cin2=0, tile=3, split_k=5),
    S(F32, 2, 8, 51, 320, 1280, 2, (1, 10, 512, 8), epi="conv2u", Cin2=0),  # the only (512, 8) form
    S(F32, 2, 10, 20, 320, 1280, 3, (1, 10, 256, 8)),
    S(F32, 1, 24, 24, 320, 1280, 8, (1, 10, 512, 16), epi="conv2u"),
    S(F32, 16, 3, 5, 320, 1280, 9, (1, 10, 64, 8), epi="conv2m", Cin2=320),
    S(F32, 16, 6, 6, 640, 1280, 7, (1, 10, 64, 8), epi="fold", tile=4),
    S(F32, 16, 4, 4, 320, 1280, 13, (1, 10, 64, 8), split_k=13, scalar=True),
    # f32, C = 640 (GB 1, S 5)
    S(F32, 17, 4, 4, 320, 640, 9, (1, 5, 64, 8), epi="conv2u"),
    S(F32, 16, 12, 12, 320, 640, 3, (1, 5, 64, 16)),
    S(F32, 1, 20, 21, 320, 640, 5, (1, 5, 256, 16)),
    # f32, C = 320 (GB 2, S 5)
    S(F32, 32, 5, 5, 320, 320, 7, (2, 5, 64, 8)),
    S(F32, 33, 13, 13, 320, 320, 2, (2, 5, 64, 16), epi="conv2u"),
    S(F32, 3, 9, 9, 320, 320, 6, (2, 5, 256, 8)),
    S(F32, 1, 20, 30, 320, 320, 3, (2, 5, 256, 16), epi="conv2u"),
    # f32, C = 512 (S 4 divides NT)
    S(F32, 16, 8, 16, 256, 512, 2, (1, 4, 64, 8), epi="conv2u", Cin2=0, tile=2),
    S(F32, 2, 32, 32, 256, 512, 3, (1, 4, 256, 16)),
]

CASES = _plan_cases() + SYN


def su(form):
  return 4 if form[2] == 64 else 2


def case_id(c):
  fm = ".".join(str(v) for v in c.form)
  tail = ("-shift" if c.family == "shift" else "") + ("-scalar" if c.scalar else "")
  return (f"{c.src}-{DTN[c.dt]}-{c.epi}-B{c.B}-{c.H}x{c.W}-C{c.C}-t{c.tile}-split{c.split}-form{fm}" + tail)


def coverage_row(c):
  """the case's row of the coverage table in the module docstring"""
  GB, S_, NT, MC = c.form
  P, HW = NT // S_, c.H * c.W
  hw = "HW < P" if HW < P else ("HW = %d P" % (HW // P) if HW % P == 0 else "HW %% P = %d" % (HW % P))
  return "  %-66s %-11s %3d %3d %3d  %-12s %s" % (case_id(c), f"{GB}/{S_}/{NT}/{MC}", c.split, c.split % su(c.form),
                                                  NT % S_, hw, c.epi)


def vec_reduce(p):
  """True if ldm_gemm_reduce runs splitk_epilogue_vec_kernel for the parameters p, else splitk_epilogue_kernel (the
  conditions of build_args and launch_reduce, csrc/gemm.hip; no activation here)"""
  def al(q, n=16):
    return (q or 0) % n == 0
  return (p.ldc_n == 1 and p.N % 8 == 0 and p.ldc_m % 8 == 0 and p.stride_c % 8 == 0 and al(p.out) and
          (not p.residual or (p.ldr % 8 == 0 and p.stride_r % 8 == 0 and al(p.residual))) and
          (not p.bias or al(p.bias)) and (not p.addend or (al(p.addend) and p.add_ld % 4 == 0)) and
          al(p.workspace))


class _NoPlainReduce:
  """ops.groupnorm(pending=...) falls back to the plain reduce + a GroupNorm when the split-K form does not
  apply: inside this block that fallback is an error."""

  def __enter__(self):
    self._finish = ops.finish

    def refuse(pending):
      raise AssertionError("ops.groupnorm fell back to the plain reduce")
    ops.finish = refuse
    return self

  def __exit__(self, *exc):
    ops.finish = self._finish
    return False


def _rand(g, shape, scale=1.0):
  return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_splitk_completion(dev, c):
  dt, B, H, W, Cc = c.dt, c.B, c.H, c.W, c.C
  HW, M = H * W, c.B * c.H * c.W
  fold = c.epi == "fold"
  assert gn_form(B, HW, Cc, dt) == c.form, f"{case_id(c)}: the split-K GroupNorm no longer runs this form"
  assert eff_split(c) == c.split, f"{case_id(c)}: ldm_gemm no longer splits this launch {c.split} ways"
  torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
  g = torch.Generator().manual_seed(1000 + 7 * B + HW + Cc + c.split)
  esz = 2 if dt == BF else 4
  OFF = 16 // esz                                   # 16-byte channel offset of every sliced buffer
  GUARD = OFF                                       # (row strides OFF + C + GUARD: multiples of 8 elements)
  # ---- inputs, rounded to the kernel dtype (CPU) ----
  if fold:
    xa = _rand(g, (B, H, W, 4 * Cc)).to(dt)          # GEGLU output
    x2 = _rand(g, (B, H, W, Cc)).to(dt)              # the block's residual stream
    w = _rand(g, (Cc, 5 * Cc), (5 * Cc) ** -0.5).to(dt)
    wt = w
  else:
    xa = _rand(g, (B, H * c.s, W * c.s, c.Cin)).to(dt)
    k = _rand(g, (3, 3, c.Cin, Cc), (9 * c.Cin) ** -0.5).to(dt)
    wt = k.permute(3, 0, 1, 2).reshape(Cc, 9 * c.Cin)
    x2 = ks = None
    if c.Cin2:
      x2 = _rand(g, (B, H, W, c.Cin2)).to(dt)
      ks = _rand(g, (c.Cin2, Cc), c.Cin2 ** -0.5).to(dt)
      wt = torch.cat([wt, ks.t()], 1)
    wt = wt.contiguous()
  bias = 0.5 * _rand(g, (Cc,))
  if c.family == "shift":
    sign = torch.where(torch.rand(GROUPS, generator=g) < 0.5, -1.0, 1.0).double()
    bias = bias + (SHIFT[dt] * sign).repeat_interleave(Cc // GROUPS)
  bias = bias.float()
  addend = residual = None
  tall_d = res_d = None
  if c.epi == "conv1":                               # a column slice of the wide time-embedding tensor
    a0 = 64 + (1 if c.scalar else 0)
    tall = (0.5 * _rand(g, (B, a0 + Cc + 32))).float()
    addend = tall[:, a0:a0 + Cc]
    tall_d = tall.to(dev)[:, a0:a0 + Cc]
    assert tall_d.stride(0) > Cc and (tall_d.data_ptr() % 16 != 0) == c.scalar
  if c.epi in ("conv2u", "fold"):                    # a channel slice of a wider buffer
    rw = _rand(g, (B, H, W, OFF + Cc + GUARD)).to(dt)
    residual = rw[..., OFF:OFF + Cc]
    res_d = rw.to(dev)[..., OFF:OFF + Cc]
  gamma = (1.0 + 0.2 * _rand(g, (Cc,))).float()
  beta = (0.2 * _rand(g, (Cc,))).float()
  silu = c.epi != "conv2m"
  xd, wd, bd = xa.to(dev), wt.to(dev), bias.to(dev)
  x2d = None if x2 is None else x2.to(dev)
  gd, btd = gamma.to(dev), beta.to(dev)
  wide = (B, H, W, OFF + Cc + GUARD)

  def nan_buf():
    return torch.full(wide, float("nan"), dtype=dt, device=dev)

  def launch(out):
    if fold:
      return ops.linear(xd, wd, out, bias=bd, residual=res_d, x2=x2d, tile=c.tile, split_k=c.split_k,
                        defer_reduce=True)
    return ops.conv3x3(xd, wd, out, bias=bd, stride=c.s, addend=tall_d, residual=res_d, tile=c.tile,
                       split_k=c.split_k, defer_reduce=True, x2=x2d)

  # ---- the exact workspace of this launch ----
  probe = nan_buf()[..., OFF:OFF + Cc]
  if fold:
    p = _skeleton(c)
  else:
    p = ops._conv_params(xd, wd, probe, bd, c.s, False, tall_d, res_d, c.tile, c.split_k, False, x2d)
  need = lib.ldm_gemm_workspace_bytes(C.byref(p))
  assert lib.ldm_gemm_splits(C.byref(p)) == c.split
  assert need == c.split * M * Cc * 4, (need, c.split, M, Cc)
  ws_buf = torch.empty(need + 4096, dtype=torch.uint8, device=dev)

  def run(mode):
    """mode: 'reduce' (i), 'gn_store' (ii), 'gn_nostore' (iii) -> (product buffer, GroupNorm buffer or None)"""
    ws_buf.fill_(0xFF)
    ow = nan_buf()
    out = ow[..., OFF:OFF + Cc]
    gw = None
    pend = None
    try:
      with ops.workspace_scope(ws_buf[:need]):
        pend = launch(out)
        assert isinstance(pend, ops.PendingReduce) and not pend.done
        assert pend.p.workspace_bytes == need
        if mode == "reduce":
          assert vec_reduce(pend.p) == (not c.scalar), \
              f"{case_id(c)}: the plain reduce would not run the {'scalar' if c.scalar else 'vectorised'} kernel"
          ops.finish(pend)
        else:
          gw = nan_buf()
          with _NoPlainReduce():
            ops.groupnorm(out, gd, btd, gw[..., OFF:OFF + Cc], GN_EPS, silu=silu, groups=GROUPS, pending=pend,
                          store_x=mode == "gn_store")
        assert pend.done
    finally:
      if pend is not None and not pend.done:     # a failed step: release the workspace for the next case
        pend.done = True
        ops._outstanding().pop(pend.ws.data_ptr(), None)
    torch.cuda.synchronize()
    assert bool((ws_buf[need:] == 0xFF).all()), "the completion wrote past the workspace"
    return ow, gw

  pi, _ = run("reduce")
  pii, gii = run("gn_store")
  pii2, gii2 = run("gn_store")
  piii, giii = run("gn_nostore")
  gref = nan_buf()
  assert lib.ldm_groupnorm_fused_supported(B, HW, Cc, GROUPS, ops.code(dt)) == 1
  ops.groupnorm(pi[..., OFF:OFF + Cc], gd, btd, gref[..., OFF:OFF + Cc], GN_EPS, silu=silu, groups=GROUPS,
                fused=True)
  torch.cuda.synchronize()
  label = case_id(c)
  for name, t in (("reduce out", pi), ("gn out", pii), ("gn out (no store)", piii), ("gn", gii), ("gn", giii),
                  ("single-launch gn", gref)):
    assert bool(torch.isnan(t[..., :OFF].float()).all() and torch.isnan(t[..., OFF + Cc:].float()).all()), \
        f"{label}: {name} wrote outside its channel slice"
  prod = pi[..., OFF:OFF + Cc]
  assert bool(torch.isfinite(prod.float()).all()), f"{label}: the plain reduce produced non-finite values"
  # 1. the split-K GroupNorm stores the plain reduce's bits
  assert torch.equal(prod, pii[..., OFF:OFF + Cc]), f"{label}: stored product differs from the plain reduce"
  # 2. its normalisation is the single-launch GroupNorm's of the reduced product, stored or not
  gsl = slice(OFF, OFF + Cc)
  assert torch.equal(gii[..., gsl], gref[..., gsl]), f"{label}: split-K GroupNorm != reduce + GroupNorm"
  assert torch.equal(giii[..., gsl], gref[..., gsl]), f"{label}: split-K GroupNorm (no store) != reduce + GroupNorm"
  # 3. (iii) leaves the product untouched; two runs give the same bits
  assert bool(torch.isnan(piii.float()).all()), f"{label}: store_x=False wrote the product"
  assert torch.equal(pii[..., gsl], pii2[..., gsl]) and torch.equal(gii[..., gsl], gii2[..., gsl]), f"{label}: two runs differ"
  # 4. the stored product against float64, samples {0, B/2, B-1}
  rows = sorted({0, B // 2, B - 1})
  f32 = dt == F32                                   # (A, the magnitude bound, is needed for the f32 gate only)

  def product(op):
    """the float64 product of the case's operands on `rows`, every operand passed through `op`"""
    if fold:
      w64 = op(w.double())
      y = op(xa[rows].double()) @ w64[:, :4 * Cc].t() + op(x2[rows].double()) @ w64[:, 4 * Cc:].t()
    else:
      y = O.conv2d(op(xa[rows].double()), op(k.double()), None, stride=c.s)
      if c.Cin2:
        y = y + O.dense(op(x2[rows].double()), op(ks.double()))
    y = y + op(bias.double())
    if addend is not None:
      y = y + op(addend[rows].double())[:, None, None, :]
    if residual is not None:
      y = y + op(residual[rows].double())
    return y

  ref = product(lambda t: t)
  mag = product(torch.abs) if f32 else None
  got = prod[rows].cpu().double()
  err = (got - ref).abs()
  if dt == BF:
    worst = (err / bf16_ulp(ref)).max().item()
    print(f"{label}: product worst err {worst:.3f} bf16 ulp")
    assert worst <= 1.0, f"{label}: a product element is {worst:.2f} bf16 ulp from the float64 reference"
  else:
    worst = (err / mag).max().item()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"{label}: product worst err/A {worst:.3e} (gate {F32_GATE:.3e})  rel-L2 {rel:.3e}")
    assert worst <= F32_GATE, f"{label}: product err/A {worst:.3e} > 2^-20"
    assert rel <= 2e-6, f"{label}: product rel-L2 {rel:.3e} > 2e-6"
  # 5. the GroupNorm output against the float64 GroupNorm (+SiLU) of the product as stored (every sample)
  gref64 = O.group_norm(prod.cpu().double(), gamma.double(), beta.double(), groups=GROUPS, eps=GN_EPS)
  if silu:
    gref64 = O.silu(gref64)
  k_sig = SHIFT[dt] if c.family == "shift" else 0.0
  check(label, gii[..., gsl], gref64, dt, k_sig, gamma.abs().max().item())
