"""Every key and every query row of every attention form accounted for, with inputs whose correct output is known exactly
(tests/attn_probes.py: key census, key selection, powers of two, and a per-element float64 bound on random data).

Forms: attn_kernel<Sp, KT> (float32 and bf16, Sp = 32 .. 160), its 8-wave two-tiles-in-flight form, the matrix-side
softmax (4 and 8 waves), attn_wide_kernel (Sp = 512), all through ops.attention; the in-panel cross-attention of
ldm_st_xtail / ldm_st_block through an identity harness: r0 = r1 = 0, all biases 0, w1 = w2 = 0 (GEGLU(0, 0) = 0),
Wp = I and Wo the 320 x 384 selector that drops each head's 8 padded dims, so that out = bf16(att) exactly.

Sizes sit on each form's own tile edges (A.cases); operands are views with NaN pad rows / columns, distinct batch strides,
q | k as halves of one buffer, out as a column slice.  Each case prints its figures in units of the gate (<= 1 passes).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_probes as A  # noqa: E402
from ldm_tf2_amd import layout as L  # noqa: E402

BF = torch.bfloat16
C_, K0_, H_, S_, SP_ = 320, 384, 8, 40, 48


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


_HARNESS = {}


def harness(dev):
  """The identity panel: (wo, zero [C], w1, aux, w2, wp)."""
  if dev not in _HARNESS:
    wo = torch.zeros(C_, K0_)
    for h in range(H_):
      for s in range(S_):
        wo[S_ * h + s, SP_ * h + s] = 1.0
    z = lambda *shape: torch.zeros(*shape, dtype=BF, device=dev)
    aux = L.ffn_aux(torch.zeros(8 * C_), torch.zeros(8 * C_)).to(dev)
    _HARNESS[dev] = (wo.to(BF).to(dev), torch.zeros(C_, device=dev), z(8 * C_, C_), aux, z(C_, 4 * C_),
                     torch.eye(C_).to(BF).to(dev))
  return _HARNESS[dev]


def run(dev, form, c, q, k, v):
  """The kernel's output on (q, k, v) as float64 [R, Tq, H, S]; padded dims must be exact zeros, columns of a wider
  out buffer must stay NaN."""
  o = ops()
  qd, kd, vt, out, ob = A.pack(form, c, q, k, v, dev)
  if form.kind == "xtail":
    wo, zero, w1, aux, w2, wp = harness(dev)
    M = c.R * c.Tq
    r = torch.zeros(M, C_, dtype=BF, device=dev)
    res = torch.full((M, C_), float("nan"), dtype=BF, device=dev)
    o.st_xtail(qd.contiguous(), kd.contiguous(), vt, wo, zero, r, w1, aux, w2, zero, wp, zero, r, res, 1e-5)
    torch.cuda.synchronize()
    return res.cpu().to(A.F64).reshape(c.R, c.Tq, H_, S_)
  o.attention(qd, kd, vt, out, c.H, form.Sp, form.S ** -0.5, matrix_softmax=form.kind == "ms")
  torch.cuda.synchronize()
  got, pad, rest = A.unpack(form, c, out, ob)
  assert pad.numel() == 0 or float(pad.abs().max()) == 0.0, "padded head dims must be exact zeros"
  assert rest is None or torch.isnan(rest).all(), "columns outside the out slice were written"
  return got


def test_layout_constants():
  assert L.MS_DIM == A.MS_DIM and abs(L.MS_LOG2E - 1.0 / A.LN2) < 1e-15
  assert tuple(sp for sp, _ in A._HEADS) == tuple(L.ATTN_SP)


@pytest.mark.parametrize("c", A.all_cases(), ids=A.case_id)
def test_attention_accounting(dev, c):
  form = A.FORMS[c.form]
  figures, failed = [], []

  def judge(probe, excess):
    figures.append(f"{probe} {excess:.3f}")
    print(f"ACCT {c.form} {probe} {excess:.4f} {A.case_id(c)}")
    if not excess <= 1.0:
      failed.append(probe)

  sc, base = A.scale_base(form, 1)
  q, k, v = A.probe_census(form, c)
  ref, _ = A.attn_ref64(q, k, v, sc, base)
  judge("census", A.census_excess(run(dev, form, c, q, k, v), ref, form.dtype))

  q, k, v, _ = A.probe_selection(form, c)
  ref, _ = A.attn_ref64(q, k, v, sc, base)
  judge("selection", A.selection_excess(run(dev, form, c, q, k, v), ref, form.dtype))

  if form.kind in ("ms", "xtail"):
    q, k, v, _, _ = A.probe_pow2(form, c)
    ref, _ = A.attn_ref64(q, k, v, sc, base)
    judge("pow2", A.selection_excess(run(dev, form, c, q, k, v), ref, form.dtype))

  for variant in A.P4_VARIANTS:
    q, k, v = A.probe_random(form, c, variant)
    ref, absref = A.attn_ref64(q, k, v, sc, base)
    judge(f"bound-{variant}", A.bound_excess(run(dev, form, c, q, k, v), ref, absref, form.dtype, variant))

  assert not failed, f"{A.case_id(c)}: over the gate (units of the gate, <= 1 passes): {', '.join(figures)}"


@pytest.mark.parametrize("T", [128, 384])
@pytest.mark.parametrize("pair", [False, True], ids=["plain", "cfg-pair"])
def test_st_block_key_census(dev, T, pair):
  """ldm_st_block with att = 0, r0 = r1 = 0, bo1 = 0 (h1 = 0), wq = qcs = qb = 0 (q = 0) and the identity harness behind
  the attention: out = count_d / Tk of each sample's OWN context.  cfg-pair: the inputs hold half the rows, the two
  halves of the output meet contexts whose census is rotated differently."""
  o = ops()
  form = A.FORMS["xtail-bf16"]
  wo, zero, w1, aux, w2, wp = harness(dev)
  worst = 0.0
  for Tk, ldx in ((1, 0), (5, 8), (16, 0), (17, 8), (64, 0), (77, 0), (77, 8), (80, 0), (80, 8)):
    R = 2 if pair else 3
    c = A.Case(form.name, T, Tk, R, H_, ldx, False, False)
    q, k, v = A.probe_census(form, c)
    ref, _ = A.attn_ref64(q, k, v, 1.0, 2)
    if pair:
      assert not torch.equal(ref[0], ref[1]) or Tk % S_ == 0
    _, kd, vt, _, _ = A.pack(form, c, q, k, v, dev)
    Rin = R // 2 if pair else R
    att = torch.zeros(Rin, T, K0_, dtype=BF, device=dev)
    r = torch.zeros(Rin * T, C_, dtype=BF, device=dev)
    z = lambda *shape: torch.zeros(*shape, dtype=BF, device=dev)
    qcs = torch.zeros(K0_, device=dev)
    out = torch.full((R * T, C_), float("nan"), dtype=BF, device=dev)
    o.st_block(att, z(C_, K0_), zero, r, z(K0_, C_), qcs, qcs, kd.contiguous(), vt, wo, zero, w1, aux, w2, zero, wp, zero,
               r, out, 1e-5)
    torch.cuda.synchronize()
    got = out.cpu().to(A.F64).reshape(R, T, H_, S_)
    x = A.census_excess(got, ref, BF)
    print(f"ACCT st_block{'-pair' if pair else ''} census {x:.4f} T={T} Tk={Tk} ldv={vt.shape[2]}")
    worst = max(worst, x)
  assert worst <= 1.0, f"st_block census: an element is {worst:.2f} bf16 ulp from count_d / Tk"
