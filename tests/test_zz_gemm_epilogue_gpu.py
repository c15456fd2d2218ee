"""Every activation epilogue of ldm_gemm -- act(alpha sum + bias + addend) + residual, written out in five places -- on
every store path, with probe data whose pre-activation value z is known exactly (tests/gemm_probes.py, "activation
epilogues": z is a multiple of 2^-4 with |z| <= 4, so that one 2^-4 step moves GELU or SiLU by at least 3.4e-5).

Store paths: the LDS-staged vector epilogue (an aligned view), the generic epilogue (output 8 bytes behind a 16-byte
boundary; row pitch + 4; a bias slice that is not 16-byte aligned), both reduce kernels (forced split_k = 2, aligned and
off by 8 bytes), the deferred reduce + ops.finish, the transposed store, one 3x3 convolution, the persistent tiles in both
deals with and without the LayerNorm fold.  Every operand is a view of a NaN-filled buffer and every output buffer must
still be NaN outside the stored [M, N or N / 2] region.  The (tile, split) plan is asserted through the spy.

A case passes when
  (a) uniformity, exact: within the launch, outputs with the same z (GEGLU: the same value and gate) and the same
      residual hold the same bits;
  (b) ceiling, float32 output, GELU / SiLU: |out - ref64| <= 2e-6 (A&S 7.1.26: 1.5e-7 on erf, 3e-7 at |z| = 4; the
      hardware exp2 and rcp at 1 ulp each; the output's own rounding);
  (c) ceiling, float32 output, GEGLU: |value| 2e-6 + 2^-23 |ref|;
  (d) ceiling, bf16 output: (b) or (c) plus 2^-8 |ref|;
  (e) gate, measured: figure = max |out - ref64| / max(max |oracle - ref64|, u max |ref64|) <= GATES[activation, output
      type]; oracle = oracle.ldm_oracle's gelu / silu in float32 on the same exact z, rounded to the output type; u the
      unit roundoff of the output type (small_probes.u_of).  A gate is twice the largest figure of the first MI355X run,
      rounded up to one significant digit.
A case marked `rej` must raise LdmHipError with the named message and leave its output buffer NaN.

RESULTS of the first run on an MI355X (422 cases, 6.4 s)
  activation, output type: cases, the largest figure, its gate, the largest share of the ceiling used
    gelu   f32     109    figure 2.0766   gate 5    share 0.163
    gelu   bf16     52    figure 0.6938   gate 2    share 0.958
    silu   f32     110    figure 1.0000   gate 2    share 0.122
    silu   bf16     53    figure 0.7380   gate 2    share 0.994
    geglu  f32      45    figure 1.1515   gate 3    share 0.251
    geglu  bf16     24    figure 0.6631   gate 2    share 0.991
  (the bf16 shares are the output's own rounding: 2^-8 |ref| is reached where a value lies just above a power of two.)
  All 398 cases that run were uniform and within their ceiling on every store path, the generic epilogue and the scalar
  reduce included, which no test had run with an activation before.
  Cross-path bit equality (printed as XPATH, not a gate): the float32 outputs of the store paths of one group were
  bit-identical in all 170 comparisons (72 GELU, 71 SiLU, 27 GEGLU): vector epilogue = generic epilogue = both reduces.
  The two findings, as the run reported them before the host fixes (the cases now expect the rejection instead):
    1. GEGLU, forced tile 11 / 12, unsplit, output off the vector epilogue (8 bytes off; row pitch + 4; bias slice 4 bytes
       off): ldm_gemm returned LDM_OK and all six outputs met the mutation `nothing_stored` (the NaN fill was intact).
    2. GEGLU + addend: the vector epilogue (tiles 0, 1, 2, 5, 11, 12, 19; float32 output) met `geglu_gate_addend_missing`
       and missed the header's formula, the generic epilogue, both reduces and the deferred reduce met the formula: the
       answer depended on alignment and split count.  ldm_gemm and ldm_gemm_reduce now reject the combination.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_probes as G  # noqa: E402
from small_probes import u_of  # noqa: E402
from test_gemm_accounting_gpu import F32, F64, ops, run, spy  # noqa: E402,F401

# twice the largest figure of the first MI355X run per (activation, output type), rounded up to one significant digit
GATES = {
    ("gelu", "f32"): 5.0, ("gelu", "bf16"): 2.0,
    ("silu", "f32"): 2.0, ("silu", "bf16"): 2.0,
    ("geglu", "f32"): 3.0, ("geglu", "bf16"): 2.0,
}
_FIRST_F32 = {}                                   # group -> (id, float32 output of the group's first store path)


def _oracle():
  from oracle import ldm_oracle as O
  return O


def _expect_rejection(dev, spy, c, d):
  from ldm_tf2_amd._lib import LdmHipError
  hold = []
  try:
    got = run(dev, c, d, hold)
  except LdmHipError as e:
    import re
    assert re.search(c.rej, str(e)), (G.epi_id(c), str(e))
    torch.cuda.synchronize()
    assert len(spy) == 0 and hold and bool(torch.isnan(hold[0][1]).all()), "a rejected call launched something"
    print(f"EPI {G.epi_id(c)} rejected: {e}")
    return
  matches = G.matching_mutations(c, d, got)
  right = not bool(G.exceeds(got, G.reference_act(c, d), G.ceiling(c, d)).any())
  pytest.fail(f"{G.epi_id(c)}: expected a rejection ({c.rej}); the launch ran (plan {spy}) and its output "
              f"{'meets' if right else 'MISSES'} the header's formula; mutations it meets: {matches}")


@pytest.mark.parametrize("c", G.epilogue_cases(), ids=G.epi_id)
def test_gemm_epilogue(dev, spy, c):
  f = G.FORMS[c.form]
  d = G.probe_epilogue(c)
  if c.rej:
    _expect_rejection(dev, spy, c, d)
    return
  got = run(dev, c, d)
  assert len(spy) == 1
  tile, _, slabs = spy[0]
  if f.tile:
    assert tile == f.tile and slabs == G.expected_slabs(c), (G.epi_id(c), spy[0])
  ref, ce = G.reference_act(c, d), G.ceiling(c, d)
  odn = "bf16" if c.odt == G.BF else "f32"
  err = torch.where(torch.isfinite(got), (got - ref).abs(), torch.full_like(ref, float("inf")))
  oerr = max(float((G.oracle_act(c, d, _oracle()) - ref).abs().max()), u_of(c.odt) * float(ref.abs().max()))
  figure = float(err.max()) / oerr
  share = float(torch.where(err > 0, err / ce, torch.zeros_like(err)).max())
  split_groups = G.not_uniform(got, G.uniformity_groups(c, d))
  over = G.exceeds(got, ref, ce)
  failed = []
  if split_groups:
    failed.append(f"uniformity: {split_groups} groups of equal (z, residual) hold different bits")
  if bool(over.any()):
    bt, m, n = [int(v) for v in over.nonzero()[0]]
    failed.append(f"ceiling: {int(over.sum())} of {over.numel()} elements; first at (m, n) = ({m}, {n}): got "
                  f"{float(got[bt, m, n])!r}, want {float(ref[bt, m, n])!r}, ceiling {float(ce[bt, m, n]):.3g}; "
                  f"mutations the output meets: {G.matching_mutations(c, d, got)}")
  if figure > GATES[(c.act, odn)]:
    failed.append(f"gate: figure {figure:.3f} above {GATES[(c.act, odn)]}")
  xpath = ""
  if c.odt == F32:
    key = G.epi_group(c)
    if key in _FIRST_F32:
      first_id, first = _FIRST_F32[key]
      ndiff = int((got.to(F32).view(torch.int32) != first.view(torch.int32)).sum())
      xpath = f" XPATH vs {first_id}: " + ("bit-identical" if ndiff == 0 else f"{ndiff} of {got.numel()} differ")
    else:
      _FIRST_F32[key] = (G.epi_id(c), got.to(F32))
  print(f"EPI {G.epi_id(c)} plan {spy[0]} act {c.act} out {odn} figure {figure:.4f} share-of-ceiling {share:.4f} "
        f"{'FAILED' if failed else 'ok'}{xpath}")
  assert not failed, G.epi_id(c) + "\n" + "\n".join(failed)
