"""Every element of the row-panel kernels (ldm_ffn_geglu, ldm_st_tail, ldm_st_xtail, ldm_st_block) accounted for with
inputs whose correct output is known exactly (tests/ffn_probes.py: one phase of the chain at a time, everything else an
identity or a zero), at the panel edges (M = 1, 200, 256; one to three samples; the pair form), once with contiguous
operands and once with padded row pitches, NaN in the input pads and behind the pair form's half-height inputs, a
sentinel in out's pad columns and in two guard rows that must stay bit-identical.  The 128-row form of ldm_st_block runs
at the smallest M the dispatch sends there and is compared on the device.

Each case prints one `ACCT ffn ...` line per probe with its worst figure in units of the gate (<= 1 passes; the exact
probes pass only at 0)."""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import ffn_probes as Fp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


def run(dev, P, padded, on_device=False):
  """One launch: (out rows [M, C], guard rows and pad columns untouched)."""
  D = Fp.device_operands(P, dev, padded)
  before = D.out_buf.clone()
  Fp.launch(ops(), P, D)
  torch.cuda.synchronize()
  ok = Fp.untouched(before, D.out_buf, P.case.M)
  return (D.out if on_device else D.out.cpu()), ok


@pytest.mark.parametrize("c", Fp.cases(), ids=Fp.case_id)
def test_row_panel_accounting(dev, c):
  failed = []
  for probe in Fp.probes_of(c):
    worst, where = 0.0, ""
    for tag, P, gate in Fp.PROBES[probe](c):
      ref, info = Fp.ref64(P, rnd=gate != "gelu")
      for padded in (False, True):
        got, clean = run(dev, P, padded)
        f, ok = Fp.judge(gate, got, ref, info, P, c)
        view = "padded" if padded else "contig"
        if not clean:
          failed.append(f"{probe} {tag} {view}: a pad column or a guard row of out was written")
        if not ok:
          bad = (got.to(Fp.F64) - ref).abs()
          r, n = divmod(int(torch.nan_to_num(bad, nan=float("inf")).argmax()), Fp.C)
          failed.append(f"{probe} {tag} {view}: {f:.3f} at row {r} column {n}: got {float(got[r, n])}, ref {float(ref[r, n])}")
        if f >= worst:
          worst, where = f, f"{tag}-{view}"
    print(f"ACCT ffn {Fp.case_id(c)} {probe} {worst:.4f} ({where})")
  assert not failed, f"{Fp.case_id(c)}: {'; '.join(failed[:8])} ({len(failed)} in all)"


@pytest.mark.parametrize("c", Fp.big_cases(), ids=Fp.case_id)
def test_st_block_128_row_form(dev, c):
  """M = 192 panels: the 128-row FRONT instance (what the benchmark's 32x32 level runs).  Five launches in all over the two
  cases; the reference runs in float64 on the device and only the figures come back."""
  src = open(os.path.join(ROOT, "ldm_tf2_amd", "csrc", "ffn.hip")).read()
  assert re.findall(r"if \(\(M \+ 127\) / 128 >= (\d+)\)", src) == [str(Fp.SWITCH_PANELS)], "the dispatch was retuned"
  assert c.M // 128 == Fp.SWITCH_PANELS
  pair = c.in_rows != c.M
  failed = []
  for i, probe in enumerate(Fp.BIG_PROBES[pair]):
    tag, P, gate = Fp.PROBES[probe](c)[0]
    padded = pair or i % 2 == 1
    got, clean = run(dev, P, padded, on_device=True)
    ref, info = Fp.ref64(Fp.to_device(P, dev))
    f, ok = Fp.judge(gate, got, ref, info, P, c)
    print(f"ACCT ffn {Fp.case_id(c)} {probe} {f:.4f} ({tag}-{'padded' if padded else 'contig'})")
    if not clean:
      failed.append(f"{probe}: a pad column or a guard row of out was written")
    if not ok:
      bad = torch.nan_to_num((got.to(Fp.F64) - ref).abs(), nan=float("inf"))
      r, n = divmod(int(bad.argmax()), Fp.C)
      failed.append(f"{probe} {tag}: {f:.3f}, {int((bad > 0).sum())} elements differ, worst at row {r} column {n}")
  assert not failed, f"{Fp.case_id(c)}: {'; '.join(failed)}"
