"""Host query of the split-K GroupNorm's launch form (ldm_groupnorm_splitk_form, no GPU), and that the split-K
completion cases of tests/test_splitk_completion_gpu.py reach every form it can return at the U-Net's widths."""
import ctypes as C

import pytest

from ldm_tf2_amd._lib import BF16, F32, lib

import test_splitk_completion_gpu as SC

GROUPS = 32


def _form(B, HW, Cc, dtype, groups=GROUPS):
  f = (C.c_int32 * 4)(-7, -7, -7, -7)
  st = lib.ldm_groupnorm_splitk_form(B, HW, Cc, groups, dtype, f)
  return st, tuple(f)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_form_query_agrees_with_supported(dtype):
  esize = 4 if dtype == F32 else 2
  n = 0
  for Cc in (4, 32, 64, 128, 256, 320, 512, 640, 960, 1280, 1920, 2560, 100, 330):
    for B in (1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128):
      for HW in (1, 2, 4, 5, 12, 16, 25, 48, 49, 64, 96, 97, 100, 192, 193, 256, 400, 401, 408, 409, 816, 817,
                 1024, 1632, 1633, 2048, 4096):
        sup = lib.ldm_groupnorm_splitk_supported(B, HW, Cc, GROUPS, dtype)
        st, (GB, S, NT, MAXCH) = _form(B, HW, Cc, dtype)
        assert (st == 0) == (sup == 1), (B, HW, Cc, dtype, st, sup)
        if st != 0:
          assert (GB, S, NT, MAXCH) == (-7, -7, -7, -7)        # untouched
          continue
        n += 1
        cpg = Cc // GROUPS
        assert GROUPS % GB == 0 and S * 16 == GB * cpg * esize, (B, HW, Cc, GB, S)
        assert NT in (64, 256, 512) and MAXCH in (8, 16)
        assert (HW + NT // S - 1) // (NT // S) <= MAXCH            # every pixel has a chunk slot
        if NT == 64:
          assert B * (GROUPS // GB) >= 512
  assert n > 1000
  # bad arguments
  assert _form(16, 16, 1280, 5)[0] != 0
  assert _form(0, 16, 1280, dtype)[0] != 0
  assert _form(16, 16, 1282, dtype)[0] != 0
  assert _form(16, 16, 1280, dtype, groups=0)[0] != 0
  assert lib.ldm_groupnorm_splitk_form(16, 16, 1280, GROUPS, dtype, None) != 0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_completion_cases_cover_every_form(dtype):
  """Every form splitk_plan returns for C in {320, 640, 1280} (any B, HW) has a case in the GPU module, and every
  synthetic case there still reaches the form and the effective split it is named after."""
  dt = SC.F32 if dtype == F32 else SC.BF
  reachable = set()
  for Cc in (320, 640, 1280):
    for B in (1, 8, 15, 16, 31, 32, 63, 64, 65, 128):
      for HW in range(1, 2100):
        st, f = _form(B, HW, Cc, dtype)
        if st == 0:
          reachable.add((Cc, f))
  covered = {(c.C, c.form) for c in SC.CASES if c.dt == dt}
  assert reachable - covered == set(), sorted(reachable - covered)
  for c in SC.SYN:
    if c.dt == dt:
      assert SC.gn_form(c.B, c.H * c.W, c.C, c.dt) == c.form, SC.case_id(c)
      assert SC.eff_split(c) == c.split, SC.case_id(c)


def test_completion_cases_cover_split_residues():
  """Effective splits of every residue mod SU (4 on the one-wave form, 2 otherwise), and splits whose last slab
  has fewer K-tiles than the others, on both kinds of form."""
  for one_wave, need in ((True, {2, 3, 5, 6, 7, 8, 9, 12, 13}), (False, {2, 3, 5, 8, 16})):
    cases = [c for c in SC.CASES if (c.form[2] == 64) == one_wave]
    assert need <= {c.split for c in cases}, need - {c.split for c in cases}
    short = []
    for c in cases:
      p = SC._skeleton(c)
      kt = -(-p.K // (64 if c.dt == SC.BF else 32))
      if kt % -(-kt // c.split):
        short.append(c)
    assert short, "no case with a short last slab"
