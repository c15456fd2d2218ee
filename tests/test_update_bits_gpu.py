"""The output bits of the eight sampler update entries against tests/golden/update_bits.json, which
tools/update_bits.py recorded on an MI355X from a build of the commit named in the file (the one in front of the fold of
the update kernels into csrc/sampler.hip).  Every case recomputes one SHA-256 over xt_out, pred_x0_out, both halves of
x_unet_out and the ring slot written, and *index, with the library under test and asserts equality.

The device libm behind logf / sincospif and the compiler's contraction choices belong to the ROCm release, so the
hashes are comparable only under the recorded release: under another one the module skips.
"""
import json

import pytest

pytestmark = pytest.mark.gpu

from tools import update_bits as U  # noqa: E402

with open(U.FIXTURE) as _f:
  GOLD = json.load(_f)
CASES = U.cases()


@pytest.fixture(scope="module", autouse=True)
def _same_rocm():
  if U.rocm_version() != GOLD["rocm"]:
    pytest.skip(f"fixture recorded under ROCm {GOLD['rocm']}, this is {U.rocm_version()}: regenerate it with a build "
                f"of commit {GOLD['commit']} (LDM_HIP_LIB=<that library> python tools/update_bits.py --commit "
                f"{GOLD['commit']} --write)")


def test_fixture_covers_the_case_list():
  assert sorted(GOLD["cases"]) == sorted(n for n, _ in CASES)
  assert len(GOLD["commit"]) == 40


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_bits(dev, name, case):
  got = U.run_case(case, dev)
  want = GOLD["cases"][name]
  assert got == want, (got, want)
