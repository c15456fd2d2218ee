"""The output bits of one U-Net evaluation per launch form against tests/golden/unet_form_bits.json, which
tools/unet_form_bits.py recorded on an MI355X with the host walk of the commit named in the file (the one in front of
the form picker, ldm_tf2_amd/st_form.py) over the library of this source.  Every case -- the 25 of
test_zz_block_parity_gpu.CASES and the 9 of test_unet_calls_gpu.CASES, 16x16 latents with R = 4 -- rebuilds its
model, evaluates it with the tree under test and asserts the SHA-256 of the output's bytes.

The kernels' rounding belongs to the compiler of the ROCm release, so the hashes are comparable only under the
recorded release: under another one the module skips.
"""
import json

import pytest

pytestmark = pytest.mark.gpu

from tools import unet_form_bits as U  # noqa: E402

with open(U.FIXTURE) as _f:
  GOLD = json.load(_f)
CASES = U.cases()


@pytest.fixture(scope="module", autouse=True)
def _same_rocm():
  if U.rocm_version() != GOLD["rocm"]:
    pytest.skip(f"fixture recorded under ROCm {GOLD['rocm']}, this is {U.rocm_version()}: regenerate it from a "
                f"checkout of commit {GOLD['commit']} (LDM_HIP_LIB=<library under test> python "
                f"tools/unet_form_bits.py --tree <checkout> --commit {GOLD['commit']} --write)")


def test_fixture_covers_the_case_list():
  import test_unet_calls_gpu as TC
  import test_zz_block_parity_gpu as TP
  assert sorted(GOLD["cases"]) == sorted(n for n, _ in CASES) and len(CASES) == len(TP.CASES) + len(TC.CASES) == 25 + 9
  assert len(GOLD["commit"]) == 40


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_bits(dev, name, case):
  got = U.run_case(case, dev)
  assert got == GOLD["cases"][name], (got, GOLD["cases"][name])
