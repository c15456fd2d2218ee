"""The plan ldm_gemm makes is what it was when tests/golden/gemm_plans.json was recorded (its "recorded_at_commit"):
ldm_gemm_plan, ldm_gemm_splits and ldm_gemm_workspace_bytes over the grid of tests/golden/record_gemm_plans.py -- both
dtypes x six launch forms x GEGLU or not x 7 M x 7 N x 5 K x forced tile 0..19 x split_k 0 / 1 / 4 x with and without a
workspace, and every key of the packaged plan tables -- about 700 000 host queries, no GPU.  Equality is exact: per group
the count of every distinct (tile, split) answer and a SHA-256 over all rows in sweep order.  A change that means to
alter the cost model, a tile rule or a packaged table re-records the file (the recorder's --rows dumps the rows of two
builds for diffing)."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _recorder():
  spec = importlib.util.spec_from_file_location("record_gemm_plans", os.path.join(HERE, "golden", "record_gemm_plans.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.fixture(scope="module")
def sweep():
  from ldm_tf2_amd import _lib
  rec = _recorder()
  return json.load(open(rec.GOLDEN)), rec.sweep(_lib.lib, _lib.GemmParams)


def test_the_grid_is_the_recorded_one(sweep):
  gold, now = sweep
  assert len(gold["recorded_at_commit"]) == 40
  assert set(now) == set(gold["groups"]) and len(now) == 2 * 6 * 2 + 1
  for name, g in now.items():
    assert g["rows"] == gold["groups"][name]["rows"], name
  assert sum(g["rows"] for g in now.values()) == gold["queries"] > 700000


def test_every_plan_is_the_recorded_one(sweep):
  gold, now = sweep
  for name, g in now.items():
    assert g["answers"] == gold["groups"][name]["answers"], name
    assert g["sha256"] == gold["groups"][name]["sha256"], name
