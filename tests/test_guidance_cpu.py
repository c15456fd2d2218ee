"""Guidance schedules, host side: the table builder against the restatement on every step
table, the interval's edges, every rejected input, the YAML keys and the untouched default.  Nothing runs on a GPU."""
import os

import numpy as np
import pytest
import torch
import yaml

import deis_ref as D
import guidance_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012)
AB = D.alphas_cumprod(**LDM)
EXPLICIT = [3, 40, 41, 250, 600, 601, 900, 999]


class _FakeModel:
  device = torch.device("cpu")


def _sampler(**kw):
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), **dict(LDM, **kw))


def _tables():
  out = [(f"{sp}/{n}", D.step_table(AB, n, sp)) for sp in D.SPACINGS for n in (10, 50)]
  return out + [("explicit", np.array(EXPLICIT))]


@pytest.mark.parametrize("name,steps", _tables(), ids=[t[0] for t in _tables()])
def test_table_against_the_restatement(name, steps):
  from ldm_tf2_amd.model_runners import guidance_table
  n = len(steps)
  if name == "explicit":
    s = _sampler(num_ddim_steps=n, ddim_steps=EXPLICIT)
  else:
    s = _sampler(num_ddim_steps=n, step_spacing=name.split("/")[0])
  assert s._ddim_steps.tolist() == steps.tolist()
  ramp = np.linspace(7.5, 1.5, n)
  cases = [(5., None), (5., (int(steps[2]), int(steps[-3]))), (7.5, (0, 999)), (3., (0, 0)),
           (ramp, None), (1., None)]
  for scale, iv in cases:
    got = guidance_table(s._ddim_steps, scale, iv)
    want = G.table(steps, scale, iv)
    assert got.dtype == np.float32 and got.shape == (n,) and got.tobytes() == want.tobytes(), (name, scale, iv)
  # interval edges are inclusive, in timesteps
  lo, hi = int(steps[2]), int(steps[-3])
  g = guidance_table(steps, 5., (lo, hi))
  assert g[2] == 5. and g[-3] == 5. and g[1] == 1. and g[-2] == 1. and G.guided(g) == [2 <= i <= n - 3 for i in range(n)]
  g = guidance_table(steps, 5., (lo + 1, hi - 1))
  assert g[2] == 1. and g[-3] == 1. and g[3] == 5.
  # an interval that covers everything is the constant table; one that covers nothing is all ones
  assert np.array_equal(guidance_table(steps, 5., (int(steps[0]), int(steps[-1]))), np.full(n, 5., np.float32))
  assert np.array_equal(guidance_table(steps, 5., (0, 999)), guidance_table(steps, 5.))
  assert np.array_equal(guidance_table(steps, 5., (0, 0)), np.ones(n, np.float32))        # (every table starts at 1 or above)
  assert np.array_equal(guidance_table(steps, 5., (1000, 2000)), np.ones(n, np.float32))
  assert np.array_equal(guidance_table(steps, 5., (lo, lo)), np.where(steps == lo, 5., 1.).astype(np.float32))


def test_rejected_inputs():
  from ldm_tf2_amd.model_runners import guidance_table
  steps = D.step_table(AB, 10, "uniform")
  with pytest.raises(ValueError, match="guidance_scale has shape"):
    guidance_table(steps, [5.] * 9)
  with pytest.raises(ValueError, match="guidance_scale has shape"):
    guidance_table(steps, np.ones((2, 5)))
  for bad in (float("nan"), float("inf"), 1e39):
    with pytest.raises(ValueError, match="finite"):
      guidance_table(steps, [5.] * 9 + [bad])
    with pytest.raises(ValueError, match="finite"):
      guidance_table(steps, bad)
  with pytest.raises(ValueError, match="t_lo"):
    guidance_table(steps, 5., (600, 200))
  with pytest.raises(ValueError, match="sequence"):
    guidance_table(steps, [5.] * 10, (200, 600))
  with pytest.raises(ValueError, match="t_lo, t_hi"):
    guidance_table(steps, 5., (200, 400, 600))


@pytest.mark.parametrize("sampler", ["ddim", "plms", "deis"])
def test_a_schedule_needs_eta_zero_and_a_float_builds_no_table(sampler):
  s = _sampler(num_ddim_steps=10, sampler=sampler)
  assert s._skip_unguided is True
  assert s._guidance(5., None) is None and s._gtab is None          # today's path: nothing is constructed
  assert s._guidance(np.float32(5.), None) is None and s._gtab is None
  g = s._guidance(5., (200, 600))
  assert g.tolist() == G.table(s._ddim_steps, 5., (200, 600)).tolist()
  buf = s._gtab
  assert buf.dtype == torch.float32 and buf.tolist() == g.tolist()
  g2 = s._guidance(list(range(2, 12)), None)                        # new values, the same buffer
  assert s._gtab is buf and buf.tolist() == g2.tolist() == [float(v) for v in range(2, 12)]
  assert s._guidance(5., None) is None and s._gtab is buf
  assert _sampler(num_ddim_steps=10, skip_unguided=False)._skip_unguided is False
  if sampler != "ddim":
    return                                                          # (plms / deis reject eta > 0 themselves)
  e = _sampler(num_ddim_steps=10, eta=0.5)
  assert e._guidance(5., None) is None
  ids = np.zeros((4, 77), dtype=np.int64)
  for kw in (dict(guidance_scale=5., guidance_interval=(200, 600)), dict(guidance_scale=[5.] * 10)):
    with pytest.raises(ValueError, match="eta = 0"):
      e._guidance(kw["guidance_scale"], kw.get("guidance_interval"))
    with pytest.raises(ValueError, match="eta = 0"):
      e.ddim_p_sample_loop(ids, [2, 16, 16, 4], **kw)
    with pytest.raises(ValueError, match="eta = 0"):
      e.ddim_p_sample_loop_progressive(ids, [2, 16, 16, 4], **kw)
    with pytest.raises(ValueError, match="eta = 0"):
      e.ddim_p_sample_loop_img2img(ids, np.zeros((2, 128, 128, 3), np.float32), **kw)
  with pytest.raises(ValueError, match="guidance_scale has shape"):   # a wrong length is reported before eta
    e.ddim_p_sample_loop(ids, [2, 16, 16, 4], guidance_scale=[5.] * 3)


def test_yaml_keys_bind():
  from ldm_tf2_amd import run_ldm_sampler as R
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  ids = np.zeros((8, 77), dtype=np.int64)
  assert R.guidance_kwargs(cfg) == {}
  before = R.sampling_call(cfg, ids, 5)
  assert "guidance_interval" not in before[2]                       # the reference's YAML: the call is today's
  cfg = yaml.safe_load(yaml.safe_dump(dict(cfg, ldm_sampling=dict(cfg["ldm_sampling"], guidance_interval=[200, 600],
                                                                  guidance_scale=[7.5, 5.0, 2.5]))))
  method, args, kwargs = R.sampling_call(cfg, ids, 5)
  assert method == before[0] and kwargs["guidance_interval"] == (200, 600) and args[2] == [7.5, 5.0, 2.5]
  assert {k: v for k, v in kwargs.items() if k != "guidance_interval"} == before[2]
  cfg["ldm_sampling"]["sample_save_progress"] = not cfg["ldm_sampling"].get("sample_save_progress")
  assert R.sampling_call(cfg, ids, 5)[2]["guidance_interval"] == (200, 600)
  cfg["ldm_sampling"]["guidance_interval"] = [200]
  with pytest.raises(ValueError, match="guidance_interval"):
    R.sampling_call(cfg, ids, 5)


def test_the_new_entry_is_declared_bound_and_exported():
  import ctypes
  import re
  from ldm_tf2_amd import _lib, ops
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldm_hip.h")).read(), flags=re.S)
  m = re.search(r"\bint\s+ldm_cfg_sched_update\s*\(([^)]*)\)\s*;", src)
  ps = [p.strip() for p in m.group(1).split(",")]
  res, args = _lib.SIGNATURES["ldm_cfg_sched_update"]
  assert res is ctypes.c_int32 and len(args) == len(ps) == 25
  for p, a in zip(ps, args):
    want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int32)
    assert a is want, (p, a)
  assert "float guidance_scale" not in ps and "const float* gtab" in ps     # no scale argument: a table
  assert getattr(ctypes.CDLL(_lib.LIB_PATH), "ldm_cfg_sched_update") is not None
  assert "cfg_sched_update" in ops.__all__
  z, i = torch.zeros(2, 4, 4, 4), torch.zeros(1, dtype=torch.int32)
  with pytest.raises(ValueError):                                    # host tensors: no CPU fallback
    ops.cfg_sched_update(torch.zeros(4, 4, 4, 4), z, z.clone(), torch.zeros(10, 4), torch.ones(10), i, True)
