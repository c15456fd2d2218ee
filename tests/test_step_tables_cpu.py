"""Step tables and the table-weighted multistep sampler, host side: the defaults are
untouched, the tables against the restatement and the golden file, the weights, the solvers on the problem with a
known answer, the two C ABI entries, the ops and the CLI keys.  Nothing runs on a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

import deis_ref as D
import plms_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_tables.json")
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012)
HOST_TABLES = ("_betas", "_alphas_cumprod", "_ddim_steps", "_ddim_alphas_cumprod_prev", "_ddim_sigmas",
               "_ddim_sqrt_recip_alphas_cumprod", "_ddim_sqrt_recipm1_alphas_cumprod", "_sqrt_alphas_cumprod",
               "_sqrt_one_minus_alphas_cumprod")


class _FakeModel:
  device = torch.device("cpu")

  def __init__(self, **kwargs):
    self.kwargs = kwargs


def _sampler(**kw):
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), **dict(LDM, **kw))


AB = D.alphas_cumprod(**LDM)


# ---- the defaults ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 50, 200, 1000])
@pytest.mark.parametrize("eta", [0., 0.7])
def test_defaults_are_todays_tables_byte_for_byte(n, eta):
  """Without the new kwargs (and with step_spacing="uniform") every host table is what the constructor built before
  the kwarg existed: restated here line by line from that constructor."""
  a, b = _sampler(num_ddim_steps=n, eta=eta), _sampler(num_ddim_steps=n, eta=eta, step_spacing="uniform")
  assert a._step_spacing == b._step_spacing == "uniform" and a._sampler == "ddim"
  steps = np.arange(0, 1000, 1000 // n, dtype=np.int32)
  if n < 1000:
    steps = steps + 1
  ac = AB[steps]
  prev = np.concatenate([[AB[0]], AB[steps[:-1]]], axis=0)
  want = dict(_alphas_cumprod=AB, _ddim_steps=steps, _ddim_alphas_cumprod_prev=prev,
              _ddim_sigmas=eta * np.sqrt((1 - prev) / (1 - ac) * (1 - ac / prev)),
              _ddim_sqrt_recip_alphas_cumprod=np.sqrt(1. / AB)[steps],
              _ddim_sqrt_recipm1_alphas_cumprod=np.sqrt(1. / AB - 1)[steps],
              _sqrt_alphas_cumprod=np.sqrt(AB), _sqrt_one_minus_alphas_cumprod=np.sqrt(1. - AB))
  for name in HOST_TABLES:
    x, y = getattr(a, name), getattr(b, name)
    assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    if name in want:
      assert x.dtype == want[name].dtype and x.tobytes() == want[name].tobytes(), name
  assert a._ddim_steps.tolist() == D.uniform_table(n).tolist()


def test_reference_yaml_binds_unchanged(monkeypatch):
  from ldm_tf2_amd import run_ldm_sampler as R
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  for name in ("TransformerModel", "UNet", "AutoencoderKL", "AutoencoderVQ"):
    monkeypatch.setattr(R, name, _FakeModel)
  monkeypatch.setattr(R, "_load_weights", lambda path, what: None)
  assert "step_spacing" not in cfg["ldm_sampling"] and "sampler" not in cfg["ldm_sampling"]
  assert "step_spacing" not in cfg["ldm"] and "ddim_steps" not in cfg["ldm"]
  assert R.step_spacing_name(cfg) == "uniform" and R.sampler_name(cfg) == "ddim"
  s = R.build_from_config(cfg, device="cpu")
  assert s._step_spacing == "uniform" and s._sampler == "ddim"
  assert s._ddim_steps.tolist() == D.uniform_table(cfg["ldm"]["num_ddim_steps"], cfg["ldm"]["num_steps"]).tolist()


def test_cli_plumbs_both_keys(monkeypatch):
  from ldm_tf2_amd import run_ldm_sampler as R
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  for name in ("TransformerModel", "UNet", "AutoencoderKL", "AutoencoderVQ"):
    monkeypatch.setattr(R, name, _FakeModel)
  monkeypatch.setattr(R, "_load_weights", lambda path, what: None)
  n = cfg["ldm"]["num_ddim_steps"]
  ab = D.alphas_cumprod(cfg["ldm"]["num_steps"], cfg["ldm"]["beta_start"], cfg["ldm"]["beta_end"])
  cfg["ldm_sampling"]["sampler"] = "deis"
  cfg["ldm_sampling"]["step_spacing"] = "karras"
  assert R.sampler_name(cfg) == "deis" and R.step_spacing_name(cfg) == "karras"
  s = R.build_from_config(cfg, device="cpu")
  assert s._sampler == "deis" and s._step_spacing == "karras"
  assert s._ddim_steps.tolist() == D.step_table(ab, n, "karras").tolist()
  cfg["ldm_sampling"]["sampler"] = "plms"
  cfg["ldm_sampling"]["step_spacing"] = "logsnr"
  s = R.build_from_config(cfg, device="cpu")
  assert s._sampler == "plms" and s._ddim_steps.tolist() == D.step_table(ab, n, "logsnr").tolist()
  cfg["ldm_sampling"]["step_spacing"] = "cosine"
  with pytest.raises(ValueError, match="step_spacing"):
    R.build_from_config(cfg, device="cpu")
  cfg["ldm_sampling"]["step_spacing"] = "karras"
  cfg["ldm_sampling"]["sampler"] = "deis"
  cfg["ldm"]["eta"] = 0.5
  with pytest.raises(ValueError, match="eta"):
    R.build_from_config(cfg, device="cpu")


# ---- constructor ------------------------------------------------------------------------------------------
def test_constructor_switches_and_errors():
  from ldm_tf2_amd import model_runners as M
  assert M.STEP_SPACINGS == ("uniform", "logsnr", "karras") == D.SPACINGS
  assert "deis" in M.SAMPLERS and "plms" in M.SAMPLERS and "ddim" in M.SAMPLERS
  assert _sampler(num_ddim_steps=50, sampler="deis", step_spacing="karras")._sampler == "deis"
  with pytest.raises(ValueError, match="eta"):
    _sampler(num_ddim_steps=50, eta=1., sampler="deis")
  assert _sampler(num_ddim_steps=50, eta=1., step_spacing="logsnr")._eta == 1.        # ddim with eta on any table
  with pytest.raises(ValueError, match="step_spacing"):
    _sampler(num_ddim_steps=50, step_spacing="cosine")
  # a table handed in
  table = [1, 5, 30, 200, 700, 999]
  s = _sampler(num_ddim_steps=6, ddim_steps=table)
  assert s._ddim_steps.dtype == np.int32 and s._ddim_steps.tolist() == table
  s = _sampler(num_ddim_steps=6, ddim_steps=np.array(table, dtype=np.int64), sampler="deis")
  assert s._ddim_steps.tolist() == table
  for bad in ([1, 5, 5, 200, 700, 999], [1, 5, 30, 200, 999, 700], [0, 5, 30, 200, 700, 999],
              [1, 5, 30, 200, 700, 1000], [1, 5, 30, 200, 700], [1., 5., 30., 200., 700., 999.]):
    with pytest.raises(ValueError, match="ddim_steps"):
      _sampler(num_ddim_steps=6, ddim_steps=bad)
  with pytest.raises(ValueError, match="ddim_steps"):
    _sampler(num_ddim_steps=6, ddim_steps=table, step_spacing="karras")
  # a table of its own length: the N-divides-1000 rule is the uniform table's
  assert _sampler(num_ddim_steps=3, ddim_steps=[10, 500, 999])._ddim_steps.tolist() == [10, 500, 999]
  assert len(_sampler(num_ddim_steps=300, ddim_steps=list(range(1, 301)))._ddim_steps) == 300
  # the N-divides-1000 rule is unchanged on the spaced tables
  with pytest.raises(IndexError):
    _sampler(num_ddim_steps=300, step_spacing="logsnr")


# ---- tables -----------------------------------------------------------------------------------------------
def test_known_answers_of_the_table_rule():
  assert D.step_table(AB, 10, "logsnr").tolist() == [2, 8, 26, 73, 167, 313, 484, 646, 784, 901]
  t = D.step_table(AB, 50, "logsnr").tolist()
  assert t[:14] == list(range(1, 11)) + [13, 17, 21, 27] and t[-3:] == [938, 960, 981]
  assert _sampler(num_ddim_steps=10, step_spacing="logsnr")._ddim_steps.tolist() == D.step_table(AB, 10, "logsnr").tolist()


def test_golden_step_tables():
  with open(GOLDEN) as f:
    g = json.load(f)
  assert g["schedule"] == LDM and sorted(g["tables"]) == ["karras", "logsnr"]
  for spacing in ("logsnr", "karras"):
    assert sorted(int(n) for n in g["tables"][spacing]) == [8, 10, 20, 25, 50]
    for n, want in g["tables"][spacing].items():
      s = _sampler(num_ddim_steps=int(n), step_spacing=spacing)
      assert s._ddim_steps.dtype == np.int32 and s._ddim_steps.tolist() == want, (spacing, n)
      assert D.step_table(AB, int(n), spacing).tolist() == want, (spacing, n)


@pytest.mark.parametrize("spacing", ["logsnr", "karras"])
def test_every_divisor_gives_a_valid_table_and_derived_tables(spacing):
  for n in [n for n in range(4, 501) if 1000 % n == 0]:
    s = _sampler(num_ddim_steps=n, step_spacing=spacing, eta=0.5)
    t = s._ddim_steps
    top = int(D.uniform_table(n)[-1])
    assert len(t) == n and np.all(np.diff(t) > 0) and t[0] >= 1 and t[-1] == top, (n, t)
    assert t.tolist() == D.step_table(AB, n, spacing).tolist(), n
    ab, ab_prev = D.derived_tables(AB, t)
    assert np.array_equal(s._ddim_alphas_cumprod_prev, ab_prev) and s._ddim_alphas_cumprod_prev[0] == AB[0]
    assert np.array_equal(s._ddim_sqrt_recip_alphas_cumprod, np.sqrt(1. / AB)[t])
    assert np.array_equal(s._ddim_sqrt_recipm1_alphas_cumprod, np.sqrt(1. / AB - 1)[t])
    assert np.array_equal(s._ddim_sigmas, 0.5 * np.sqrt((1 - ab_prev) / (1 - ab) * (1 - ab / ab_prev)))
    assert np.all(np.isfinite(s._ddim_sigmas)) and np.all(s._ddim_sigmas > 0)


def test_img2img_start_and_progressive_slots_do_not_depend_on_the_table():
  from ldm_tf2_amd.model_runners import img2img_start
  for n in (10, 50):
    for strength in (0.3, 0.75, 1.0):
      assert img2img_start(strength, n) == int(strength * n)          # an index count, not a timestep


# ---- weights ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["uniform", "logsnr", "karras"])
@pytest.mark.parametrize("n", [8, 10, 20, 25, 50, 200])
def test_weight_table(n, spacing):
  """The product's table (16-point Gauss-Legendre) against the restatement's closed form and its 32-point
  quadrature, to 1e-12 of the row's largest weight; rows sum to 1; j = 0 is [1]."""
  s = _sampler(num_ddim_steps=n, step_spacing=spacing, sampler="deis")
  got = s.multistep_weights()
  closed = D.weight_table(AB, s._ddim_steps, D.weights_closed)
  gauss = D.weight_table(AB, s._ddim_steps, D.weights_gauss)
  assert got.shape == (n, 4, 4) and got.dtype == np.float64
  scale = np.maximum(np.abs(closed).max(axis=-1, keepdims=True), 1.)
  print(f"N={n} {spacing}: product - closed {np.abs((got - closed) / scale).max():.2e}, gauss32 - closed "
        f"{np.abs((gauss - closed) / scale).max():.2e}, largest sum |w| {np.abs(closed).sum(-1).max():.2f}")
  assert np.abs((got - closed) / scale).max() <= 1e-12
  assert np.abs((gauss - closed) / scale).max() <= 1e-12
  for i in range(n):
    for j in range(4):
      if i + j <= n - 1:
        assert abs(got[i, j].sum() - 1.) <= 1e-12 * scale[i, j, 0], (i, j)
        assert np.all(got[i, j, j + 1:] == 0.)
      else:
        assert np.all(got[i, j] == 0.)                                # no such history exists
    assert got[i, 0].tolist() == [1., 0., 0., 0.]


def test_weights_approach_the_adams_bashforth_constants():
  """Nodes exactly uniform in lambda, spacing h, the step again h: as h -> 0 the weight e^{-lambda} is flat over the
  step and the weights are the Adams-Bashforth ones, with a difference of order h."""
  from ldm_tf2_amd.model_runners import PLMS_WEIGHTS, deis_weights
  prev = None
  for h in (1e-1, 1e-2, 1e-3, 1e-4):
    worst = 0.
    for j in range(4):
      lams = -h * np.arange(j + 1)
      w = deis_weights(lams, h)
      assert np.abs(w - D.weights_closed(lams, h)).max() <= 1e-12
      assert abs(w.sum() - 1.) <= 1e-12
      worst = max(worst, float(np.abs(w - np.array(PLMS_WEIGHTS[j])).max()))
    print(f"h={h:g}: max |w - AB| = {worst:.3e}")
    assert worst <= h
    if prev is not None:
      assert worst <= prev / 5
    prev = worst
  assert deis_weights([0.3], 1.7).tolist() == [1.]
  with pytest.raises(ValueError):
    deis_weights([0.3, 0.1], 0.3)


# ---- the solvers on a problem with a known answer ------------------------------------------------------------
def _product_loop(s, x, start, name):
  """The loop through the product's host tables and weights, float64; eps = the exact eps of plms_ref's Gaussian
  mixture at abar[steps[i]].  name: "ddim" (order 0), "plms" (PLMS_WEIGHTS), "deis" (multistep_weights())."""
  from ldm_tf2_amd.model_runners import PLMS_WEIGHTS
  c1, c2, a_prev = s._ddim_sqrt_recip_alphas_cumprod, s._ddim_sqrt_recipm1_alphas_cumprod, s._ddim_alphas_cumprod_prev
  wtab = s.multistep_weights() if name == "deis" else None
  hist = []
  for i in range(start, -1, -1):
    hist.insert(0, P.mixture_eps(x, s._alphas_cumprod[s._ddim_steps[i]]))
    del hist[4:]
    j = 0 if name == "ddim" else min(start - i, 3)
    w = PLMS_WEIGHTS[j] if wtab is None else wtab[i, j, :j + 1]
    e = sum(wk * ek for wk, ek in zip(w, hist))
    x0 = c1[i] * x - c2[i] * e
    x = np.sqrt(a_prev[i]) * x0 + np.sqrt(1. - a_prev[i]) * e
  return x


_TRUTH = {}


def _truth(top, seed):
  """The loop on EVERY integer timestep from `top` down to 1, ending on abar[0] (tests/test_plms_cpu.py's truth)."""
  if (top, seed) not in _TRUTH:
    x_T = np.random.default_rng(seed).standard_normal(4096)
    _TRUTH[top, seed] = (x_T, P.plms_loop(lambda x, i: P.mixture_eps(x, AB[i + 1]), x_T, AB[1:top + 1], AB[0:top],
                                          top - 1))
  return _TRUTH[top, seed]


def _error(n, spacing, name, seed):
  s = _sampler(num_ddim_steps=n, step_spacing=spacing)
  x_T, truth = _truth(int(D.uniform_table(n)[-1]), seed)
  got = _product_loop(s, x_T, n - 1, name)
  st = D.step_table(AB, n, spacing)
  ab, ab_prev = D.derived_tables(AB, st)
  f = lambda x, i: P.mixture_eps(x, AB[st[i]])
  if name == "deis":
    ref = D.ms_loop(f, x_T, ab, ab_prev, n - 1, D.weight_table(AB, st))
  else:
    ref = P.plms_loop(f, x_T, ab, ab_prev, n - 1, max_order=0 if name == "ddim" else 3)
  assert np.allclose(got, ref, rtol=0, atol=1e-10), (n, spacing, name)
  return float(np.linalg.norm(got - truth) / np.linalg.norm(truth))


COLUMNS = (("ddim", "uniform"), ("plms", "uniform"), ("plms", "logsnr"), ("plms", "karras"), ("deis", "uniform"),
           ("deis", "logsnr"), ("deis", "karras"))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tables_and_weights_make_the_better_solver(seed):
  err = {}
  for n in (10, 20, 25, 50):
    for name, spacing in COLUMNS:
      err[n, name, spacing] = _error(n, spacing, name, seed)
    print(f"seed {seed} N={n}: " + "  ".join(f"{a}/{b} {err[n, a, b]:.2e}" for a, b in COLUMNS))
  err[200, "ddim", "uniform"] = _error(200, "uniform", "ddim", seed)
  print(f"seed {seed} N=200: ddim/uniform {err[200, 'ddim', 'uniform']:.2e}")
  assert err[10, "plms", "logsnr"] <= err[200, "ddim", "uniform"]
  assert err[25, "plms", "karras"] <= err[25, "plms", "uniform"] / 1.4
  assert err[25, "deis", "karras"] <= err[25, "plms", "uniform"] / 8
  assert err[50, "deis", "karras"] <= err[50, "plms", "uniform"] / 20


def test_first_step_of_a_loop_is_a_ddim_step():
  s = _sampler(num_ddim_steps=50, step_spacing="karras")
  x = np.random.default_rng(0).standard_normal(64)
  assert np.array_equal(_product_loop(s, x, 0, "deis"), _product_loop(s, x, 0, "ddim"))
  assert not np.array_equal(_product_loop(s, x, 1, "deis"), _product_loop(s, x, 1, "ddim"))
  assert not np.array_equal(_product_loop(s, x, 3, "deis"), _product_loop(s, x, 3, "plms"))


# ---- C ABI and ops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,count", [("ldm_cfg_ms_update", 23), ("ldm_cfg_ms_update_rng", 22)])
def test_header_lib_and_library_agree_on_the_entries(entry, count):
  from ldm_tf2_amd import _lib
  src = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

  def params(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"include/ldm_hip.h does not declare {name}"
    return [p.strip() for p in m.group(1).split(",")]
  ps = params(entry)
  res, args = _lib.SIGNATURES[entry]
  assert res is ctypes.c_int32 and len(args) == len(ps) == count
  for p, a in zip(ps, args):
    want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else
            ctypes.c_float if p.startswith("float") else ctypes.c_int32)
    assert a is want, (p, a)
  # the signature of the PLMS entry plus `const float* weights` and its row pitch, after `start`
  plms = params(entry.replace("_ms_", "_plms_"))
  k = plms.index("const int32_t* start") + 1
  assert ps == plms[:k] + ["const float* weights", "int64_t weights_pitch"] + plms[k:]
  assert getattr(ctypes.CDLL(_lib.LIB_PATH), entry) is not None


def test_ops_reject_host_tensors():
  from ldm_tf2_amd import ops
  z = torch.zeros(2, 4, 4, 4)
  i = torch.zeros(1, dtype=torch.int32)
  w = torch.zeros(10, 4, 4)
  with pytest.raises(ValueError):
    ops.cfg_ms_update(torch.zeros(4, 4, 4, 4), z, z.clone(), torch.zeros(4, 2, 4, 4, 4), torch.zeros(10, 4), i, i, w, 5.)
  with pytest.raises(ValueError):
    ops.cfg_ms_update_rng(torch.zeros(4, 4, 4, 4), z, z.clone(), torch.zeros(4, 2, 4, 4, 4), torch.zeros(10, 4), i, i,
                          w, torch.zeros(4, dtype=torch.int32), 5.)
  assert "cfg_ms_update" in ops.__all__ and "cfg_ms_update_rng" in ops.__all__
