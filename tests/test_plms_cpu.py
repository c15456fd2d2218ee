"""PLMS sampler, host side: the C ABI entry, the constructor switch, the CLI key, the
Adams-Bashforth weights, and the solver itself on a problem with a known answer.  Nothing runs on a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import plms_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012)


class _FakeModel:
  device = torch.device("cpu")

  def __init__(self, **kwargs):
    self.kwargs = kwargs


def _sampler(**kw):
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), **dict(LDM, **kw))


# ---- C ABI --------------------------------------------------------------------------------------------
def test_header_lib_and_library_agree_on_the_entry():
  from ldm_tf2_amd import _lib
  src = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
  m = re.search(r"\bint\s+ldm_cfg_plms_update\s*\(([^)]*)\)\s*;", src)
  assert m, "include/ldm_hip.h does not declare ldm_cfg_plms_update"
  params = [p.strip() for p in m.group(1).split(",")]
  res, args = _lib.SIGNATURES["ldm_cfg_plms_update"]
  assert res is ctypes.c_int32 and len(args) == len(params) == 21
  for p, a in zip(params, args):                      # pointers, 64-bit and 32-bit integers, the one float
    want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else
            ctypes.c_float if p.startswith("float") else ctypes.c_int32)
    assert a is want, (p, a)
  assert getattr(ctypes.CDLL(_lib.LIB_PATH), "ldm_cfg_plms_update") is not None


def test_op_rejects_host_tensors():
  from ldm_tf2_amd import ops
  z = torch.zeros(2, 4, 4, 4)
  i = torch.zeros(1, dtype=torch.int32)
  with pytest.raises(ValueError):
    ops.cfg_plms_update(torch.zeros(4, 4, 4, 4), z, z.clone(), torch.zeros(4, 2, 4, 4, 4), torch.zeros(10, 4), i, i, 5.)


# ---- constructor --------------------------------------------------------------------------------------
def test_constructor_switch():
  from ldm_tf2_amd import model_runners as M
  assert _sampler(num_ddim_steps=50)._sampler == "ddim"
  assert _sampler(num_ddim_steps=50, sampler="ddim")._sampler == "ddim"
  s = _sampler(num_ddim_steps=50, eta=0., sampler="plms")
  assert s._sampler == "plms" and s._graph is None
  with pytest.raises(ValueError, match="eta"):
    _sampler(num_ddim_steps=50, eta=1., sampler="plms")
  with pytest.raises(ValueError, match="sampler"):
    _sampler(num_ddim_steps=50, sampler="nope")
  assert "plms" in M.SAMPLERS and "ddim" in M.SAMPLERS
  assert "DDIM" in M.LatentDiffusionModelSampler.ddim_sample.__doc__ and "plms" in M.LatentDiffusionModelSampler.ddim_sample.__doc__


# ---- CLI ----------------------------------------------------------------------------------------------
def test_cli_plumbs_the_sampler_key(monkeypatch):
  from ldm_tf2_amd import run_ldm_sampler as R
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  for name in ("TransformerModel", "UNet", "AutoencoderKL", "AutoencoderVQ"):
    monkeypatch.setattr(R, name, _FakeModel)
  monkeypatch.setattr(R, "_load_weights", lambda path, what: None)
  ids = np.zeros((8, 77), dtype=np.int64)
  assert "sampler" not in cfg["ldm_sampling"]                      # the reference's YAML, unchanged
  assert R.sampler_name(cfg) == "ddim"
  assert R.build_from_config(cfg, device="cpu")._sampler == "ddim"
  call = R.sampling_call(cfg, ids, 5)
  cfg["ldm_sampling"]["sampler"] = "plms"
  assert R.sampler_name(cfg) == "plms"
  s = R.build_from_config(cfg, device="cpu")
  assert s._sampler == "plms" and s._num_ddim_steps == cfg["ldm"]["num_ddim_steps"]
  got = R.sampling_call(cfg, ids, 5)                               # the call itself does not depend on the solver
  assert got[0] == call[0] == "ddim_p_sample_loop" and got[2] == call[2]
  cfg["ldm_sampling"]["sampler"] = "euler"
  with pytest.raises(ValueError, match="sampler"):
    R.build_from_config(cfg, device="cpu")
  cfg["ldm_sampling"]["sampler"] = "plms"
  cfg["ldm"]["eta"] = 0.5
  with pytest.raises(ValueError, match="eta"):
    R.build_from_config(cfg, device="cpu")


# ---- weights ------------------------------------------------------------------------------------------
def test_plms_weights():
  from ldm_tf2_amd.model_runners import PLMS_WEIGHTS
  want = [[1.], [3 / 2, -1 / 2], [23 / 12, -16 / 12, 5 / 12], [55 / 24, -59 / 24, 37 / 24, -9 / 24]]
  assert len(PLMS_WEIGHTS) == len(P.WEIGHTS) == 4
  for j, row in enumerate(want):
    assert list(PLMS_WEIGHTS[j]) == row == list(P.WEIGHTS[j])
    assert abs(sum(row) - 1.) < 1e-15
    assert abs(sum(abs(w) for w in row) - P.ABS_WEIGHT_SUMS[j]) < 1e-15
  # the exact eps of the mixture integrates to the score of a single Gaussian when there is one component
  x = np.linspace(-3, 3, 7)
  one = P.mixture_eps(x, 1e-12)                                    # abar -> 0: p_t = N(0, 1), eps* = x
  assert np.allclose(one, x, atol=1e-5)


# ---- the specified solver is the better solver on a problem with a known answer --------------------------
def _product_loop(s, x, start, max_order):
  """The loop of DESIGN.md section 8 through the product's host tables and PLMS_WEIGHTS, float64; eps = the exact
  eps of plms_ref's Gaussian mixture at abar[steps[i]]."""
  from ldm_tf2_amd.model_runners import PLMS_WEIGHTS
  c1, c2, a_prev = s._ddim_sqrt_recip_alphas_cumprod, s._ddim_sqrt_recipm1_alphas_cumprod, s._ddim_alphas_cumprod_prev
  hist = []
  for i in range(start, -1, -1):
    hist.insert(0, P.mixture_eps(x, s._alphas_cumprod[s._ddim_steps[i]]))
    del hist[4:]
    w = PLMS_WEIGHTS[min(start - i, max_order)]
    e = sum(wk * ek for wk, ek in zip(w, hist))
    x0 = c1[i] * x - c2[i] * e
    x = np.sqrt(a_prev[i]) * x0 + np.sqrt(1. - a_prev[i]) * e
  return x


_TRUTH = {}


def _truth(s, seed):
  """plms_loop on EVERY integer timestep from steps[N-1] down to 1, ending on abar[0]: the interval and endpoint
  of the N-step run.  (N = 20, 25, 50 and 200 start at 951, 961, 981 and 996.)"""
  top = int(s._ddim_steps[-1])
  if (top, seed) not in _TRUTH:
    ac = s._alphas_cumprod
    x_T = np.random.default_rng(seed).standard_normal(4096)
    _TRUTH[top, seed] = (x_T, P.plms_loop(lambda x, i: P.mixture_eps(x, ac[i + 1]), x_T, ac[1:top + 1], ac[0:top],
                                          top - 1))
  return _TRUTH[top, seed]


def _errors(n, seed):
  s = _sampler(num_ddim_steps=n)
  x_T, truth = _truth(s, seed)
  out = {}
  for name, order in (("ddim", 0), ("plms", 3)):
    got = _product_loop(s, x_T, n - 1, order)
    # the product tables and the restatement give the same loop
    ref = P.plms_loop(lambda x, i: P.mixture_eps(x, s._alphas_cumprod[s._ddim_steps[i]]), x_T,
                      s._alphas_cumprod[s._ddim_steps], s._ddim_alphas_cumprod_prev, n - 1, max_order=order)
    assert np.allclose(got, ref, rtol=0, atol=1e-10)
    out[name] = float(np.linalg.norm(got - truth) / np.linalg.norm(truth))
  return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plms_is_the_better_solver_on_the_gaussian_mixture(seed):
  err = {n: _errors(n, seed) for n in (20, 25, 50, 200)}
  for n in (20, 25, 50, 200):
    print(f"seed {seed} N={n}: ddim {err[n]['ddim']:.3e} plms {err[n]['plms']:.3e} "
          f"ratio {err[n]['ddim'] / err[n]['plms']:.2f}")
  for n in (20, 25, 50):
    assert err[n]["plms"] <= err[n]["ddim"] / 4, (n, err[n])
  assert err[50]["plms"] <= err[200]["ddim"], (err[50], err[200])


def test_one_step_loop_is_a_ddim_step():
  s = _sampler(num_ddim_steps=50)
  x = np.random.default_rng(0).standard_normal(64)
  assert np.array_equal(_product_loop(s, x, 0, 3), _product_loop(s, x, 0, 0))
  assert not np.array_equal(_product_loop(s, x, 1, 3), _product_loop(s, x, 1, 0))
