"""DDIM inversion host rules: the restatement undoes the sampling step, the level table, the new
entry's declarations and the CLI's call.  Host-only: nothing runs on a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import inversion_ref as I
from ldm_tf2_amd import _lib, ops
from ldm_tf2_amd import run_ldm_sampler as R
from ldm_tf2_amd.model_runners import LatentDiffusionModel, LatentDiffusionModelSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012, v_posterior=0., scale_factor=0.18215, eta=0.,
           num_ddim_steps=10)
SPACINGS = ("uniform", "logsnr", "karras")


@pytest.mark.parametrize("spacing", SPACINGS)
def test_inversion_undoes_the_sampling_step_in_float64(spacing):
  m = LatentDiffusionModel(None, None, None, step_spacing=spacing, **LDM)
  ac, steps = m._alphas_cumprod, m._ddim_steps
  tab = dict(c1=np.sqrt(1. / ac)[steps], c2=np.sqrt(1. / ac - 1.)[steps], a_prev=ac[I.t_in(steps)])
  g = np.random.default_rng(3)
  x, e_u, e_c = (g.standard_normal((2, 8, 8, 4)) for _ in range(3))
  for i in range(len(steps)):
    for gs in (1., 5.):
      up, x0 = I.invert_update(x, e_u, e_c, gs, i, tab)
      back, x0_f = I.forward_update(up, I.guided(e_u, e_c, gs), i, tab)
      r = np.linalg.norm(back - x) / np.linalg.norm(x)
      assert r <= 1e-12 and np.linalg.norm(x0_f - x0) <= 1e-12 * max(np.linalg.norm(x0), 1.), (spacing, i, gs, r)
  # g == 1 never touches the unconditional half
  assert np.array_equal(I.invert_update(x, None, e_c, 1., 3, tab)[0], I.invert_update(x, e_u * np.nan, e_c, 1., 3, tab)[0])


@pytest.mark.parametrize("spacing", SPACINGS)
def test_t_in_is_the_level_a_prev_names(spacing):
  m = LatentDiffusionModelSampler(None, None, None, step_spacing=spacing, verbose=False, **LDM)
  tin = I.t_in(m._ddim_steps)
  assert tin[0] == 0 and np.array_equal(tin[1:], m._ddim_steps[:-1])
  assert np.array_equal(m._alphas_cumprod[tin], m._ddim_alphas_cumprod_prev)           # exactly
  assert np.array_equal(m.inversion_timesteps(), tin) and m.inversion_timesteps().dtype == np.int32
  # the float32 tables the device holds
  tab = I.make_tables(m._alphas_cumprod, m._ddim_steps)
  assert np.array_equal(tab["a_prev"], m._ddim_alphas_cumprod_prev.astype(np.float32).astype(np.float64))
  assert np.array_equal(tab["c1"], m._ddim_sqrt_recip_alphas_cumprod.astype(np.float32).astype(np.float64))
  assert np.array_equal(tab["c2"], m._ddim_sqrt_recipm1_alphas_cumprod.astype(np.float32).astype(np.float64))


def test_loops_compose_the_updates():
  m = LatentDiffusionModel(None, None, None, **LDM)
  steps, tab = m._ddim_steps, I.make_tables(m._alphas_cumprod, m._ddim_steps)
  seen = []

  def eps_fn(x, t):
    seen.append(t)
    return 0.3 * x, np.sin(x) * (1 + t / 1000.)
  z0 = np.random.default_rng(5).standard_normal((2, 4, 4, 4))
  rec = []
  up = I.invert_loop(eps_fn, z0, 3., 4, steps, tab, record=rec)
  assert seen == [0, int(steps[0]), int(steps[1]), int(steps[2])] and len(rec) == 4 and np.array_equal(rec[-1], up)
  x = z0
  for i in range(4):
    x, _ = I.invert_update(x, *eps_fn(x, 0 if i == 0 else int(steps[i - 1])), 3., i, tab)
  assert np.array_equal(x, up)
  del seen[:]
  I.sample_loop(eps_fn, up, 3., 4, steps, tab)
  assert seen == [int(steps[i]) for i in (3, 2, 1, 0)]
  assert I.invert_loop(eps_fn, z0.astype(np.float32), 3., 4, steps, I.make_tables(m._alphas_cumprod, steps, np.float32),
                       dtype=np.float32).dtype == np.float32


def test_entry_is_declared_everywhere_and_refuses_cpu_tensors():
  with open(os.path.join(ROOT, "include", "ldm_hip.h")) as f:
    src = f.read()
  decl = re.search(r"\bint\s+ldm_cfg_ddim_invert_update\s*\(([^)]*)\)\s*;", src)
  assert decl is not None
  res, args = _lib.SIGNATURES["ldm_cfg_ddim_invert_update"]
  assert res is _lib.c_i32 and len(args) == len(decl.group(1).split(","))
  assert getattr(ctypes.CDLL(_lib.LIB_PATH), "ldm_cfg_ddim_invert_update") is not None
  assert "cfg_ddim_invert_update" in ops.__all__
  z, i = torch.zeros(2, 4, 4, 4), torch.zeros(1, dtype=torch.int32)
  for guided in (True, False):
    with pytest.raises(ValueError, match="device tensors"):
      ops.cfg_ddim_invert_update(torch.zeros(4, 4, 4, 4), z, z.clone(), torch.zeros(10, 4), i, guided, 5.)


def test_host_rejections_need_no_device():
  s = LatentDiffusionModelSampler(None, None, None, verbose=False, **LDM)
  ids = np.zeros((4, 77), dtype=np.int64)
  z0 = np.zeros((2, 8, 8, 4), np.float32)
  with pytest.raises(ValueError, match="schedule"):
    s.ddim_invert_loop(ids, latents=z0, guidance_scale=[1.] * 10)
  with pytest.raises(ValueError, match="exactly one"):
    s.ddim_invert_loop(ids)
  with pytest.raises(ValueError, match="strength"):
    s.ddim_invert_loop(ids, latents=z0, strength=0.05)
  with pytest.raises(ValueError, match="start_index"):
    s.ddim_p_sample_loop(ids, [2, 8, 8, 4], 5., start_index=3)
  with pytest.raises(ValueError, match="start_index"):
    s.ddim_p_sample_loop(ids, [2, 8, 8, 4], 5., x_T=z0, start_index=11)
  with pytest.raises(ValueError, match="same shape"):
    s.ddim_p_sample_loop_edit(ids, ids[:2], z0)
  assert s._inv_graph is None and s._graph is None


def _edit_cfg(tmp_path):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  img = np.arange(64 * 64 * 3, dtype=np.int64).reshape(64, 64, 3).astype(np.uint8)
  np.save(tmp_path / "img.npy", img)
  np.save(tmp_path / "mask.npy", np.ones((64, 64), dtype=np.uint8))
  cfg["ldm_sampling"].update(init_image=str(tmp_path / "img.npy"), source_prompt="a photo of a cat")
  return cfg, img


def test_cli_source_prompt_selects_the_edit_loop(tmp_path):
  cfg, img = _edit_cfg(tmp_path)
  samp = cfg["ldm_sampling"]
  ids, src = np.zeros((8, 77), dtype=np.int64), np.ones((8, 77), dtype=np.int64)
  assert R.needs_encoder(cfg)
  method, args, kwargs = R.sampling_call(cfg, ids, 4, source_ids=src)
  assert method == "ddim_p_sample_loop_edit" and hasattr(LatentDiffusionModelSampler, method)
  assert args[0] is src and args[1] is ids and args[3] == samp["guidance_scale"]
  assert args[2].dtype == np.float32 and np.array_equal(args[2], img.astype(np.float32) / 127.5 - 1)
  assert kwargs == dict(strength=0.75, invert_guidance_scale=1., seed=4)
  samp.update(strength=0.5, invert_guidance_scale=2, guidance_interval=[200, 800])
  kwargs = R.sampling_call(cfg, ids, 4, source_ids=src)[2]
  assert kwargs == dict(strength=0.5, invert_guidance_scale=2., seed=4, guidance_interval=(200, 800))
  # without the key nothing changes: the img2img call, source ids or not
  del samp["source_prompt"], samp["invert_guidance_scale"], samp["guidance_interval"]
  method, args, kwargs = R.sampling_call(cfg, ids, 4)
  assert method == "ddim_p_sample_loop_img2img" and kwargs == dict(strength=0.5, seed=4) and args[0] is ids
  assert R.sampling_call(cfg, ids, 4, source_ids=src)[0] == "ddim_p_sample_loop_img2img"


def test_cli_source_prompt_errors_name_the_key(tmp_path):
  ids, src = np.zeros((8, 77), dtype=np.int64), np.ones((8, 77), dtype=np.int64)
  for key, value in (("mask", str(tmp_path / "mask.npy")), ("window", [8, 8]), ("sample_save_progress", True)):
    cfg, _ = _edit_cfg(tmp_path)
    cfg["ldm_sampling"][key] = value
    with pytest.raises(ValueError, match=rf"source_prompt.*{key}"):
      R.sampling_call(cfg, ids, 0, source_ids=src)
  cfg, _ = _edit_cfg(tmp_path)
  del cfg["ldm_sampling"]["init_image"]
  with pytest.raises(ValueError, match="source_prompt needs ldm_sampling.init_image"):
    R.sampling_call(cfg, ids, 0, source_ids=src)
  cfg, _ = _edit_cfg(tmp_path)
  cfg["ldm_sampling"]["source_prompt"] = ["a", "b"]
  with pytest.raises(ValueError, match="source_prompt must be a string"):
    R.sampling_call(cfg, ids, 0, source_ids=src)
  cfg, _ = _edit_cfg(tmp_path)
  with pytest.raises(ValueError, match="source_prompt"):
    R.sampling_call(cfg, ids, 0)                     # the key without its token ids
