"""Panorama sampling, host side: the window grid, the NumPy restatement's own identities, the
YAML keys, the loop's rejections, and the new entries' declaration and binding.  Nothing runs on a GPU."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

import panorama_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")


@pytest.mark.parametrize("args,want", [((16, 16, 8), [0]), ((24, 16, 8), [0, 8]), ((28, 16, 8), [0, 8, 12]),
                                       ((7, 3, 3), [0, 3, 4]), ((5, 5, 1), [0])])
def test_window_origins(args, want):
  from ldm_tf2_amd.model_runners import window_origins
  assert window_origins(*args) == want and P.origins(*args) == want


@pytest.mark.parametrize("args", [(8, 9, 4), (8, 4, 0), (8, 4, 5), (8, 0, 1), (8, 4, -1)])
def test_window_origins_rejects(args):
  from ldm_tf2_amd.model_runners import window_origins
  with pytest.raises(ValueError):
    window_origins(*args)


def test_window_origins_increase_and_cover_every_position():
  from ldm_tf2_amd.model_runners import window_origins
  for L in range(1, 13):
    for l in range(1, L + 1):
      for s in range(1, l + 1):
        o = window_origins(L, l, s)
        assert o == P.origins(L, l, s) and o[0] == 0 and o[-1] == L - l, (L, l, s, o)
        assert len(o) == -((l - L) // s) + 1
        assert all(b > a for a, b in zip(o, o[1:])), (L, l, s, o)
        covered = np.zeros(L, dtype=int)
        for a in o:
          assert 0 <= a and a + l <= L
          covered[a:a + l] += 1
        assert covered.min() >= 1, (L, l, s, o)
        assert all(b - a <= s for a, b in zip(o, o[1:]))          # (only the clamped last window moves closer)


@pytest.mark.parametrize("shape,window,stride", [((2, 16, 24, 4), (8, 8), (4, 4)), ((1, 8, 8, 3), (8, 8), (4, 4)),
                                                 ((2, 6, 8, 4), (3, 4), (3, 4)), ((1, 16, 40, 4), (16, 16), (8, 8))])
def test_restatement_fold_of_gather_is_the_identity(shape, window, stride):
  """Every cell is covered 1, 2 or 4 times by copies of the same value: the sums and the division by a power of
  two are exact."""
  B, H, W, c = shape
  assert set(np.unique(P.counts(H, W, window, stride))) <= {1, 2, 4}
  x = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
  x[0, 0, 0, 0] = -0.0
  win = P.gather(x, window, stride)
  assert win.shape == (2, B, len(P.windows(H, W, window, stride)), window[0], window[1], c)
  assert np.array_equal(win[0], win[1])
  back = P.fold(win, H, W, window, stride)
  assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), np.stack([x, x]).view(np.uint32))
  b64 = P.fold64(win, H, W, window, stride)
  assert b64.dtype == np.float64 and np.array_equal(b64, np.stack([x, x]).astype(np.float64))


def test_restatement_fold_sums_in_window_order():
  """Three covering values whose float32 sum depends on the order: (1 + 2^-24) + 2^-24 = 1 (each addend is lost),
  while 2^-24 + 2^-24 + 1 = 1 + 2^-23."""
  H, W, window, stride = 1, 3, (1, 2), (1, 1)                        # windows at x = 0, 1; cell 1 is covered by both
  assert P.windows(H, W, window, stride) == [(0, 0), (0, 1)]
  tiny = np.float32(2.0 ** -24)
  win = np.zeros((1, 1, 2, 1, 2, 1), dtype=np.float32)
  win[0, 0, 0, 0, 1, 0], win[0, 0, 1, 0, 0, 0] = 1., tiny
  assert P.fold(win, H, W, window, stride)[0, 0, 0, 1, 0] == np.float32(0.5)      # (1 + 2^-24 -> 1) / 2
  assert P.fold64(win, H, W, window, stride)[0, 0, 0, 1, 0] == (1. + 2.0 ** -24) / 2


def test_default_stride_and_pairs():
  from ldm_tf2_amd.model_runners import window_and_stride
  assert window_and_stride((32, 32)) == ((32, 32), (16, 16))
  assert window_and_stride([5, 1]) == ((5, 1), (2, 1))              # rounded down, at least 1
  assert window_and_stride(16, 8) == ((16, 16), (8, 8))
  assert window_and_stride((16, 32), (4, 12)) == ((16, 32), (4, 12))
  for bad in ((16,), (16, 16, 16), "ab", (1.5, 2)):
    with pytest.raises(ValueError):
      window_and_stride(bad)


def _cfg(**keys):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  return yaml.safe_load(yaml.safe_dump(dict(cfg, ldm_sampling=dict(cfg["ldm_sampling"], **keys))))


def test_yaml_keys_bind():
  from ldm_tf2_amd import run_ldm_sampler as R
  ids = np.zeros((8, 77), dtype=np.int64)
  before = R.sampling_call(_cfg(), ids, 5)
  assert before[0] in ("ddim_p_sample_loop", "ddim_p_sample_loop_progressive")
  assert "window" not in before[2] and "stride" not in before[2]     # no `window` key: today's method and arguments
  plain = _cfg(sample_save_progress=False)
  assert R.sampling_call(plain, ids, 5)[0] == "ddim_p_sample_loop"
  assert R.sampling_call(plain, ids, 5)[2] == dict(seed=5)
  cfg = _cfg(sample_save_progress=False, latent_shape=[4, 32, 144, 4], window=[32, 32])
  method, args, kwargs = R.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop_panorama"
  assert args[0] is ids and args[1] == [4, 32, 144, 4] and args[2] == cfg["ldm_sampling"]["guidance_scale"]
  assert kwargs == dict(window=(32, 32), stride=(16, 16), seed=5)    # the default stride: half the window
  cfg["ldm_sampling"]["window_stride"] = [32, 8]
  assert R.sampling_call(cfg, ids, 5)[2] == dict(window=(32, 32), stride=(32, 8), seed=5)
  # the loop's own signature takes what the CLI passes
  import inspect
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  params = inspect.signature(LatentDiffusionModelSampler.ddim_p_sample_loop_panorama).parameters
  assert list(params)[1:6] == ["cond_model_inputs", "shape", "window", "stride", "guidance_scale"]
  assert set(kwargs) <= set(params)


@pytest.mark.parametrize("extra,match", [
    (dict(init_image="x.npy"), "init_image"), (dict(init_image="x.npy", mask="m.npy"), "init_image"),
    (dict(mask="m.npy"), "mask"), (dict(sample_save_progress=True), "sample_save_progress"),
    (dict(guidance_interval=[200, 600]), "guidance_interval"), (dict(guidance_scale=[5.] * 50), "guidance_scale"),
    (dict(window=[32]), "window"), (dict(window_stride=[8, 8, 8]), "window_stride")])
def test_yaml_rejected_combinations(extra, match):
  from ldm_tf2_amd import run_ldm_sampler as R
  keys = dict(sample_save_progress=False, latent_shape=[4, 32, 144, 4], window=[32, 32])
  keys.update(extra)
  with pytest.raises(ValueError, match=match):
    R.sampling_call(_cfg(**keys), np.zeros((8, 77), dtype=np.int64), 5)


class _FakeModel:
  device = torch.device("cpu")


def test_loop_rejections_need_no_gpu():
  """Raised before anything touches a model or the device."""
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  s = LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), num_steps=1000, beta_start=0.00085,
                                  beta_end=0.012, num_ddim_steps=10)
  ids = np.zeros((4, 77), dtype=np.int64)
  with pytest.raises(ValueError, match="guidance"):
    s.ddim_p_sample_loop_panorama(ids, [2, 16, 28, 4], (16, 16), guidance_scale=[5.] * 10)
  with pytest.raises(ValueError, match="guidance"):
    s.ddim_p_sample_loop_panorama(ids, [2, 16, 28, 4], (16, 16), guidance_interval=(200, 600))
  with pytest.raises(ValueError, match="window extent"):
    s.ddim_p_sample_loop_panorama(ids, [2, 16, 28, 4], (16, 32))
  with pytest.raises(ValueError, match="stride"):
    s.ddim_p_sample_loop_panorama(ids, [2, 16, 28, 4], (16, 16), stride=(8, 17))
  with pytest.raises(ValueError, match="stride"):
    s.ddim_p_sample_loop_panorama(ids, [2, 16, 28, 4], (16, 16), stride=(0, 8))


def test_the_new_entries_are_declared_bound_and_exported():
  import ctypes
  from ldm_tf2_amd import _lib, ops
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldm_hip.h")).read(), flags=re.S)
  ctype = {"int": _lib.c_i32, "void*": _lib.c_vp, "const float*": _lib.c_vp, "float*": _lib.c_vp}
  for name in ("ldm_window_gather", "ldm_window_fold"):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    ps = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    types = [ctype[p.rsplit(" ", 1)[0]] for p in ps]
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_i32 and args == types, (name, ps)
    assert isinstance(getattr(_lib.lib, name), ctypes._CFuncPtr)
  assert "window_gather" in ops.__all__ and "window_fold" in ops.__all__
  assert _lib.lib.ldm_version() >= 100
