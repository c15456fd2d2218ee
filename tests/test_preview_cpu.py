"""Latent previews, host rules: the slot rule, the quantisation, the matrix fit and the CLI's
keys.  Host-only: nothing runs on a GPU."""
import os

import numpy as np
import pytest
import yaml

import preview_ref as P
from ldm_tf2_amd import run_ldm_sampler as R
from ldm_tf2_amd.model_runners import fit_latent_preview, preview_slots

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "all_in_one_config.yaml")


# ---- the slot rule against the progressive loop's overwrite rule -------------------------------------
@pytest.mark.parametrize("N", [10, 7])
@pytest.mark.parametrize("q", [1, 3, 5, 10, 11])
def test_slot_rule_is_last_write_wins(N, q):
  """ddim_p_sample_loop_progressive writes slot index // q on EVERY step (while the slot exists) and the last write,
  the smallest index of the slot, stays.  The kernel's rule writes a slot once, at that index."""
  R_ = preview_slots(N, q)
  assert R_ == (N - 1) // q + 1
  replay = {}
  for index in range(N - 1, -1, -1):             # brute force: every step overwrites its slot
    if index // q < R_:
      replay[index // q] = index
  ours = {}
  for index in range(N - 1, -1, -1):
    r = P.slot_of(index, q, R_)
    if r is not None:
      assert r not in ours                       # (no dead writes: a slot is written once)
      ours[r] = index
  assert ours == replay
  assert sorted(ours) == list(range(R_)) and all(ours[r] == r * q for r in ours)
  # the progressive loop's own strip is shorter (N // q slots): on the slots it has, the two agree
  for r in range(N // q):
    assert ours[r] == r * q
  # outside the strip nothing is written
  assert P.slot_of(-1, q, R_) is None and P.slot_of(-q, q, R_) is None and P.slot_of(R_ * q, q, R_) is None
  # an img2img loop from k - 1 reaches the slots up to (k - 1) // q only
  k = max(N // 2, 1)
  reached = {P.slot_of(i, q, R_) for i in range(k - 1, -1, -1)} - {None}
  assert reached == set(range((k - 1) // q + 1))


# ---- quantise ------------------------------------------------------------------------------------------
def test_quantise_values():
  t = lambda v: 127.5 * np.asarray(v, dtype=np.float64) + 127.5
  assert P.quantise(t(-1.)) == 0 and P.quantise(t(1.)) == 255 and P.quantise(t(0.)) == 128     # 127.5 is a tie: up
  assert np.array_equal(P.quantise([0.5, 1.5, 2.5, 254.5, 0.49999, 1.49999]), [1, 2, 3, 255, 0, 1])
  assert np.array_equal(P.quantise([-1e9, -0.6, -0.4, 255.4, 255.6, 1e9, np.inf, -np.inf]), [0, 0, 0, 255, 255, 255, 255, 0])
  assert P.quantise(np.nan) == 0 and P.quantise(np.array([np.nan, 3.2]))[1] == 3
  assert P.quantise([1.]).dtype == np.uint8


def test_preview32_tracks_preview64():
  g = np.random.default_rng(0)
  lat = g.standard_normal((2, 5, 7, 4))
  proj = 0.3 * g.standard_normal((5, 3))
  for mode in P.MODES:
    for scale in (1, 3):
      t64 = P.preview64(lat.astype(np.float32), proj.astype(np.float32), scale, mode)
      t32 = P.preview32(lat, proj, scale, mode)
      assert t32.dtype == np.float32 and t32.shape == t64.shape == (2, 5 * scale, 7 * scale, 3)
      assert np.abs(t32 - t64).max() < 1e-3
  # nearest repeats cells; scale 1 is the projection itself
  t = P.preview64(lat, proj, 2, "nearest")
  assert np.array_equal(t[:, ::2, ::2], t[:, 1::2, 1::2])
  assert np.allclose(P.preview64(lat, proj, 1, "bilinear"), 127.5 * (lat @ proj[:4] + proj[4]) + 127.5)


# ---- the fit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 3])
def test_fit_recovers_affine_map(c):
  g = np.random.default_rng(c)
  n, h, w, f = 6, 4, 4, 2
  proj = g.uniform(-0.5, 0.5, size=(c + 1, 3))
  lat = g.standard_normal((n, h, w, c))
  cells = lat @ proj[:c] + proj[c]
  images = np.repeat(np.repeat(cells, f, axis=1), f, axis=2)          # block-constant images
  got = fit_latent_preview(lat, images)
  assert got.dtype == np.float32 and got.shape == (c + 1, 3)
  assert np.abs(got - proj).max() < 1e-6
  # a block MEAN: images that vary inside a block with the same mean give the same matrix
  wobble = np.tile(np.array([[1., -1.], [-1., 1.]]), (h, w))[None, :, :, None] * 0.25
  assert np.abs(fit_latent_preview(lat, images + wobble) - proj).max() < 1e-6


def test_fit_errors():
  g = np.random.default_rng(1)
  with pytest.raises(ValueError, match="rank"):                        # n h w = 4 < c + 1 = 5
    fit_latent_preview(g.standard_normal((1, 2, 2, 4)), g.standard_normal((1, 4, 4, 3)))
  with pytest.raises(ValueError, match="rank"):                        # a constant channel is the bias column
    lat = g.standard_normal((2, 4, 4, 4))
    lat[..., 2] = 1.
    fit_latent_preview(lat, g.standard_normal((2, 8, 8, 3)))
  lat = g.standard_normal((2, 4, 4, 4))
  for shape in ((2, 9, 8, 3), (2, 8, 12, 3), (2, 2, 2, 3)):            # not one integer multiple
    with pytest.raises(ValueError, match="multiple"):
      fit_latent_preview(lat, np.zeros(shape))
  with pytest.raises(ValueError):
    fit_latent_preview(lat, np.zeros((3, 8, 8, 3)))


# ---- the CLI's keys ------------------------------------------------------------------------------------
def _cfg():
  with open(CFG) as f:
    return yaml.safe_load(f)


def test_cli_preview_keys(tmp_path):
  cfg = _cfg()
  ids = np.zeros((8, 77), dtype=np.int64)
  samp = cfg["ldm_sampling"]
  assert R.preview_settings(cfg) is None and R.sampling_call(cfg, ids, 5)[2] == dict(seed=5)     # nothing changes
  samp["preview_freq"] = 5
  method, _, kwargs = R.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop" and kwargs == dict(seed=5, preview_freq=5)
  assert R.preview_settings(cfg) == dict(freq=5, scale=R.downsampling_factor(cfg), mode="bilinear", matrix=None)
  samp.update(preview_scale=2, preview_mode="nearest", preview_matrix="m.npy")
  assert R.preview_settings(cfg) == dict(freq=5, scale=2, mode="nearest", matrix="m.npy")
  # img2img takes it too
  np.save(tmp_path / "img.npy", np.zeros((64, 64, 3), np.uint8))
  samp["init_image"] = str(tmp_path / "img.npy")
  method, _, kwargs = R.sampling_call(cfg, ids, 4)
  assert method == "ddim_p_sample_loop_img2img" and kwargs["preview_freq"] == 5 and kwargs["seed"] == 4


@pytest.mark.parametrize("key,value", [("window", [16, 16]), ("hires_shape", [4, 16, 16, 4]),
                                       ("source_prompt", "a photo"), ("sample_save_progress", True)])
def test_cli_preview_rejects_other_loops(tmp_path, key, value):
  cfg = _cfg()
  samp = cfg["ldm_sampling"]
  samp["sample_save_progress"] = False
  np.save(tmp_path / "img.npy", np.zeros((64, 64, 3), np.uint8))
  if key == "source_prompt":
    samp["init_image"] = str(tmp_path / "img.npy")
  samp[key] = value
  ids = np.zeros((8, 77), dtype=np.int64)
  assert R.sampling_call(cfg, ids, 0, source_ids=ids)[0] != "ddim_p_sample_loop"       # the key alone is fine
  samp["preview_freq"] = 2
  with pytest.raises(ValueError, match=f"preview_freq cannot be combined with ldm_sampling.{key}"):
    R.sampling_call(cfg, ids, 0, source_ids=ids)


@pytest.mark.parametrize("key,value", [("preview_scale", 4), ("preview_mode", "nearest"), ("preview_matrix", "m.npy")])
def test_cli_preview_keys_need_freq(key, value):
  cfg = _cfg()
  cfg["ldm_sampling"][key] = value
  with pytest.raises(ValueError, match=f"{key} needs ldm_sampling.preview_freq"):
    R.sampling_call(cfg, np.zeros((8, 77), dtype=np.int64), 0)


@pytest.mark.parametrize("key,value", [("preview_freq", 0), ("preview_freq", 2.5), ("preview_freq", True),
                                       ("preview_scale", 0), ("preview_scale", 17), ("preview_mode", "bicubic"),
                                       ("preview_matrix", 3)])
def test_cli_preview_bad_values(key, value):
  cfg = _cfg()
  cfg["ldm_sampling"]["preview_freq"] = 2
  cfg["ldm_sampling"][key] = value
  with pytest.raises(ValueError, match=key):
    R.sampling_call(cfg, np.zeros((8, 77), dtype=np.int64), 0)


def test_loops_without_previews_do_not_take_the_keyword():
  import inspect
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler as S
  for name in ("ddim_p_sample_loop", "ddim_p_sample_loop_img2img"):
    params = inspect.signature(getattr(S, name)).parameters
    assert params["preview_freq"].default is None and params["on_preview"].default is None
  for name in ("ddim_p_sample_loop_panorama", "ddim_p_sample_loop_hires", "ddim_p_sample_loop_edit", "ddim_invert_loop",
               "ddim_p_sample_loop_progressive"):
    assert "preview_freq" not in inspect.signature(getattr(S, name)).parameters
