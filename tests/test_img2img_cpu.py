"""img2img / inpainting host rules: the latent mask, the noise streams, the start
index and the CLI's call.  Host-only: nothing runs on a GPU."""
import os

import numpy as np
import pytest
import yaml

from ldm_tf2_amd.model_runners import (ENCODE_STREAM, Q_STREAM, img2img_start, latent_mask,
                                       normal_latents)
from ldm_tf2_amd import run_ldm_sampler as R

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "all_in_one_config.yaml")


def test_latent_mask_min_pool():
  m = np.ones((2, 16, 16), dtype=np.uint8)
  m[0, 9, 3] = 0                                  # one regenerated pixel clears its whole 8x8 cell
  m[1, :8, :] = 0
  got = latent_mask(m, 8)
  assert got.dtype == np.float32 and got.shape == (2, 2, 2)
  assert np.array_equal(got[0], [[1, 1], [0, 1]])
  assert np.array_equal(got[1], [[0, 0], [1, 1]])
  # nonzero (any value) = keep; [H,W] is one mask
  assert np.array_equal(latent_mask(np.full((16, 16), 7), 8), np.ones((1, 2, 2), np.float32))
  with pytest.raises(ValueError):
    latent_mask(np.ones((2, 12, 16)), 8)


def test_noise_streams_shard_independent_and_disjoint():
  shape = (4, 4, 4)
  for stream in (ENCODE_STREAM, Q_STREAM, Q_STREAM + 7):
    whole = normal_latents(3, 0, 4, shape, stream=stream)
    shard = normal_latents(3, 2, 2, shape, stream=stream)
    assert np.array_equal(whole[2:], shard)                   # keyed by global sample index
  x_T = normal_latents(3, 0, 4, shape)
  draws = [x_T] + [normal_latents(3 + 1 + i, 0, 4, shape) for i in range(3)]     # eta noise of DDIM index i
  draws += [normal_latents(3, 0, 4, shape, stream=ENCODE_STREAM)]
  draws += [normal_latents(3, 0, 4, shape, stream=Q_STREAM + i) for i in range(3)]
  flat = [d.reshape(4, -1) for d in draws]
  for a in range(len(flat)):
    for b in range(a + 1, len(flat)):
      for r in range(4):
        for q in range(4):
          assert not np.array_equal(flat[a][r], flat[b][q]), (a, b, r, q)
  # the default (no stream) is unchanged
  g = np.random.default_rng([3, 1])
  assert np.array_equal(x_T[1], g.standard_normal(shape, dtype=np.float32))


def test_start_index_rule():
  assert img2img_start(0.75, 200) == 150
  assert img2img_start(1.0, 10) == 10
  assert img2img_start(0.3, 10) == 3
  assert img2img_start(0.29, 10) == 2                  # int(), not round()
  for bad in (0., -0.5, 1.5, 0.05):                   # 0.05 * 10 -> k = 0
    with pytest.raises(ValueError):
      img2img_start(bad, 10)


def test_reference_yaml_call_unchanged():
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  ids = np.zeros((8, 77), dtype=np.int64)
  assert not R.needs_encoder(cfg)
  method, args, kwargs = R.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop" and kwargs == dict(seed=5)
  assert args[0] is ids and args[1] == cfg["ldm_sampling"]["latent_shape"] and args[2] == 5.
  cfg["ldm_sampling"]["sample_save_progress"] = True
  assert R.sampling_call(cfg, ids, 5)[0] == "ddim_p_sample_loop_progressive"


def test_cli_img2img_keys(tmp_path):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  img = np.arange(64 * 64 * 3, dtype=np.int64).reshape(64, 64, 3).astype(np.uint8)
  pm = np.ones((64, 64), dtype=np.uint8)
  pm[10, 50] = 0
  np.save(tmp_path / "img.npy", img)
  np.save(tmp_path / "mask.npy", pm)
  samp = cfg["ldm_sampling"]
  samp["mask"] = str(tmp_path / "mask.npy")
  with pytest.raises(ValueError):                      # a mask needs an init image
    R.sampling_call(cfg, np.zeros((8, 77)), 0)
  samp["init_image"] = str(tmp_path / "img.npy")
  assert R.needs_encoder(cfg) and R.downsampling_factor(cfg) == 8
  method, args, kwargs = R.sampling_call(cfg, np.zeros((8, 77)), 4)
  assert method == "ddim_p_sample_loop_img2img"
  assert args[1].dtype == np.float32 and np.array_equal(args[1], img.astype(np.float32) / 127.5 - 1)
  assert args[1].min() == -1.0 and args[2] == samp["guidance_scale"]
  assert kwargs["strength"] == 0.75 and kwargs["seed"] == 4
  want = np.ones((8, 8), np.float32)                  # one [H,W] mask -> one [h,w] mask, tiled by the sampler
  want[1, 6] = 0
  assert np.array_equal(kwargs["mask"], want)
  np.save(tmp_path / "mask.npy", np.stack([pm, np.ones_like(pm)]))
  assert R.sampling_call(cfg, np.zeros((4, 77)), 4)[2]["mask"].shape == (2, 8, 8)
  samp["strength"] = 0.5
  assert R.sampling_call(cfg, np.zeros((8, 77)), 4)[2]["strength"] == 0.5
  np.save(tmp_path / "img.npy", img.astype(np.float32))
  with pytest.raises(ValueError):                      # uint8 only
    R.sampling_call(cfg, np.zeros((8, 77)), 4)
