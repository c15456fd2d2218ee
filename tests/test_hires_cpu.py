"""Two-pass high-resolution sampling, host side: the NumPy restatement of the resize against
torch float64, its own identities, the seed rule, the YAML keys, the loop's rejections, and the new entry's declaration
and binding.  Nothing runs on a GPU."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

import hires_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
SHAPES = [((16, 16), (32, 32)), ((8, 8), (12, 20)), ((5, 7), (16, 9)), ((16, 16), (16, 16)), ((1, 1), (4, 4)),
          ((16, 24), (8, 12)), ((3, 5), (7, 4)), ((2, 2), (3, 3))]


def _x(hw, c=4, seed=0):
  x = np.random.default_rng(seed).standard_normal((2,) + tuple(hw) + (c,))
  x[0, 0, 0, 0] = -0.0
  return x


@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_against_torch_float64(src, dst, mode):
  x = _x(src)
  got = H.resize64(x, dst, mode)
  kw = {} if mode == "nearest" else dict(align_corners=False)
  want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=dst, mode=mode, **kw)
  want = want.permute(0, 2, 3, 1).numpy()
  err = np.abs(got - want).max()
  print(f"{mode} {src}->{dst}: max |restatement - torch| = {err:.3e}")
  assert got.shape == want.shape and err <= 1e-14
  if src == dst or mode == "nearest":
    assert np.array_equal(got, want)


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_nearest_is_index_arithmetic(src, dst):
  x = _x(src).astype(np.float32)
  iy = [min((i * src[0]) // dst[0], src[0] - 1) for i in range(dst[0])]
  ix = [min((i * src[1]) // dst[1], src[1] - 1) for i in range(dst[1])]
  want = x[:, iy][:, :, ix]
  got = H.resize64(x, dst, "nearest").astype(np.float32)
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("mode", H.MODES)
def test_identity_size_returns_the_same_bits(mode):
  x = _x((5, 7)).astype(np.float32)
  got = H.resize64(x, (5, 7), mode)
  assert np.array_equal(got, x.astype(np.float64)) and np.signbit(got[0, 0, 0, 0])
  if mode != "nearest":
    got32 = H.resize32(x, (5, 7), mode)
    assert np.array_equal(got32, x)             # (values; the device entry copies, which also keeps the sign of -0.0)


def test_nearest_2x_is_repeat():
  x = _x((16, 16)).astype(np.float32)
  got = H.resize64(x, (32, 32), "nearest").astype(np.float32)
  assert np.array_equal(got, np.repeat(np.repeat(x, 2, axis=1), 2, axis=2))


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_float32_emulation_stays_at_rounding_level(src, dst, mode):
  """The emulation that sets the GPU gates is the same function: within a few float32 roundings of the restatement
  (bicubic: four taps per axis, weights up to 1.27 in absolute sum per axis)."""
  x = _x(src).astype(np.float32)
  err = np.abs(H.resize32(x, dst, mode).astype(np.float64) - H.resize64(x, dst, mode)).max()
  print(f"{mode} {src}->{dst}: float32 emulation error {err / (2.0 ** -23 * np.abs(x).max()):.2f} x 2^-23 max|x|")
  assert err <= 16 * 2.0 ** -23 * np.abs(x).max()


def test_weights_sum_to_one_and_taps_stay_inside():
  """(four cubics of about ten float64 operations each, values up to 1: their sum is 1 to a few tens of 2^-53)"""
  for L in range(1, 9):
    for Lo in range(1, 19):
      for mode in H.MODES:
        idx, w = H.axis_taps(L, Lo, mode)
        assert idx.min() >= 0 and idx.max() <= L - 1, (L, Lo, mode)
        assert np.abs(w.sum(1) - 1.).max() <= 1e-14, (L, Lo, mode)


def test_derived_seed():
  from ldm_tf2_amd.model_runners import hires_seed
  n = 1000
  for seed in (0, 1, 7, 2 ** 31, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 5, 2 ** 64 - 1, 2 ** 64 + 3):
    s2 = hires_seed(seed)
    assert 0 <= s2 < 2 ** 64 and s2 != seed
    first = {seed} | {seed + 1 + i for i in range(n)}                 # the seed words of pass 1's host generators
    second = {s2} | {s2 + 1 + i for i in range(n)}
    assert not first & second
    assert hires_seed(s2) == seed % 2 ** 64


def _cfg(**keys):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  return yaml.safe_load(yaml.safe_dump(dict(cfg, ldm_sampling=dict(cfg["ldm_sampling"], **keys))))


def test_yaml_keys_bind():
  import inspect
  from ldm_tf2_amd import run_ldm_sampler as R
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  ids = np.zeros((8, 77), dtype=np.int64)
  plain = _cfg(sample_save_progress=False)
  assert R.sampling_call(plain, ids, 5) == ("ddim_p_sample_loop", (ids, plain["ldm_sampling"]["latent_shape"],
                                                                  plain["ldm_sampling"]["guidance_scale"]),
                                            dict(seed=5))              # no `hires_shape`: today's call
  assert R.decode_latent_size(plain) == plain["ldm_sampling"]["latent_shape"][1]
  cfg = _cfg(sample_save_progress=False, latent_shape=[4, 32, 32, 4], hires_shape=[4, 64, 64, 4])
  method, args, kwargs = R.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop_hires"
  assert args[0] is ids and args[1:] == ([4, 32, 32, 4], [4, 64, 64, 4])
  assert kwargs == dict(strength=0.5, resize="bilinear", guidance_scale=cfg["ldm_sampling"]["guidance_scale"], seed=5)
  assert R.decode_latent_size(cfg) == 64
  cfg = _cfg(sample_save_progress=False, latent_shape=[4, 32, 32, 4], hires_shape=[4, 64, 48, 4], hires_strength=0.3,
             hires_resize="bicubic", guidance_interval=[200, 600])
  kwargs = R.sampling_call(cfg, ids, 5)[2]
  assert kwargs["strength"] == 0.3 and kwargs["resize"] == "bicubic" and kwargs["guidance_interval"] == (200, 600)
  params = inspect.signature(LatentDiffusionModelSampler.ddim_p_sample_loop_hires).parameters
  assert list(params)[1:6] == ["cond_model_inputs", "shape", "hires_shape", "strength", "resize"]
  assert set(kwargs) <= set(params)


@pytest.mark.parametrize("extra,match", [
    (dict(init_image="x.npy"), "init_image"), (dict(mask="m.npy"), "mask"), (dict(window=[32, 32]), "window"),
    (dict(source_prompt="a cat"), "source_prompt"), (dict(sample_save_progress=True), "sample_save_progress"),
    (dict(hires_shape=[4, 64, 64]), "hires_shape"), (dict(hires_shape=[4, 64.0, 64, 4]), "hires_shape"),
    (dict(hires_resize="lanczos"), "hires_resize")])
def test_yaml_rejected_combinations(extra, match):
  from ldm_tf2_amd import run_ldm_sampler as R
  keys = dict(sample_save_progress=False, latent_shape=[4, 32, 32, 4], hires_shape=[4, 64, 64, 4])
  keys.update(extra)
  with pytest.raises(ValueError, match=match):
    R.sampling_call(_cfg(**keys), np.zeros((8, 77), dtype=np.int64), 5, source_ids=np.zeros((8, 77), dtype=np.int64))


class _FakeModel:
  device = torch.device("cpu")
  skip_lvl = [0, 0, 1, 1, 2, 2, 3]               # (a U-Net that halves its input three times)


def test_loop_rejections_need_no_gpu():
  """Raised before anything touches a model or the device."""
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  s = LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), num_steps=1000, beta_start=0.00085,
                                  beta_end=0.012, num_ddim_steps=10)
  ids = np.zeros((4, 77), dtype=np.int64)
  with pytest.raises(ValueError, match="batch and channels"):
    s.ddim_p_sample_loop_hires(ids, [2, 16, 16, 4], [3, 32, 32, 4])
  with pytest.raises(ValueError, match="batch and channels"):
    s.ddim_p_sample_loop_hires(ids, [2, 16, 16, 4], [2, 32, 32, 3])
  for bad in ([2, 32, 36, 4], [2, 30, 32, 4], [2, 0, 32, 4]):
    with pytest.raises(ValueError, match="multiples of 8"):
      s.ddim_p_sample_loop_hires(ids, [2, 16, 16, 4], bad)
  with pytest.raises(ValueError, match="resize"):
    s.ddim_p_sample_loop_hires(ids, [2, 16, 16, 4], [2, 32, 32, 4], resize="lanczos")
  for strength in (0., 1.5, 0.05):
    with pytest.raises(ValueError, match="strength"):
      s.ddim_p_sample_loop_hires(ids, [2, 16, 16, 4], [2, 32, 32, 4], strength=strength)
  assert s._state_key is None and s._graph is None and not s._states   # nothing was allocated or captured


def test_the_new_entry_is_declared_bound_and_exported():
  import ctypes
  from ldm_tf2_amd import _lib, ops
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldm_hip.h")).read(), flags=re.S)
  ctype = {"int": _lib.c_i32, "void*": _lib.c_vp, "const float*": _lib.c_vp, "float*": _lib.c_vp}
  m = re.search(r"\bint\s+ldm_resize_nhwc\s*\(([^)]*)\)\s*;", src)
  assert m
  ps = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
  assert [p.rsplit(" ", 1)[1] for p in ps] == ["x", "out", "B", "H", "W", "c", "Ho", "Wo", "mode", "stream"]
  res, args = _lib.SIGNATURES["ldm_resize_nhwc"]
  assert res is _lib.c_i32 and args == [ctype[p.rsplit(" ", 1)[0]] for p in ps]
  assert isinstance(_lib.lib.ldm_resize_nhwc, ctypes._CFuncPtr)
  for name, value in _lib.RESIZE_MODES.items():
    assert re.search(r"#define\s+LDM_RESIZE_%s\s+%d\b" % (name.upper(), value), src), name
  assert "resize_nhwc" in ops.__all__
  with pytest.raises(ValueError, match="resize mode"):
    ops.resize_nhwc(torch.zeros(1, 2, 2, 4), (4, 4), "lanczos")
