"""DiffEdit host rules: the NumPy restatement against hand-worked cases, the inputs of the GPU
mask test, the new entries' declarations, the keyword rejections and the CLI's call.  Host-only: nothing runs on a GPU."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

import diffedit_ref as DR
from ldm_tf2_amd import _lib, ops
from ldm_tf2_amd import run_ldm_sampler as R
from ldm_tf2_amd.model_runners import MAP_STREAM, PREVIEW_FIT_STREAM, Q_STREAM, LatentDiffusionModelSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012, v_posterior=0., scale_factor=0.18215, eta=0.,
           num_ddim_steps=10)


# ---- the restatement against hand-worked cases -------------------------------------------------------------
def test_contrast_accum_by_hand():
  e_src = np.array([[[1., 2., 3., 4.]], [[0., 0., 0., 0.]]], np.float32)           # [B=2, cells=1, c=4]
  e_tgt = np.array([[[2., 0., 3., 8.]], [[-1., 1., -1., 1.]]], np.float32)
  acc = DR.contrast_accum(np.array([[10.], [0.5]], np.float32), e_src, e_tgt)
  assert acc.dtype == np.float32 and acc.tolist() == [[17.], [4.5]]                # 1 + 2 + 0 + 4; 1 + 1 + 1 + 1
  # the order is the stated one: ((|d0| + |d1|) + |d2|) + |d3|, then acc + s, each rounded to float32
  d = np.array([1., 2. ** -24, 2. ** -24, 2. ** -24], np.float32)
  got = DR.contrast_accum(np.zeros((1, 1), np.float32), np.zeros((1, 1, 4), np.float32), d[None, None])
  assert got[0, 0] == np.float32(1.)                                               # each small term is rounded away
  got = DR.contrast_accum(np.zeros((1, 1), np.float32), np.zeros((1, 1, 4), np.float32), d[::-1][None, None].copy())
  assert got[0, 0] == np.float32(1. + 2. ** -22)                 # summed first they survive: 1 + 1.5 ulp, tie to even
  # a NaN in one channel reaches its own cell only
  e = np.zeros((1, 3, 4), np.float32)
  e[0, 1, 2] = np.nan
  got = DR.contrast_accum(np.ones((1, 3), np.float32), np.zeros((1, 3, 4), np.float32), e)
  assert np.isnan(got[0, 1]) and got[0, 0] == 1. and got[0, 2] == 1.


def test_mask_of_a_3x3_map_with_a_known_mean():
  acc = np.array([[[0., 1., 2.], [3., 4., 5.], [6., 7., 8.]]], np.float32)        # sum 36, mean 4
  m = DR.contrast_mask(acc, 1.5)                                                   # thr 6: edits 7 and 8 only
  assert m["mean64"].tolist() == [4.] and m["thr"].tolist() == [6.] and m["edited"].tolist() == [2]
  assert m["mask"][0].tolist() == [[1., 1., 1.], [1., 1., 1.], [1., 0., 0.]]       # (6 itself is kept: > is strict)
  assert m["mask"].dtype == np.float32
  # HF diffusers' rule with the mean per sample: clamp(map, 0, ratio mean) / (ratio mean) > threshold
  ratio, thr = 3., 0.5
  hf = np.clip(acc, 0, ratio * 4.) / (ratio * 4.) > thr
  assert np.array_equal(DR.contrast_mask(acc, thr * ratio)["mask"] == 0, hf)


def test_dilation_at_a_corner_and_at_an_edge():
  e = np.zeros((1, 5, 6), bool)
  e[0, 0, 0] = True                                                                # a corner
  d1 = DR.dilate(e, 1)[0]
  assert d1.sum() == 4 and d1[:2, :2].all()
  d3 = DR.dilate(e, 3)[0]
  assert d3.sum() == 16 and d3[:4, :4].all()
  e = np.zeros((1, 5, 6), bool)
  e[0, 2, 5] = True                                                                # the right edge
  d1 = DR.dilate(e, 1)[0]
  assert d1.sum() == 6 and d1[1:4, 4:6].all()
  d2 = DR.dilate(e, 2)[0]
  assert d2.sum() == 15 and d2[0:5, 3:6].all()
  assert np.array_equal(DR.dilate(e, 0), e)
  # through contrast_mask: the count is taken after the dilation
  acc = np.zeros((1, 5, 6), np.float32)
  acc[0, 2, 5] = 30.
  m = DR.contrast_mask(acc, 1.5, 1)
  assert m["edited"].tolist() == [6] and np.array_equal(m["mask"][0] == 0, d1)


def test_an_all_zero_sample_edits_nothing_and_a_nan_keeps_its_cell():
  acc = np.zeros((2, 4, 4), np.float32)
  acc[1] = np.arange(16, dtype=np.float32).reshape(4, 4)
  m = DR.contrast_mask(acc, 0.5, 3)
  assert m["mask"][0].min() == 1. and m["edited"][0] == 0 and m["thr"][0] == 0.    # 0 > 0 is false
  assert m["edited"][1] == 16
  # a NaN cell: the mean and the threshold are NaN, every comparison is false, the whole sample is kept
  acc[1, 2, 2] = np.nan
  m = DR.contrast_mask(acc, 0.5)
  assert np.isnan(m["thr"][1]) and m["mask"][1].min() == 1. and m["edited"][1] == 0
  # tau = 0 edits every positive cell
  assert DR.contrast_mask(np.array([[[0., 1.]]], np.float32), 0.)["mask"].tolist() == [[[1., 0.]]]


def test_blend_keeps_the_trajectory_bit_for_bit():
  g = np.random.default_rng(5)
  traj, x = g.standard_normal((2, 4, 4, 4)).astype(np.float32), g.standard_normal((2, 4, 4, 4)).astype(np.float32)
  m = np.zeros((2, 4, 4), np.float32)
  m[:, :, :2] = 1.
  out = DR.blend(m, traj, x)
  assert out.dtype == np.float32
  assert np.array_equal(out[:, :, :2], traj[:, :, :2]) and np.array_equal(out[:, :, 2:], x[:, :, 2:])
  # the update launch's form of it: m (0 z0 + 1 traj) + (1 - m) x
  z0 = g.standard_normal((2, 4, 4, 4)).astype(np.float32)
  q = np.float32(0.) * z0 + np.float32(1.) * traj
  assert np.array_equal(m[..., None] * q + (1 - m[..., None]) * x, out)


def test_diffedit_loop_degenerate_masks():
  """All zeros: the plain edit (inversion, then sampling); all ones: every step but the last lands on the trajectory."""
  import inversion_ref as I
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  m = LatentDiffusionModel(None, None, None, **LDM)
  tab, steps = I.make_tables(m._alphas_cumprod, m._ddim_steps), m._ddim_steps
  g = np.random.default_rng(6)
  z0 = g.standard_normal((1, 4, 4, 4))
  wa, wb = g.standard_normal((4, 4)) * 0.3, g.standard_normal((4, 4)) * 0.3
  src = lambda x, t: (None, np.tanh(x @ wa) * (1 + t / 1000.))
  tgt = lambda x, t: (np.tanh(x @ wa), np.tanh(x @ wb) * (1 + t / 1000.))
  k = 6
  up = I.invert_loop(src, z0, 1., k, steps, tab)
  plain = I.sample_loop(tgt, up, 3., k, steps, tab)
  got, traj = DR.diffedit_loop(src, tgt, z0, np.zeros((1, 4, 4)), 1., 3., k, steps, tab)
  assert np.array_equal(got, plain) and np.array_equal(traj[k - 1], up) and traj.shape[0] == k
  rec = []
  DR.diffedit_loop(src, tgt, z0, np.ones((1, 4, 4)), 1., 3., k, steps, tab, record=rec)
  assert len(rec) == k and all(np.array_equal(rec[s], traj[k - 2 - s]) for s in range(k - 1))
  assert not np.array_equal(rec[-1], z0)                                           # nothing is blended at index 0


# ---- the inputs of the GPU mask test ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", DR.MASK_CASES, ids=lambda c: "x".join(str(v) for v in c[:3]))
def test_random_mask_inputs_have_an_empty_band(case):
  """So the GPU comparison is exact on every cell: no legal summation order moves a cell across the threshold."""
  h, w, r, seed = case
  acc = DR.mask_case_acc(case)
  assert acc.dtype == np.float32 and acc.shape == (3, h, w) and (acc >= 0).all() and not acc[1].any()
  # (the all-zero sample's sum is 0 in any order: its threshold is exact, and 0 > 0 is false)
  assert not DR.band(acc, DR.MASK_TAU)[[0, 2]].any()
  m =DR.contrast_mask(acc, DR.MASK_TAU, r)
  assert m["edited"][1] == 0
  if h * w > 1:
    assert 0 < m["edited"][0] < h * w and 0 < m["edited"][2] < h * w               # (both sides of the threshold occur)


def test_band_holds_the_cells_at_the_threshold():
  assert DR.band(np.full((1, 2, 2), 2., np.float32), 1.).all()                     # every cell equals the mean
  assert not DR.band(np.array([[[0., 0.], [0., 4.]]], np.float32), 1.).any()       # mean 1: no cell near it
  acc = np.array([[[0., 0.], [0., 4.]]], np.float32)
  acc[0, 0, 0] = np.float32(1.) + np.float32(2. ** -23)                            # one ulp above a threshold of ~1
  assert DR.band(acc, 0.8)[0, 0, 0] and DR.band(acc, 0.8).sum() == 1               # mean 1.25 (1 + 2^-25), thr 1 + ..


# ---- declarations -----------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
  with open(os.path.join(ROOT, "include", "ldm_hip.h")) as f:
    src = f.read()
  for name in ("ldm_eps_contrast_accum", "ldm_contrast_mask_supported", "ldm_contrast_mask", "ldm_store_row"):
    decl = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
    assert decl is not None, name
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_i32 and len(args) == len(decl.group(1).split(",")), name
    assert getattr(_lib.lib, name) is not None
  for name in ("eps_contrast_accum", "contrast_mask", "contrast_mask_supported", "store_row"):
    assert name in ops.__all__
  assert ops.contrast_mask_supported(8, 8192, 3) and ops.contrast_mask_supported(1, 1, 0)
  assert not ops.contrast_mask_supported(8, 8193) and not ops.contrast_mask_supported(16, 16, 4)
  assert not ops.contrast_mask_supported(0, 4) and not ops.contrast_mask_supported(4, 4, -1)
  with pytest.raises(ValueError, match="device tensors"):
    ops.eps_contrast_accum(torch.zeros(2, 4, 4), torch.zeros(1, 4))
  with pytest.raises(ValueError, match="device tensors"):
    ops.contrast_mask(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), 1.5)
  with pytest.raises(ValueError, match="device tensors"):
    ops.store_row(torch.zeros(8), torch.zeros(2, 8), torch.zeros(1, dtype=torch.int32))
  # the draws' streams share no generator key with the other host streams
  assert Q_STREAM + (1 << 29) - 2 < MAP_STREAM and MAP_STREAM + (1 << 29) - 1 < PREVIEW_FIT_STREAM


# ---- keyword rejections (a sampler built without models: every check comes before the first model call) ----------
def test_host_rejections_need_no_device():
  s = LatentDiffusionModelSampler(None, None, None, verbose=False, **LDM)
  ids = np.zeros((4, 77), dtype=np.int64)
  img = np.zeros((2, 64, 64, 3), np.float32)
  z0 = np.zeros((2, 8, 8, 4), np.float32)
  loop = s.ddim_p_sample_loop_diffedit
  with pytest.raises(ValueError, match="schedule"):
    loop(ids, ids, img, guidance_scale=[5.] * 10)
  with pytest.raises(ValueError, match="schedule"):
    loop(ids, ids, img, guidance_interval=(200, 800))
  with pytest.raises(ValueError, match="do not combine"):
    loop(ids, ids, img, preview_freq=2)
  with pytest.raises(ValueError, match="do not combine"):
    loop(ids, ids, img, attn_maps=True)
  with pytest.raises(ValueError, match="same shape"):
    loop(ids, ids[:2], img)
  for fn, args in ((loop, (ids, ids, img)), (s.diffedit_mask, (ids, ids, None, z0))):
    for bad in (-1, 4, 1.5, True):
      with pytest.raises(ValueError, match="mask_dilate"):
        fn(*args, mask_dilate=bad)
    for bad in (0, -3, 2.5):
      with pytest.raises(ValueError, match="num_maps"):
        fn(*args, num_maps=bad)
    for bad in (0.05, 0., 1.5):                                                    # int(0.05 * 10) = 0: k_m < 1
      with pytest.raises(ValueError, match="mask_strength"):
        fn(*args, mask_strength=bad)
    with pytest.raises(ValueError, match="mask_threshold"):
      fn(*args, mask_threshold=-1.)
  with pytest.raises(ValueError, match="strength"):
    loop(ids, ids, img, strength=0.05)
  with pytest.raises(ValueError, match="exactly one"):
    s.diffedit_mask(ids, ids)
  with pytest.raises(ValueError, match="exactly one"):
    s.diffedit_mask(ids, ids, img, z0)
  with pytest.raises(ValueError, match="trajectory"):
    s.last_trajectory()
  with pytest.raises(ValueError, match="contrast map"):
    s.last_contrast_map()
  assert s._dm_graph is None and s._invt_graph is None and s._de_graph is None and s._inv_graph is None


# ---- the CLI ----------------------------------------------------------------------------------------------------
def _edit_cfg(tmp_path):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  img = np.arange(64 * 64 * 3, dtype=np.int64).reshape(64, 64, 3).astype(np.uint8)
  np.save(tmp_path / "img.npy", img)
  cfg["ldm_sampling"].update(init_image=str(tmp_path / "img.npy"), source_prompt="a photo of a cat")
  return cfg, img


def test_cli_edit_mask_selects_the_diffedit_loop(tmp_path):
  cfg, img = _edit_cfg(tmp_path)
  samp = cfg["ldm_sampling"]
  ids, src = np.zeros((8, 77), dtype=np.int64), np.ones((8, 77), dtype=np.int64)
  before = R.sampling_call(cfg, ids, 4, source_ids=src)
  assert before[0] == "ddim_p_sample_loop_edit" and before[2] == dict(strength=0.75, invert_guidance_scale=1., seed=4)
  samp["edit_mask"] = "auto"
  method, args, kwargs = R.sampling_call(cfg, ids, 4, source_ids=src)
  assert method == "ddim_p_sample_loop_diffedit" and hasattr(LatentDiffusionModelSampler, method)
  assert args[0] is src and args[1] is ids and args[3] == samp["guidance_scale"]
  assert args[2].dtype == np.float32 and np.array_equal(args[2], img.astype(np.float32) / 127.5 - 1)
  assert kwargs == dict(strength=0.75, invert_guidance_scale=1., seed=4)           # (the loop has the defaults)
  samp.update(strength=0.5, edit_mask_strength=0.4, edit_mask_maps=6, edit_mask_threshold=0.6,
              edit_mask_clamp_ratio=2, edit_mask_dilate=1, init_fit="crop")
  kwargs = R.sampling_call(cfg, ids, 4, source_ids=src)[2]
  f = R.downsampling_factor(cfg)
  assert kwargs == dict(strength=0.5, invert_guidance_scale=1., seed=4, mask_strength=0.4, num_maps=6,
                        mask_threshold=0.6, mask_clamp_ratio=2., mask_dilate=1,
                        image_size=(f * samp["latent_shape"][1], f * samp["latent_shape"][2]), fit="crop",
                        resample="lanczos3")
  assert type(kwargs["num_maps"]) is int and type(kwargs["mask_clamp_ratio"]) is float
  # every keyword is one of the loop's
  import inspect
  assert set(kwargs) <= set(inspect.signature(LatentDiffusionModelSampler.ddim_p_sample_loop_diffedit).parameters)
  # without the key the calls are what they were
  for key in [k for k in samp if k.startswith("edit_mask")] + ["init_fit"]:
    del samp[key]
  samp["strength"] = 0.75
  after = R.sampling_call(cfg, ids, 4, source_ids=src)
  assert after[0] == before[0] and after[2] == before[2] and after[1][0] is src
  del samp["source_prompt"]
  method, _, kwargs = R.sampling_call(cfg, ids, 4)
  assert method == "ddim_p_sample_loop_img2img" and kwargs == dict(strength=0.75, seed=4)


def test_cli_edit_mask_errors_name_the_key(tmp_path):
  ids, src = np.zeros((8, 77), dtype=np.int64), np.ones((8, 77), dtype=np.int64)
  for key, value in (("edit_mask_strength", 0.4), ("edit_mask_maps", 4), ("edit_mask_threshold", 0.5),
                     ("edit_mask_clamp_ratio", 3.), ("edit_mask_dilate", 1)):
    cfg, _ = _edit_cfg(tmp_path)
    cfg["ldm_sampling"][key] = value
    with pytest.raises(ValueError, match=rf"{key} needs ldm_sampling.edit_mask"):
      R.sampling_call(cfg, ids, 0, source_ids=src)
    del cfg["ldm_sampling"]["source_prompt"]                                       # whatever the loop
    with pytest.raises(ValueError, match=rf"{key} needs ldm_sampling.edit_mask"):
      R.sampling_call(cfg, ids, 0)
  for key in ("source_prompt", "init_image"):
    cfg, _ = _edit_cfg(tmp_path)
    cfg["ldm_sampling"]["edit_mask"] = "auto"
    del cfg["ldm_sampling"][key]
    with pytest.raises(ValueError, match=rf"edit_mask needs ldm_sampling.{key}"):
      R.sampling_call(cfg, ids, 0, source_ids=src)
  for key, value in (("edit_mask", "manual"), ("edit_mask", True), ("edit_mask_maps", 0), ("edit_mask_maps", 2.5),
                     ("edit_mask_dilate", 4), ("edit_mask_dilate", True), ("edit_mask_strength", 0.),
                     ("edit_mask_strength", "half"), ("edit_mask_threshold", -1.), ("edit_mask_clamp_ratio", "x")):
    cfg, _ = _edit_cfg(tmp_path)
    cfg["ldm_sampling"]["edit_mask"] = "auto"
    cfg["ldm_sampling"][key] = value
    with pytest.raises(ValueError, match=rf"ldm_sampling\.{key}\b"):
      R.sampling_call(cfg, ids, 0, source_ids=src)
  cfg, _ = _edit_cfg(tmp_path)
  cfg["ldm_sampling"].update(edit_mask="auto", guidance_interval=[200, 800])
  with pytest.raises(ValueError, match="edit_mask.*guidance_interval"):
    R.sampling_call(cfg, ids, 0, source_ids=src)
  cfg, _ = _edit_cfg(tmp_path)
  cfg["ldm_sampling"].update(edit_mask="auto", guidance_scale=[5.] * 50)
  with pytest.raises(ValueError, match="edit_mask.*guidance_scale"):
    R.sampling_call(cfg, ids, 0, source_ids=src)
  # source_prompt still rejects mask, with or without edit_mask
  np.save(tmp_path / "mask.npy", np.ones((64, 64), dtype=np.uint8))
  for extra in ({}, dict(edit_mask="auto")):
    cfg, _ = _edit_cfg(tmp_path)
    cfg["ldm_sampling"].update(mask=str(tmp_path / "mask.npy"), **extra)
    with pytest.raises(ValueError, match="source_prompt.*mask"):
      R.sampling_call(cfg, ids, 0, source_ids=src)
