"""Pixel-space paste-back, host side: the properties of the restatement (tests/paste_ref.py) the
GPU tests rest on, the tap table, the loops' keyword rejections, the CLI keys and the declarations of the new entries.

The float32-against-float64 bound.  A feather value is 1 - V, V two nested chains of 2r + 1 fmas over non-negative
terms whose total is at most 1: every partial sum is at most 1, so each fma rounds by at most 2^-24 absolute (half an
ulp of a value below 1 is 2^-25; 2^-24 also covers the float64-rounded-twice emulation), 2 (2r + 1) roundings in all,
the row chain's error entering the column chain with weights that sum to 1, and the final subtraction rounds once
more: (4r + 3) 2^-24, asserted as the (4r + 6) 2^-24 the GPU test gates the kernel with.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import yaml

import paste_ref as P
from ldm_tf2_amd.feather import MAX_SIGMA, feather_radius, feather_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
SHAPES = [(1, 1, 1, 3), (1, 1, 9, 4), (2, 5, 7, 3), (2, 33, 31, 3), (2, 37, 53, 4), (1, 64, 48, 3), (1, 65, 40, 4)]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
SIGMAS = [0., 0.5, 1.5, 4., 6.]                  # r = 0, 2, 5, 12 and 18 (past the LDS tile's 16: the four launches)
DTYPES = [np.float64, np.float32]
EPS = 2. ** -24


def masks(shape, seed=0):
  """The keep masks of the GPU tests, [B,H,W] float32: sample 0 keeps a centred box (the outpaint shape inverted:
  the middle is kept, the border regenerated); sample 1 keeps all but a sparse 5 % of the pixels and a hole in the
  corner, its holes holding 0, 0.5 and NaN in turn (all three are holes)."""
  B, H, W, _ = shape
  g = np.random.default_rng([seed, B, H, W])
  m = np.zeros((B, H, W), dtype=np.float32)
  m[0, H // 4:H // 4 + max(H // 2, 1), W // 4:W // 4 + max(W // 2, 1)] = 1.
  if B > 1:
    hole = g.random((H, W)) < 0.05
    hole[:max(H // 8, 1), :max(W // 8, 1)] = True
    fill = np.array([0., 0.5, np.nan], dtype=np.float32)[np.arange(H * W).reshape(H, W) % 3]
    m[1] = np.where(hole, fill, np.float32(1.))
  return m


def images(shape, seed=0):
  """(o, d) float32 in [-1, 1]."""
  g = np.random.default_rng([seed, 1, *shape])
  return g.uniform(-1., 1., shape).astype(np.float32), g.uniform(-1., 1., shape).astype(np.float32)


def far_from_holes(m, r):
  """True where no hole lies within Chebyshev distance 2r (pixels outside the image are no holes)."""
  return P.erode(P.kept(m), 2 * r)


# ---- 1. the tap table -----------------------------------------------------------------------------------------
def test_taps():
  assert [feather_radius(s) for s in SIGMAS] == [0, 2, 5, 12, 18] and feather_radius(MAX_SIGMA) == 48
  assert np.array_equal(feather_taps(0.), np.ones(1, dtype=np.float32))
  for sigma in SIGMAS + [1. / 3., 16.]:
    g, r = feather_taps(sigma), feather_radius(sigma)
    assert g.dtype == np.float32 and g.shape == (2 * r + 1,) and (g > 0).all()
    assert np.array_equal(g, g[::-1]) and g.argmax() == r
    assert abs(g.astype(np.float64).sum() - 1.) <= (2 * r + 1) * EPS, sigma
    if r:
      i = np.arange(-r, r + 1, dtype=np.float64)
      want = np.exp(-i * i / (2 * sigma * sigma))
      assert np.array_equal(g, (want / want.sum()).astype(np.float32))
  # the smallest tap: what a wrong or missing tap moves a value by, far above the float32 gate
  assert feather_taps(0.5).min() > 2.6e-4 and feather_taps(4.).min() > 1.1e-3
  for bad in (-0.5, 16.5, float("nan"), float("inf"), "4", None, True):
    with pytest.raises(ValueError, match="mask_feather"):
      feather_radius(bad)


# ---- 2. the restatement's properties --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_feather_properties(shape, sigma, dtype):
  m, r = masks(shape), feather_radius(sigma)
  w = P.feather_ref(m, sigma, dtype)
  assert w.dtype == dtype and w.shape == m.shape
  hole = ~P.kept(m)
  assert not w[hole].any()
  assert (w >= 0).all() and (w <= 1).all()
  assert (w[far_from_holes(m, r)] == 1).all()
  if sigma == 0:
    assert np.array_equal(w, P.kept(m).astype(dtype))
  # a NaN in m is a hole, like any value below 1; values above 1 are kept
  odd = m.copy()
  odd[hole] = np.nan
  odd[~hole] = 7.
  assert np.array_equal(P.feather_ref(odd, sigma, dtype), w)
  # an all-kept mask gives all ones: the picture's border does not fade
  assert np.array_equal(P.feather_ref(np.ones_like(m), sigma, dtype), np.ones(m.shape, dtype=dtype))
  assert not P.feather_ref(np.zeros_like(m), sigma, dtype).any()


def test_the_ramp_lies_inside_the_kept_region():
  """One hole in the middle of a 41 x 41 image, sigma 1.5 (r = 5): 0 on the hole, below 1 next to it, 1 from distance
  2r + 1 on, monotone along the row through the hole."""
  m = np.ones((1, 41, 41), dtype=np.float32)
  m[0, 20, 20] = 0.
  w = P.feather_ref(m, 1.5)[0]
  assert w[20, 20] == 0 and 0 < w[20, 21] < 1 and w[20, 30] < 1 and w[20, 31] == 1 and w[9, 9] == 1 and w[10, 10] < 1
  assert (np.diff(w[20, 21:]) >= 0).all() and (np.diff(w[21:, 20]) >= 0).all()


def test_float32_against_float64_gap():
  for shape in SHAPES:
    for sigma in SIGMAS:
      m, r = masks(shape), feather_radius(sigma)
      gap = np.abs(P.feather_ref(m, sigma, np.float32).astype(np.float64) - P.feather_ref(m, sigma, np.float64)).max()
      print(f"{shape} sigma {sigma}: float32 against float64 {gap:.3e}, bound {(4 * r + 6) * EPS:.3e}")
      assert gap <= (4 * r + 6) * EPS, (shape, sigma)
    o, d = images(shape)
    w = P.feather_ref(m, 1.5, np.float32)
    gap = np.abs(P.paste_ref(o, d, w, dtype=np.float32).astype(np.float64) - P.paste_ref(o, d, w)).max()
    assert gap <= 3 * EPS, shape                 # (o - d and the fma: magnitudes below 2)


def test_stats_and_paste_restatement():
  shape = (2, 33, 31, 3)
  m = masks(shape)
  o, d = images(shape)
  hole = ~P.kept(m)
  on, dn = o.copy(), d.copy()
  on[hole], dn[hole] = np.nan, np.nan
  stats = P.keep_stats_ref(on, dn, m)
  assert np.isfinite(stats).all() and np.array_equal(stats, P.keep_stats_ref(o, d, m))
  assert np.array_equal(stats[:, 0, 0], (~hole).sum(axis=(1, 2)))
  # matching d = 0.5 o + 0.25 gives back a = 2, b = -0.5
  a, b = P.gain_offset_ref(P.keep_stats_ref(o, 0.5 * o + 0.25, m))
  assert np.allclose(a, 2., atol=1e-6) and np.allclose(b, -0.5, atol=1e-6)
  # the degenerate cases are the identity: nothing kept, one pixel kept, a flat d
  one = np.zeros_like(m)
  one[:, 3, 4] = 1.
  for mm, dd in ((np.zeros_like(m), d), (one, d), (m, np.full_like(d, 0.25))):
    a, b = P.gain_offset_ref(P.keep_stats_ref(o, dd, mm))
    assert (a == 1).all()
    if not P.kept(mm).any():
      assert (b == 0).all()
  # the paste: kept pixels are o, holes d, whatever o holds in a hole
  for dtype in DTYPES:
    w = P.feather_ref(m, 1.5, dtype)
    out = P.paste_ref(on, d, w, dtype=dtype)
    assert np.isfinite(out).all()
    assert np.array_equal(out[w == 1], o.astype(dtype)[w == 1]) and np.array_equal(out[hole], d.astype(dtype)[hole])
    w0 = P.feather_ref(m, 0., dtype)
    assert np.array_equal(P.paste_ref(on, d, w0, dtype=dtype), np.where(hole[..., None], d, o).astype(dtype))
  neg = np.where(hole[..., None], np.float32(-0.), o)
  assert np.array_equal(np.signbit(P.paste_ref(o, neg, P.feather_ref(m, 0.), dtype=np.float32)[hole]),
                        np.ones((hole.sum(), 3), dtype=bool))


# ---- 3. the loops' rejections, before anything is allocated ---------------------------------------------------
class _FakeModel:
  device = torch.device("cpu")
  skip_lvl = [0, 0, 1, 1, 2, 2, 3]
  _multipliers = (1, 2, 4, 4)


def _fake_sampler():
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), num_steps=1000, beta_start=0.00085,
                                     beta_end=0.012, num_ddim_steps=10)


def test_keyword_rejections_need_no_gpu():
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler as S
  s = _fake_sampler()
  ids = np.zeros((4, 77), dtype=np.int64)
  img = np.zeros((2, 128, 128, 3), dtype=np.float32)
  lm = np.ones((16, 16), dtype=np.float32)
  with pytest.raises(ValueError, match="paste_back.*needs mask"):
    s.ddim_p_sample_loop_img2img(ids, img, paste_back=True)
  loops = (lambda **kw: s.ddim_p_sample_loop_img2img(ids, img, mask=lm, **kw),
           lambda **kw: s.ddim_p_sample_loop_outpaint(ids, img[:, :96, :96], (16, 16, 16, 16), **kw))
  for loop in loops:
    with pytest.raises(ValueError, match="mask_feather.*needs paste_back"):
      loop(mask_feather=2.)
    with pytest.raises(ValueError, match="color_match.*needs paste_back"):
      loop(color_match=True)
    for bad in (-1., 16.5, float("nan"), "2"):
      with pytest.raises(ValueError, match="mask_feather must be"):
        loop(paste_back=True, mask_feather=bad)
    with pytest.raises(ValueError, match="paste_back must be True or False"):
      loop(paste_back="yes")
    with pytest.raises(ValueError, match="color_match must be True or False"):
      loop(paste_back=True, color_match=1)
  with pytest.raises(ValueError, match="neither a latent mask"):
    s.ddim_p_sample_loop_img2img(ids, img, mask=np.ones((2, 17, 16)), paste_back=True)
  assert s._state_key is None and s._graph is None and not s._states
  assert s.last_paste_weights() is None and s.last_color_match() is None
  for name in ("ddim_p_sample_loop_img2img", "ddim_p_sample_loop_outpaint"):
    p = inspect.signature(getattr(S, name)).parameters
    assert (p["paste_back"].default, p["mask_feather"].default, p["color_match"].default) == (False, 0., False)


# ---- 4. the CLI keys ------------------------------------------------------------------------------------------
def _cfg(**keys):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  return yaml.safe_load(yaml.safe_dump(dict(cfg, ldm_sampling=dict(cfg["ldm_sampling"], **keys))))


def test_yaml_keys_bind(tmp_path):
  from ldm_tf2_amd import run_ldm_sampler as Rn
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler as S
  ids = np.zeros((8, 77), dtype=np.int64)
  img, msk = str(tmp_path / "img.npy"), str(tmp_path / "mask.npy")
  base = dict(sample_save_progress=False, latent_shape=[4, 32, 32, 4], init_image=img)
  f = Rn.downsampling_factor(_cfg(**base))
  np.save(img, np.zeros((f * 32, f * 32, 3), dtype=np.uint8))
  np.save(msk, np.ones((f * 32, f * 32), dtype=np.uint8))
  method, _, kwargs = Rn.sampling_call(_cfg(**base, mask=msk), ids, 5)
  assert method == "ddim_p_sample_loop_img2img" and set(kwargs) == {"strength", "seed", "mask"}   # today's call
  method, _, kwargs = Rn.sampling_call(_cfg(**base, mask=msk, paste_back=True, mask_feather=3, color_match=True), ids, 5)
  assert method == "ddim_p_sample_loop_img2img"
  assert (kwargs["paste_back"], kwargs["mask_feather"], kwargs["color_match"]) == (True, 3., True)
  assert isinstance(kwargs["mask_feather"], float)
  assert set(kwargs) <= set(inspect.signature(S.ddim_p_sample_loop_img2img).parameters)
  kwargs = Rn.sampling_call(_cfg(**base, mask=msk, paste_back=True), ids, 5)[2]
  assert kwargs["paste_back"] is True and "mask_feather" not in kwargs and "color_match" not in kwargs
  kwargs = Rn.sampling_call(_cfg(**base, mask=msk, paste_back=False, mask_feather=0, color_match=False), ids, 5)[2]
  assert (kwargs["paste_back"], kwargs["mask_feather"], kwargs["color_match"]) == (False, 0., False)
  np.save(img, np.zeros((f * 32 - 48, f * 32 - 16, 3), dtype=np.uint8))
  method, _, kwargs = Rn.sampling_call(_cfg(**base, outpaint=[16, 32, 0, 16], paste_back=True, mask_feather=1.5), ids, 5)
  assert method == "ddim_p_sample_loop_outpaint"
  assert kwargs == dict(strength=1.0, seed=5, paste_back=True, mask_feather=1.5)
  assert set(kwargs) <= set(inspect.signature(S.ddim_p_sample_loop_outpaint).parameters)


@pytest.mark.parametrize("extra,match", [
    (dict(paste_back=True), "paste_back needs ldm_sampling.mask or ldm_sampling.outpaint"),
    (dict(mask_feather=2.0), "mask_feather needs ldm_sampling.mask or ldm_sampling.outpaint"),
    (dict(color_match=True), "color_match needs ldm_sampling.mask or ldm_sampling.outpaint"),
    (dict(paste_back=True, mask="mask.npy", init_image=None), "paste_back needs ldm_sampling.init_image"),
    (dict(mask_feather=2.0, mask="mask.npy", init_image=None), "mask_feather needs ldm_sampling.init_image"),
    (dict(color_match=True, mask="mask.npy", init_image=None), "color_match needs ldm_sampling.init_image"),
    (dict(paste_back=True, mask="mask.npy", source_prompt="a dog"),
     "paste_back cannot be combined with ldm_sampling.source_prompt"),
    (dict(color_match=True, mask="mask.npy", source_prompt="a dog"),
     "color_match cannot be combined with ldm_sampling.source_prompt"),
    (dict(paste_back=True, mask="mask.npy", window=[16, 16]), "paste_back cannot be combined with ldm_sampling.window"),
    (dict(mask_feather=1.0, mask="mask.npy", window=[16, 16]),
     "mask_feather cannot be combined with ldm_sampling.window"),
    (dict(mask_feather=2.0, mask="mask.npy"), "mask_feather needs ldm_sampling.paste_back"),
    (dict(color_match=True, mask="mask.npy"), "color_match needs ldm_sampling.paste_back"),
    (dict(color_match=True, paste_back=False, mask="mask.npy"), "color_match needs ldm_sampling.paste_back"),
    (dict(paste_back="yes", mask="mask.npy"), "paste_back must be true or false"),
    (dict(paste_back=1, mask="mask.npy"), "paste_back must be true or false"),
    (dict(paste_back=True, color_match="no", mask="mask.npy"), "color_match must be true or false"),
    (dict(paste_back=True, mask_feather=-1, mask="mask.npy"), "mask_feather must be a number"),
    (dict(paste_back=True, mask_feather=16.5, mask="mask.npy"), "mask_feather must be a number"),
    (dict(paste_back=True, mask_feather="4", mask="mask.npy"), "mask_feather must be a number"),
    (dict(paste_back=True, mask_feather=True, mask="mask.npy"), "mask_feather must be a number")])
def test_yaml_rejections_name_the_key(extra, match):
  from ldm_tf2_amd import run_ldm_sampler as Rn
  keys = dict(sample_save_progress=False, latent_shape=[4, 32, 32, 4], init_image="missing.npy")
  keys.update(extra)
  ids = np.zeros((8, 77), dtype=np.int64)
  with pytest.raises(ValueError, match=match):
    Rn.sampling_call(_cfg(**keys), ids, 5, source_ids=ids)


# ---- 5. the declarations --------------------------------------------------------------------------------------
def test_the_new_entries_are_declared_bound_and_exported():
  import ctypes
  from ldm_tf2_amd import _lib, ops
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldm_hip.h")).read(), flags=re.S)
  ctype = {"int": _lib.c_i32, "int64_t": _lib.c_i64, "void*": _lib.c_vp, "const float*": _lib.c_vp,
           "float*": _lib.c_vp, "double*": _lib.c_vp}
  want = {
      "ldm_mask_feather": ["keep", "keep_bstride", "taps", "r", "out", "workspace", "B", "H", "W", "lds_tile", "stream"],
      "ldm_keep_stats": ["o", "d", "keep", "keep_bstride", "partial", "stats", "gain", "offset", "B", "H", "W", "c",
                         "stream"],
      "ldm_paste_back": ["o", "d", "w", "w_bstride", "gain", "offset", "out", "B", "H", "W", "c", "stream"],
  }
  for name, names in want.items():
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    ps = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert [p.rsplit(" ", 1)[1] for p in ps] == names
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_i32 and args == [ctype[p.rsplit(" ", 1)[0]] for p in ps], name
    assert isinstance(getattr(_lib.lib, name), ctypes._CFuncPtr)
  assert re.search(r"\bsize_t\s+ldm_mask_feather_workspace_bytes\s*\(\s*int B,\s*int H,\s*int W\s*\)\s*;", src)
  assert _lib.SIGNATURES["ldm_mask_feather_workspace_bytes"] == (_lib.c_sz, [_lib.c_i32] * 3)
  assert re.search(r"\bint\s+ldm_keep_stats_partials\s*\(\s*int H,\s*int W\s*\)\s*;", src)
  assert _lib.SIGNATURES["ldm_keep_stats_partials"] == (_lib.c_i32, [_lib.c_i32] * 2)
  for name in ("mask_feather", "mask_feather_workspace", "keep_stats", "paste_back"):
    assert name in ops.__all__ and callable(getattr(ops, name))
  assert inspect.signature(ops.mask_feather).parameters["lds_tile"].default is False   # (the form measured faster)
  # the sizes are functions of the shape alone: two erosion / blur planes, and a chunk count that reads H W only
  for B, H, W, _ in SHAPES + [(4, 512, 512, 3)]:
    assert _lib.lib.ldm_mask_feather_workspace_bytes(B, H, W) == 2 * (-(-B * H * W // 4) * 4) * 4
    assert _lib.lib.ldm_keep_stats_partials(H, W) == min(max(-(-H * W // 4096), 1), 1024)
    assert _lib.lib.ldm_keep_stats_partials(W, H) == _lib.lib.ldm_keep_stats_partials(H, W)
  assert _lib.lib.ldm_mask_feather_workspace_bytes(0, 4, 4) == 0 and _lib.lib.ldm_keep_stats_partials(0, 4) == 0
  # a host tensor is refused: there is no CPU fallback
  with pytest.raises(ValueError, match="device tensors"):
    ops.mask_feather(torch.ones(1, 4, 4), 1.)
  with pytest.raises(ValueError, match="device tensors"):
    ops.keep_stats(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 3), torch.ones(1, 4, 4))
  with pytest.raises(ValueError, match="device tensors"):
    ops.paste_back(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 3), torch.ones(1, 4, 4))
