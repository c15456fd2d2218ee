"""Outpainting and masked-content fill, host side: the properties of the push-pull restatement
(tests/pushpull_ref.py) the GPU tests rest on, the canvas geometry, the mask enlargement rule, the rejections and the
CLI keys.

Convex hull.  Every level's value is a weighted mean (pull) or a convex combination (push) of values of the level
before, so in exact arithmetic every output lies between the smallest and the largest kept value.  In floating point a
pull rounds up to five times per element (four fmas and a division), a push up to six (three multiplies, three fmas) and
once more in the blend, each by at most eps/2 relative to a magnitude no larger than max |kept|, and a result passes
through L pulls and L pushes: the bound asserted is the hull widened by 6 (L + 1) eps max|kept|.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import yaml

import pushpull_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
SHAPES = [(1, 1, 1, 3), (1, 1, 9, 4), (2, 5, 7, 3), (2, 16, 16, 4), (2, 33, 31, 3), (2, 37, 53, 4), (1, 64, 48, 3),
          (1, 65, 40, 4)]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]
DTYPES = [np.float64, np.float32]


def inputs(shape, seed=0):
  """x in [-1, 1] and the masks of the GPU tests: sample 0 keeps a centred block (the outpaint shape); sample 1 keeps a
  sparse 5 % of the cells plus the corner, and its lower right quadrant has weight 0.5."""
  B, H, W, c = shape
  g = np.random.default_rng([seed, B, H, W, c])
  x = g.uniform(-1., 1., shape).astype(np.float32)
  m = np.zeros((B, H, W), dtype=np.float32)
  m[0, H // 4:H // 4 + max(H // 2, 1), W // 4:W // 4 + max(W // 2, 1)] = 1.
  if B > 1:
    m[1] = g.random((H, W)) < 0.05
    m[1, 0, 0] = 1.
    m[1, H // 2:, W // 2:] = 0.5
  return x, m


# ---- 1. the restatement's properties ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kept_cells_bit_equal_and_convex_hull(shape, dtype):
  x, m = inputs(shape)
  out = P.pushpull_ref(x, m, dtype)
  assert out.dtype == dtype and out.shape == x.shape
  kept = m == 1
  assert np.array_equal(out[kept], x.astype(dtype)[kept])
  L = len(P.pyramid_extents(*shape[1:3])) - 1
  for b in range(shape[0]):
    vals = x[b][m[b] > 0].astype(np.float64)
    slack = 6 * (L + 1) * np.finfo(dtype).eps * np.abs(vals).max()
    lo, hi = vals.min(axis=0) - slack, vals.max(axis=0) + slack          # per channel
    assert (out[b] >= lo).all() and (out[b] <= hi).all(), (b, out[b].min(axis=(0, 1)) - lo, hi - out[b].max(axis=(0, 1)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_degenerate_masks_and_holes(shape, dtype):
  x, m = inputs(shape)
  zeros = P.pushpull_ref(x, np.zeros_like(m), dtype)
  assert not zeros.any() and not np.signbit(zeros).any()
  assert np.array_equal(P.pushpull_ref(x, np.ones_like(m), dtype), x.astype(dtype))
  # a NaN in m counts as 0; values outside [0, 1] are clamped
  odd = m.copy()
  odd[m == 0] = np.nan
  odd[m == 1] = 7.
  assert np.array_equal(P.pushpull_ref(x, odd, dtype), P.pushpull_ref(x, m, dtype))
  neg = m.copy()
  neg[m == 0] = -3.
  assert np.array_equal(P.pushpull_ref(x, neg, dtype), P.pushpull_ref(x, m, dtype))
  # what a hole holds does not matter: NaN there gives what zeros give
  holes = m == 0
  xn, xz = x.copy(), x.copy()
  xn[holes] = np.nan
  xz[holes] = 0.
  got = P.pushpull_ref(xn, m, dtype)
  assert np.isfinite(got).all() and np.array_equal(got, P.pushpull_ref(xz, m, dtype))
  assert np.array_equal(got, P.pushpull_ref(x, m, dtype))


def probe_positions(H, W):
  """The four corners and the centre."""
  return sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)})


def probe_inputs(shape, pos):
  """One kept pixel per sample at `pos` with the value k/8, k distinct per sample and channel; NaN in every hole.
  Returns (x, m, the value per sample and channel [B,c])."""
  B, H, W, c = shape
  val = (np.arange(B * c, dtype=np.float32).reshape(B, c) - 3) / 8
  x = np.full(shape, np.nan, dtype=np.float32)
  m = np.zeros((B, H, W), dtype=np.float32)
  x[:, pos[0], pos[1]] = val
  m[:, pos[0], pos[1]] = 1.
  return x, m, val


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_kept_pixel_gives_a_constant_image(shape, dtype):
  """Every product of the rule is exact for k/8: the weights are 0 and 1, the taps 3/4 and 1/4 of equal values."""
  for pos in probe_positions(*shape[1:3]):
    x, m, val = probe_inputs(shape, pos)
    want = np.broadcast_to(val[:, None, None, :].astype(dtype), shape)
    assert np.array_equal(P.pushpull_ref(x, m, dtype), want), pos


def test_pyramid_extents():
  assert P.pyramid_extents(1, 1) == [(1, 1)]
  assert P.pyramid_extents(1, 9) == [(1, 9), (1, 5), (1, 3), (1, 2), (1, 1)]
  assert P.pyramid_extents(33, 31) == [(33, 31), (17, 16), (9, 8), (5, 4), (3, 2), (2, 1), (1, 1)]
  assert P.pyramid_extents(256, 256)[3] == (32, 32) and len(P.pyramid_extents(256, 256)) == 9
  for H, W in [s[1:3] for s in SHAPES] + [(128, 3), (1000, 7)]:
    ext = P.pyramid_extents(H, W)
    assert len(ext) - 1 == int(np.ceil(np.log2(max(H, W))))
    assert all(ext[l] == (-(-H >> l), -(-W >> l)) for l in range(len(ext)))


def test_float32_against_float64_gap():
  """The figure the GPU test scales its bound by, on the same inputs, within the rounding budget of the module
  docstring: 6 (L + 1) eps for values in [-1, 1]."""
  for shape in SHAPES:
    x, m = inputs(shape)
    L = len(P.pyramid_extents(*shape[1:3])) - 1
    gap = np.abs(P.pushpull_ref(x, m, np.float32).astype(np.float64) - P.pushpull_ref(x, m, np.float64)).max()
    print(f"{shape}: float32 against float64 {gap:.3e}")
    assert gap <= 6 * (L + 1) * np.finfo(np.float32).eps, shape


def test_workspace_size_matches_the_pyramid():
  from ldm_tf2_amd import _lib
  for B, H, W, c in SHAPES + [(4, 256, 256, 3)]:
    ext = P.pyramid_extents(H, W)[1:]
    want = sum(-(-B * h * w * c // 4) * 4 + -(-B * h * w // 4) * 4 for h, w in ext) * 4
    assert _lib.lib.ldm_pushpull_workspace_bytes(B, H, W, c) == want
  assert _lib.lib.ldm_pushpull_workspace_bytes(0, 4, 4, 3) == 0


# ---- 2. the canvas ------------------------------------------------------------------------------------------
def test_outpaint_geometry():
  from ldm_tf2_amd.model_runners import outpaint_geometry as G
  assert G((96, 96), (16, 16, 16, 16), 8) == ((128, 128), (16, 16, 96, 96))
  assert G((96, 96), (0, 32, 8, 24), 8, 8) == ((128, 128), (0, 8, 96, 96))
  assert G((100, 60), (28, 0, 0, 4), 8) == ((128, 64), (28, 0, 100, 60))
  assert G([5, 7], [0, 0, 0, 1], 1) == ((5, 8), (0, 0, 5, 7))
  for bad in ((0, 0, 0, 0), (-8, 24, 16, 16), (16, 16, 16), (16, 16, 16, 16, 16), 16, (16.5, 15.5, 16, 16),
              (True, 31, 16, 16)):
    with pytest.raises(ValueError, match="pad"):
      G((96, 96), bad, 8)
  for bad in ((96,), 96, (0, 96), (96.5, 96)):
    with pytest.raises(ValueError, match="image_hw"):
      G(bad, (16, 16, 16, 16), 8)
  with pytest.raises(ValueError, match="multiples of 8"):
    G((96, 96), (16, 17, 16, 16), 8)
  with pytest.raises(ValueError, match="multiples of 8"):
    G((96, 96), (16, 16, 4, 0), 8)
  with pytest.raises(ValueError, match="multiples of 64"):
    G((96, 96), (8, 8, 16, 16), 8, 8)             # 112 x 128: a latent extent of 14 does not halve three times


# ---- 3. the mask enlargement rule ---------------------------------------------------------------------------
def test_fill_keep_mask():
  from ldm_tf2_amd.model_runners import fill_keep_mask, latent_mask, latent_mask_fit
  from ldm_tf2_amd.resample import crop_box
  g = np.random.default_rng(5)
  # a latent mask: every cell's value over its f x f pixels, fractions included
  lat = g.random((2, 4, 6)).astype(np.float32)
  lat[0, :2] = 1.
  lat[1, :, 3:] = 0.
  keep = fill_keep_mask(lat, (32, 48), (32, 48), 8)
  assert keep.dtype == np.float32 and keep.shape == (2, 32, 48)
  assert all(np.array_equal(keep[:, y, x], lat[:, y // 8, x // 8]) for y in range(32) for x in range(48))
  assert np.array_equal(latent_mask(keep == 1, 8), (lat == 1).astype(np.float32))
  assert fill_keep_mask(lat[0], (100, 60), (32, 48), 8).shape == (1, 32, 48)        # [h,w]; the source size is not read
  assert fill_keep_mask(torch.from_numpy(lat), (32, 48), (32, 48), 8).shape == (2, 32, 48)
  # a pixel mask already at the canvas size: itself, as 0 / 1
  pm = (g.random((2, 32, 48)) < 0.7) * 3
  assert np.array_equal(fill_keep_mask(pm, (32, 48), (32, 48), 8), (pm != 0).astype(np.float32))
  # a pixel mask at another size: a canvas pixel is kept exactly where every source pixel it covers is
  for src, size, fit in (((40, 56), (32, 48), "stretch"), ((20, 100), (32, 48), "stretch"), ((40, 56), (32, 48), "crop"),
                         ((90, 50), (32, 48), "crop")):
    pm = g.random((2,) + src) < 0.8
    keep = fill_keep_mask(pm, src, size, 8, fit)
    y0, x0, hc, wc = crop_box(src, size) if fit == "crop" else (0, 0) + src
    box = pm[:, y0:y0 + hc, x0:x0 + wc]
    want = np.empty((2,) + size, dtype=np.float32)
    for y in range(size[0]):
      for x in range(size[1]):
        rows = slice((y * hc) // size[0], -((-(y + 1) * hc) // size[0]))
        cols = slice((x * wc) // size[1], -((-(x + 1) * wc) // size[1]))
        want[:, y, x] = box[:, rows, cols].all(axis=(1, 2))
    assert np.array_equal(keep, want), (src, size, fit)
    # nothing the latent mask of the same call keeps is filled
    lm = latent_mask_fit(box, (size[0] // 8, size[1] // 8))
    assert (np.repeat(np.repeat(lm, 8, 1), 8, 2) <= keep).all()
  for bad in (np.ones((2, 5, 6)), np.ones((2, 2, 4, 6)), np.ones(6)):
    with pytest.raises(ValueError, match="neither a latent mask"):
      fill_keep_mask(bad, (40, 56), (32, 48), 8)
  with pytest.raises(ValueError, match="multiples of 8"):
    fill_keep_mask(lat, (32, 48), (33, 48), 8)


# ---- 4. the loops' rejections, before anything is allocated -----------------------------------------------
class _FakeModel:
  device = torch.device("cpu")
  skip_lvl = [0, 0, 1, 1, 2, 2, 3]               # (a U-Net that halves its input three times)
  _multipliers = (1, 2, 4, 4)                    # (an autoencoder with 8 pixels per latent cell)


def _fake_sampler():
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), num_steps=1000, beta_start=0.00085,
                                     beta_end=0.012, num_ddim_steps=10)


def test_rejections_need_no_gpu():
  from ldm_tf2_amd.model_runners import MASKED_CONTENTS, LatentDiffusionModelSampler as S
  assert MASKED_CONTENTS == ("original", "fill")
  s = _fake_sampler()
  ids = np.zeros((4, 77), dtype=np.int64)
  img = np.zeros((2, 128, 128, 3), dtype=np.float32)
  with pytest.raises(ValueError, match="needs mask"):
    s.ddim_p_sample_loop_img2img(ids, img, masked_content="fill")
  for loop in (lambda **kw: s.ddim_p_sample_loop_img2img(ids, img, mask=np.ones((16, 16)), **kw),
               lambda **kw: s.ddim_p_sample_loop_outpaint(ids, img[:, :96, :96], (16, 16, 16, 16), **kw)):
    with pytest.raises(ValueError, match="masked_content"):
      loop(masked_content="noise")
  with pytest.raises(ValueError, match="neither a latent mask"):
    s.ddim_p_sample_loop_img2img(ids, img, mask=np.ones((2, 17, 16)), masked_content="fill")
  small = img[:, :96, :96]
  with pytest.raises(ValueError, match="multiples of 64"):
    s.ddim_p_sample_loop_outpaint(ids, small, (16, 16, 16, 8))
  with pytest.raises(ValueError, match="pad"):
    s.ddim_p_sample_loop_outpaint(ids, small, (0, 0, 0, 0))
  with pytest.raises(ValueError, match="strength"):
    s.ddim_p_sample_loop_outpaint(ids, small, (16, 16, 16, 16), strength=0.)
  with pytest.raises(ValueError, match="init_images"):
    s.ddim_p_sample_loop_outpaint(ids, np.zeros((3, 96, 96, 3), dtype=np.float32), (16, 16, 16, 16))
  assert s._state_key is None and s._graph is None and not s._states and s._gtab is None
  p = inspect.signature(S.ddim_p_sample_loop_img2img).parameters
  assert p["masked_content"].default == "original"
  p = inspect.signature(S.ddim_p_sample_loop_outpaint).parameters
  assert (p["masked_content"].default, p["strength"].default, p["guidance_scale"].default) == ("fill", 1.0, 5.)


# ---- 5. the CLI keys --------------------------------------------------------------------------------------
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
  np.save(img, np.zeros((f * 32 - 48, f * 32 - 16, 3), dtype=np.uint8))
  cfg = _cfg(**base, outpaint=[16, 32, 0, 16])
  method, args, kwargs = Rn.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop_outpaint" and Rn.needs_encoder(cfg)
  assert args[0] is ids and args[1].shape == (f * 32 - 48, f * 32 - 16, 3) and args[2] == (16, 32, 0, 16)
  assert args[3] == cfg["ldm_sampling"]["guidance_scale"] and kwargs == dict(strength=1.0, seed=5)
  kwargs = Rn.sampling_call(_cfg(**base, outpaint=[16, 32, 0, 16], masked_content="original", strength=0.9,
                                 guidance_interval=[100, 900], preview_freq=2), ids, 5)[2]
  assert kwargs == dict(strength=0.9, seed=5, masked_content="original", guidance_interval=(100, 900), preview_freq=2)
  assert set(kwargs) <= set(inspect.signature(S.ddim_p_sample_loop_outpaint).parameters)
  assert Rn.sampling_call(_cfg(**base, outpaint=[16, 32, 0, 16], masked_content="fill"), ids, 5)[2][
      "masked_content"] == "fill"
  with pytest.raises(ValueError, match="latent_shape needs"):
    Rn.sampling_call(_cfg(**base, outpaint=[16, 16, 0, 16]), ids, 5)
  # masked_content on the img2img loop; without the key the call is today's
  np.save(img, np.zeros((f * 32, f * 32, 3), dtype=np.uint8))
  np.save(msk, np.ones((f * 32, f * 32), dtype=np.uint8))
  method, _, kwargs = Rn.sampling_call(_cfg(**base, mask=msk), ids, 5)
  assert method == "ddim_p_sample_loop_img2img" and set(kwargs) == {"strength", "seed", "mask"}
  for mc in ("fill", "original"):
    method, _, kwargs = Rn.sampling_call(_cfg(**base, mask=msk, masked_content=mc), ids, 5)
    assert method == "ddim_p_sample_loop_img2img" and kwargs["masked_content"] == mc
    assert set(kwargs) <= set(inspect.signature(S.ddim_p_sample_loop_img2img).parameters)
  assert Rn.sampling_call(_cfg(**base, masked_content="original"), ids, 5)[2]["masked_content"] == "original"


@pytest.mark.parametrize("extra,match", [
    (dict(outpaint=[16, 16, 16]), "outpaint must be"), (dict(outpaint=16), "outpaint must be"),
    (dict(outpaint=[0, 0, 0, 0]), "outpaint must be"), (dict(outpaint=[16, -16, 16, 16]), "outpaint must be"),
    (dict(outpaint=[16, 16.0, 16, 16]), "outpaint must be"), (dict(outpaint=[True, 16, 16, 16]), "outpaint must be"),
    (dict(outpaint=[16, 16, 16, 16], init_image=None), "outpaint needs ldm_sampling.init_image"),
    (dict(outpaint=[16, 16, 16, 16], mask="mask.npy"), "outpaint cannot be combined with ldm_sampling.mask"),
    (dict(outpaint=[16, 16, 16, 16], window=[16, 16]), "outpaint cannot be combined with ldm_sampling.window"),
    (dict(outpaint=[16, 16, 16, 16], hires_shape=[4, 64, 64, 4]),
     "outpaint cannot be combined with ldm_sampling.hires_shape"),
    (dict(outpaint=[16, 16, 16, 16], source_prompt="a dog"),
     "outpaint cannot be combined with ldm_sampling.source_prompt"),
    (dict(outpaint=[16, 16, 16, 16], sample_save_progress=True),
     "outpaint cannot be combined with ldm_sampling.sample_save_progress"),
    (dict(outpaint=[16, 16, 16, 16], init_fit="stretch"), "outpaint cannot be combined with ldm_sampling.init_fit"),
    (dict(masked_content="noise"), "masked_content must be one of"),
    (dict(masked_content="fill"), "masked_content 'fill' needs"),
    (dict(masked_content="fill", init_image=None), "masked_content needs ldm_sampling.init_image"),
    (dict(masked_content="original", init_image=None), "masked_content needs ldm_sampling.init_image"),
    (dict(masked_content="fill", mask="mask.npy", source_prompt="a dog"),
     "masked_content cannot be combined with ldm_sampling.source_prompt")])
def test_yaml_rejections_name_the_key(extra, match):
  from ldm_tf2_amd import run_ldm_sampler as Rn
  keys = dict(sample_save_progress=False, latent_shape=[4, 32, 32, 4], init_image="missing.npy")
  keys.update(extra)
  ids = np.zeros((8, 77), dtype=np.int64)
  with pytest.raises(ValueError, match=match):
    Rn.sampling_call(_cfg(**keys), ids, 5, source_ids=ids)


def test_the_new_entries_are_declared_bound_and_exported():
  import ctypes
  from ldm_tf2_amd import _lib, ops
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldm_hip.h")).read(), flags=re.S)
  ctype = {"int": _lib.c_i32, "void*": _lib.c_vp, "const float*": _lib.c_vp, "float*": _lib.c_vp}
  m = re.search(r"\bint\s+ldm_pushpull_fill\s*\(([^)]*)\)\s*;", src)
  assert m
  ps = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
  assert [p.rsplit(" ", 1)[1] for p in ps] == ["x", "keep", "out", "workspace", "B", "H", "W", "c", "lds_tail", "stream"]
  res, args = _lib.SIGNATURES["ldm_pushpull_fill"]
  assert res is _lib.c_i32 and args == [ctype[p.rsplit(" ", 1)[0]] for p in ps]
  assert re.search(r"\bsize_t\s+ldm_pushpull_workspace_bytes\s*\(\s*int B,\s*int H,\s*int W,\s*int c\s*\)\s*;", src)
  assert _lib.SIGNATURES["ldm_pushpull_workspace_bytes"] == (_lib.c_sz, [_lib.c_i32] * 4)
  assert isinstance(_lib.lib.ldm_pushpull_fill, ctypes._CFuncPtr)
  assert "pushpull_fill" in ops.__all__
  # a host tensor is refused: there is no CPU fallback
  with pytest.raises(ValueError, match="device tensors"):
    ops.pushpull_fill(torch.zeros(1, 4, 4, 3), torch.ones(1, 4, 4))
