"""The antialiased resample, host side: the float64 restatement (tests/resample_ref.py) against
torch's antialias=True and PIL, the tables the device reads, the mask and crop rules, the rejections and the CLI keys."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
TORCH_MODE = {"triangle": "bilinear", "cubic": "bicubic"}


def _x(shape, seed=0):
  return np.random.default_rng(seed).uniform(-1., 1., shape)


# ---- 1. the rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TORCH_MODE))
@pytest.mark.parametrize("src,dst", R.SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.SHAPES])
def test_restatement_against_torch_antialias(src, dst, name):
  """float64 on both sides: 1e-13 (2.7e-15 was measured over these shapes)."""
  x = _x((2,) + src + (3,))
  want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=dst, mode=TORCH_MODE[name],
                                         antialias=True, align_corners=False).permute(0, 2, 3, 1).numpy()
  err = np.abs(R.resample64(x, dst, name) - want).max()
  print(f"{name} {src}->{dst}: {err:.3e}")
  assert err <= 1e-13


@pytest.mark.parametrize("src,dst", R.SHAPES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in R.SHAPES])
def test_lanczos_against_pil(src, dst):
  """PIL computes mode "F" in float32: 1e-6 (5.4e-8 was measured)."""
  Image = pytest.importorskip("PIL.Image")
  x = _x((1,) + src + (1,)).astype(np.float32)
  want = np.asarray(Image.fromarray(x[0, :, :, 0], mode="F").resize((dst[1], dst[0]), Image.LANCZOS))
  err = np.abs(R.resample64(x, dst, "lanczos3")[0, :, :, 0] - want).max()
  print(f"lanczos3 {src}->{dst}: {err:.3e}")
  assert err <= 1e-6


# ---- 2. the tables ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FILTERS)
def test_table_invariants(name):
  from ldm_tf2_amd import _lib
  from ldm_tf2_amd.resample import axis_weights, resample_taps
  assert _lib.RESAMPLE_FILTERS == R.FILTERS
  axes = sorted({(s[k], d[k]) for s, d in R.SHAPES for k in (0, 1)} | {(1, 7), (7, 1), (2, 3), (1, 1)})
  for L, Lo in axes:
    start, w, T = resample_taps(L, Lo, name)
    rows = R.axis_rows(L, Lo, name)
    assert start.dtype == np.int32 and w.dtype == np.float32 and start.shape == (Lo,) and w.shape == (Lo, T)
    assert T == max(len(r[1]) for r in rows) and 1 <= T <= L
    assert start.min() >= 0 and start.max() <= L - T, (L, Lo)
    assert np.abs(w.astype(np.float64).sum(1) - 1.).max() <= 2.0 ** -22, (L, Lo)
    own = axis_weights(L, Lo, name)
    dense, dense64 = np.zeros((Lo, L), dtype=np.float32), np.zeros((Lo, L), dtype=np.float64)
    for i in range(Lo):
      xmin, w64 = rows[i]
      px, pw = own[i]
      assert px == xmin and len(pw) == len(w64) and start[i] == min(xmin, L - T)
      dense[i, start[i]:start[i] + T] = w[i]                    # the shifted, zero-filled row ...
      assert np.array_equal(dense[i, xmin:xmin + len(pw)], pw.astype(np.float32))       # ... is the unshifted one
      assert np.count_nonzero(dense[i]) == np.count_nonzero(pw.astype(np.float32))
      dense64[i, xmin:xmin + len(w64)] = w64
    # against the restatement, which evaluates the filters in another form: one rounding to float32 of weights
    # that agree to a few float64 ulps
    assert np.all(np.abs(dense.astype(np.float64) - dense64) <= 2.0 ** -24 * np.abs(dense64) + 1e-15), (L, Lo)
    rs, _, rT = R.tables32(L, Lo, name)
    assert rT == T and np.array_equal(rs, start)
    if Lo == L:
      assert T == 1 and np.array_equal(start, np.arange(L)) and np.all(w == 1.)


def test_emulation_is_close_and_the_identity_is_a_copy():
  x = _x((2, 9, 7, 3)).astype(np.float32)
  x.flat[0], x.flat[1] = -0.0, np.nan
  for name in R.FILTERS:
    same = R.resample32(x, (9, 7), name)
    assert np.array_equal(same.view(np.uint32), x.view(np.uint32))
    y = _x((2, 37, 53, 3), 1).astype(np.float32)
    err = np.abs(R.resample32(y, (16, 24), name) - R.resample64(y, (16, 24), name)).max()
    assert err <= 32 * 2.0 ** -24 * 2., (name, err)             # (<= 24 taps per axis, |w| sums below 2, |x| <= 1)


def test_unknown_filter_and_bad_extents():
  from ldm_tf2_amd import ops
  from ldm_tf2_amd.resample import resample_taps
  with pytest.raises(ValueError, match="filter"):
    resample_taps(8, 4, "box")
  with pytest.raises(ValueError, match="positive"):
    resample_taps(8, 0, "cubic")
  with pytest.raises(ValueError, match="resample filter"):
    ops.resample_nhwc(torch.zeros(1, 4, 4, 3), (2, 2), "lanczos")
  with pytest.raises(ValueError, match="positive"):
    ops.resample_nhwc(torch.zeros(1, 4, 4, 3), (0, 2), "cubic")
  with pytest.raises(ValueError, match="device tensors"):
    ops.resample_nhwc(torch.zeros(1, 4, 4, 3), (2, 2), "cubic")


# ---- 3. masks and crop boxes ------------------------------------------------------------------------------
def test_latent_mask_fit():
  from ldm_tf2_amd.model_runners import latent_mask, latent_mask_fit
  g = np.random.default_rng(4)
  for f, (h, w) in ((8, (4, 6)), (4, (5, 3)), (1, (7, 7))):
    m = (g.random((3, f * h, f * w)) < 0.97).astype(np.uint8) * 3
    assert np.array_equal(latent_mask_fit(m, (h, w)), latent_mask(m, f))
    assert np.array_equal(latent_mask_fit(m[0], (h, w)), latent_mask(m[0], f))
    assert np.array_equal(latent_mask_fit(torch.from_numpy(m), (h, w)), latent_mask(m, f))
  # 10 -> 4: the cells cover rows 0-2, 2-4, 5-7, 7-9 (row 2 and row 7 each belong to two cells)
  cover = [(0, 2), (2, 4), (5, 7), (7, 9)]
  for r in range(10):
    m = np.ones((10, 10), dtype=np.float32)
    m[r, :] = 0.
    want = np.array([0. if lo <= r <= hi else 1. for lo, hi in cover], dtype=np.float32)
    got = latent_mask_fit(m, (4, 4))
    assert got.shape == (1, 4, 4) and got.dtype == np.float32
    assert np.array_equal(got[0], np.tile(want[:, None], (1, 4))), r
    assert np.array_equal(latent_mask_fit(m.T, (4, 4))[0], np.tile(want[None, :], (4, 1))), r
  one = np.ones((1, 3, 5))                                       # fewer pixels than cells: every cell covers a pixel
  one[0, 1, 2] = 0
  got = latent_mask_fit(one, (6, 10))[0]
  assert got.shape == (6, 10) and np.array_equal(np.argwhere(got == 0), [[2, 4], [2, 5], [3, 4], [3, 5]])
  with pytest.raises(ValueError):
    latent_mask_fit(np.ones((2, 3, 4, 5)), (2, 2))
  # latent_mask itself is as it was
  with pytest.raises(ValueError, match="multiples"):
    latent_mask(np.ones((10, 10)), 4)


def test_crop_boxes():
  from ldm_tf2_amd.resample import crop_box
  assert crop_box((40, 56), (128, 128)) == (0, 8, 40, 40)       # wide source: columns go
  assert crop_box((56, 40), (128, 128)) == (8, 0, 40, 40)       # tall source: rows go
  assert crop_box((300, 450), (256, 384)) == (0, 0, 300, 450)   # the same aspect ratio: everything stays
  assert crop_box((100, 301), (64, 128)) == (0, 50, 100, 200)
  assert crop_box((7, 1000), (512, 64)) == (0, 499, 7, 1)       # (7 * 64 + 256) // 512 = 1: at least one column
  assert crop_box((1000, 3), (64, 512)) == (499, 0, 1, 3)
  g = np.random.default_rng(0)
  for _ in range(200):
    src, dst = tuple(g.integers(1, 600, 2)), tuple(g.integers(1, 600, 2))
    box = crop_box(src, dst)
    assert box == R.crop_box(tuple(int(v) for v in src), tuple(int(v) for v in dst))
    y0, x0, hc, wc = box
    assert 0 <= y0 and y0 + hc <= src[0] and 0 <= x0 and x0 + wc <= src[1] and hc >= 1 and wc >= 1
    assert (hc == src[0]) or (wc == src[1])


# ---- 4. the loops' rejections, before anything is allocated -----------------------------------------------
class _FakeModel:
  device = torch.device("cpu")
  skip_lvl = [0, 0, 1, 1, 2, 2, 3]               # (a U-Net that halves its input three times)
  _multipliers = (1, 2, 4, 4)                    # (an autoencoder with 8 pixels per latent cell)

  def __init__(self, **kw):
    self.__dict__.update(kw)


def _fake_sampler(autoencoder=None):
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), autoencoder or _FakeModel(), _FakeModel(), num_steps=1000,
                                     beta_start=0.00085, beta_end=0.012, num_ddim_steps=10)


def test_image_size_rejections_need_no_gpu():
  s = _fake_sampler()
  ids = np.zeros((4, 77), dtype=np.int64)
  img = np.zeros((2, 40, 56, 3), dtype=np.float32)
  loops = [lambda **kw: s.ddim_p_sample_loop_img2img(ids, img, **kw),
           lambda **kw: s.ddim_invert_loop(ids, init_images=img, **kw),
           lambda **kw: s.ddim_p_sample_loop_edit(ids, ids, img, **kw)]
  for loop in loops:
    for bad in ((128, 100), (96, 128), (0, 128), (-64, 64)):
      with pytest.raises(ValueError, match="multiples of 64"):
        loop(image_size=bad)
    for bad in ((128,), 128, (128.5, 128)):
      with pytest.raises(ValueError, match="image_size"):
        loop(image_size=bad)
    with pytest.raises(ValueError, match="fit"):
      loop(image_size=(128, 128), fit="exact")
    with pytest.raises(ValueError, match="resample"):
      loop(image_size=(128, 128), resample="lanczos")
  with pytest.raises(ValueError, match="latents"):
    s.ddim_invert_loop(ids, latents=np.zeros((2, 16, 16, 4), dtype=np.float32), image_size=(128, 128))
  assert s._state_key is None and s._graph is None and not s._states and s._gtab is None
  # a mask that is neither form (checked on the host, against the images' and the latents' extents)
  for bad in (np.ones((2, 40, 40)), np.ones((17, 16)), np.ones((2, 2, 40, 56))):
    with pytest.raises(ValueError, match="neither a latent mask"):
      s._fit_mask(bad, (40, 56), (128, 128), "crop")
  lat = np.ones((2, 16, 16), dtype=np.float32)
  assert s._fit_mask(lat, (40, 56), (128, 128), "crop") is lat
  pm = np.ones((40, 56))
  pm[:, 7] = 0                                    # outside the crop box (columns 8 .. 47): nothing is regenerated
  assert np.array_equal(s._fit_mask(pm, (40, 56), (128, 128), "crop"), np.ones((16, 16), dtype=np.float32))
  assert not s._fit_mask(pm, (40, 56), (128, 128), "stretch").all()
  assert s._fit_mask(np.stack([pm, pm]), (40, 56), (128, 128), "stretch").shape == (2, 16, 16)


def test_pixel_filter_rejections_need_no_gpu():
  ids = np.zeros((4, 77), dtype=np.int64)
  lo, hi = [2, 16, 16, 4], [2, 32, 32, 4]
  with pytest.raises(ValueError, match="without its encoder"):
    _fake_sampler(_FakeModel(_encoder=None)).ddim_p_sample_loop_hires(ids, lo, hi, pixel_filter="cubic")
  s = _fake_sampler(_FakeModel(_encoder=object(), _latent_size=16))
  with pytest.raises(ValueError, match="one latent size"):
    s.ddim_p_sample_loop_hires(ids, lo, hi, pixel_filter="cubic")
  s = _fake_sampler(_FakeModel(_encoder=object()))
  with pytest.raises(ValueError, match="pixel_filter"):
    s.ddim_p_sample_loop_hires(ids, lo, hi, pixel_filter="bicubic")
  for pf in (None, "cubic"):                      # (the latent resize's own check stays in front)
    with pytest.raises(ValueError, match="resize"):
      s.ddim_p_sample_loop_hires(ids, lo, hi, resize="lanczos", pixel_filter=pf)
  with pytest.raises(ValueError, match="encode_noise"):
    s.ddim_p_sample_loop_hires(ids, lo, hi, encode_noise=np.zeros(hi, dtype=np.float32))
  assert s._state_key is None and s._graph is None and not s._states and s._gtab is None


# ---- 5. the CLI keys --------------------------------------------------------------------------------------
def _cfg(**keys):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  return yaml.safe_load(yaml.safe_dump(dict(cfg, ldm_sampling=dict(cfg["ldm_sampling"], **keys))))


def test_yaml_keys_bind(tmp_path):
  import inspect
  from ldm_tf2_amd import run_ldm_sampler as Rn
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler as S
  from ldm_tf2_amd.model_runners import latent_mask
  ids = np.zeros((8, 77), dtype=np.int64)
  img, msk = str(tmp_path / "img.npy"), str(tmp_path / "mask.npy")
  np.save(img, np.zeros((300, 450, 3), dtype=np.uint8))
  pm = np.ones((300, 450), dtype=np.uint8)
  pm[:10] = 0
  np.save(msk, pm)
  base = dict(sample_save_progress=False, latent_shape=[4, 32, 32, 4], init_image=img)
  f = Rn.downsampling_factor(_cfg(**base))
  # defaults: today's calls
  for extra in ({}, dict(init_fit="exact"), dict(init_fit="exact", init_filter="cubic")):
    method, args, kwargs = Rn.sampling_call(_cfg(**base, **extra), ids, 5)
    assert method == "ddim_p_sample_loop_img2img" and kwargs == dict(strength=0.75, seed=5)
  np.save(msk, np.ones((f * 32, f * 32), dtype=np.uint8))
  kwargs = Rn.sampling_call(_cfg(**base, mask=msk), ids, 5)[2]
  assert np.array_equal(kwargs["mask"], latent_mask(np.ones((f * 32, f * 32)), f)[0]) and "image_size" not in kwargs
  plain = _cfg(sample_save_progress=False)
  assert Rn.sampling_call(plain, ids, 5)[2] == dict(seed=5) and not Rn.needs_encoder(plain)
  # stretch / crop: the target is f * the latent extents; a pixel mask goes to the loop as it is
  np.save(msk, pm)
  cfg = _cfg(**dict(base, latent_shape=[4, 32, 48, 4]), init_fit="crop", mask=msk)
  method, args, kwargs = Rn.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop_img2img" and args[1].shape == (300, 450, 3)
  assert kwargs["image_size"] == (f * 32, f * 48) and kwargs["fit"] == "crop" and kwargs["resample"] == "lanczos3"
  assert np.array_equal(kwargs["mask"], pm)
  assert set(kwargs) <= set(inspect.signature(S.ddim_p_sample_loop_img2img).parameters)
  kwargs = Rn.sampling_call(_cfg(**base, init_fit="stretch", init_filter="triangle"), ids, 5)[2]
  assert (kwargs["fit"], kwargs["resample"], kwargs["image_size"]) == ("stretch", "triangle", (f * 32, f * 32))
  method, args, kwargs = Rn.sampling_call(_cfg(**base, init_fit="stretch", source_prompt="a dog"), ids, 5, source_ids=ids)
  assert method == "ddim_p_sample_loop_edit" and kwargs["fit"] == "stretch" and kwargs["image_size"] == (f * 32, f * 32)
  assert set(kwargs) <= set(inspect.signature(S.ddim_p_sample_loop_edit).parameters)
  assert Rn.sampling_call(_cfg(**base, source_prompt="a dog"), ids, 5, source_ids=ids)[2] == dict(
      strength=0.75, invert_guidance_scale=1., seed=5)
  # the two-pass loop in pixel space
  hires = dict(sample_save_progress=False, latent_shape=[4, 32, 32, 4], hires_shape=[4, 64, 64, 4])
  assert "pixel_filter" not in Rn.sampling_call(_cfg(**hires), ids, 5)[2] and not Rn.needs_encoder(_cfg(**hires))
  cfg = _cfg(**hires, hires_pixel_filter="cubic")
  method, args, kwargs = Rn.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop_hires" and kwargs["pixel_filter"] == "cubic" and Rn.needs_encoder(cfg)
  assert set(kwargs) <= set(inspect.signature(S.ddim_p_sample_loop_hires).parameters)
  for name in ("ddim_p_sample_loop_img2img", "ddim_invert_loop", "ddim_p_sample_loop_edit"):
    p = inspect.signature(getattr(S, name)).parameters
    assert (p["image_size"].default, p["fit"].default, p["resample"].default) == (None, "stretch", "lanczos3")
  p = inspect.signature(S.ddim_p_sample_loop_hires).parameters
  assert p["pixel_filter"].default is None and p["encode_noise"].default is None


@pytest.mark.parametrize("extra,match", [
    (dict(init_fit="fill"), "init_fit"), (dict(init_filter="lanczos"), "init_filter"),
    (dict(init_fit="crop", init_filter="bicubic"), "init_filter"),
    (dict(hires_shape=[4, 64, 64, 4], hires_pixel_filter="bicubic", init_image=None), "hires_pixel_filter"),
    (dict(hires_pixel_filter="cubic", init_image=None), "hires_shape")])
def test_yaml_unknown_values_name_the_key(extra, match):
  from ldm_tf2_amd import run_ldm_sampler as Rn
  keys = dict(sample_save_progress=False, latent_shape=[4, 32, 32, 4], init_image="missing.npy")
  keys.update(extra)
  with pytest.raises(ValueError, match=match):
    Rn.sampling_call(_cfg(**keys), np.zeros((8, 77), dtype=np.int64), 5)


def test_the_new_entry_is_declared_bound_and_exported():
  import ctypes
  from ldm_tf2_amd import _lib, ops
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldm_hip.h")).read(), flags=re.S)
  ctype = {"int": _lib.c_i32, "void*": _lib.c_vp, "const float*": _lib.c_vp, "float*": _lib.c_vp,
           "const int32_t*": _lib.c_vp}
  m = re.search(r"\bint\s+ldm_resample_nhwc\s*\(([^)]*)\)\s*;", src)
  assert m
  ps = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
  assert [p.rsplit(" ", 1)[1] for p in ps] == ["x", "tmp", "out", "B", "H", "W", "c", "Ho", "Wo", "xstart", "xw", "xtaps",
                                               "ystart", "yw", "ytaps", "stream"]
  res, args = _lib.SIGNATURES["ldm_resample_nhwc"]
  assert res is _lib.c_i32 and args == [ctype[p.rsplit(" ", 1)[0]] for p in ps]
  assert isinstance(_lib.lib.ldm_resample_nhwc, ctypes._CFuncPtr)
  assert "resample_nhwc" in ops.__all__
  assert _lib.RESIZE_MODES == {"nearest": 0, "bilinear": 1, "bicubic": 2}
