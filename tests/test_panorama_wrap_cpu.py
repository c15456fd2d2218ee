"""Seamless panoramas, host side: the wrapped grid against brute force, the two-range claim the
fold kernel's loop rests on, the NumPy restatement (tests/panorama_wrap_ref.py) against tests/panorama_ref.py where no
axis wraps, the profile tables, the YAML keys, the loop's rejections and the new entries' declaration and binding.
Nothing runs on a GPU."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

import panorama_ref as P
import panorama_wrap_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")


def _grids(limit):
  for L in range(1, limit):
    for l in range(1, L + 1):
      for s in range(1, l + 1):
        yield L, l, s


def test_wrap_origins_against_brute_force():
  from ldm_tf2_amd.model_runners import wrap_origins
  for L, l, s in _grids(13):
    o = wrap_origins(L, l, s)
    assert o == Q.origins(L, l, s, True) == [i * s for i in range(-(-L // s))], (L, l, s, o)
    assert len(o) == -(-L // s) and len(set(o)) == len(o) and all(0 <= a < L for a in o), (L, l, s, o)
    covered = np.zeros(L, dtype=int)
    for a in o:
      cells = [(a + j) % L for j in range(l)]
      assert len(set(cells)) == l, (L, l, s, a)                       # a window covers a cell at most once
      covered[cells] += 1
    assert covered.min() >= 1, (L, l, s, o)
    if l == L and s == L:
      assert o == [0] == P.origins(L, l, s)                           # one window: the unwrapped grid


@pytest.mark.parametrize("args", [(8, 9, 4), (8, 4, 0), (8, 4, 5), (8, 0, 1), (8, 4, -1), (0, 0, 0)])
def test_wrap_origins_rejects(args):
  from ldm_tf2_amd.model_runners import wrap_origins
  with pytest.raises(ValueError):
    wrap_origins(*args)
  with pytest.raises(ValueError):
    Q.origins(*args, True)


def test_covering_windows_are_two_ascending_ranges():
  """For every wrapped grid with L < 20 and every cell p: the windows covering p (brute force over the cells each
  window lies on) are the i with i s <= p < i s + l followed by the i with i s <= p + L < i s + l, both cut to
  i < n; the two are disjoint runs of consecutive indices and the first lies wholly below the second, so ascending
  window index is the first range followed by the second -- with the window element p - i s and p + L - i s."""
  for L, l, s in _grids(20):
    n = -(-L // s)
    for p in range(L):
      brute = {i: [j for j in range(l) if (i * s + j) % L == p] for i in range(n)}
      assert all(len(js) <= 1 for js in brute.values())
      cover = [i for i in range(n) if brute[i]]
      first, second = Q.covering_ranges(L, l, s, p)
      assert first + second == cover, (L, l, s, p, first, second, cover)
      assert first and first == list(range(first[0], first[-1] + 1))
      assert second == list(range(second[0], second[-1] + 1)) if second else True
      assert not second or (first[-1] < second[0] and second[-1] == n - 1)
      # the closed forms of the kernel
      lo0 = 0 if p < l else (p - l) // s + 1
      assert first == list(range(lo0, p // s + 1)), (L, l, s, p)
      assert second == list(range((p + L - l) // s + 1, n)), (L, l, s, p)
      assert all(brute[i] == [p - i * s] for i in first) and all(brute[i] == [p + L - i * s] for i in second)


@pytest.mark.parametrize("shape,window,stride", [((2, 5, 7, 4), (3, 4), (2, 3)), ((1, 16, 28, 4), (16, 16), (8, 8)),
                                                 ((2, 6, 8, 4), (3, 4), (3, 4)), ((1, 5, 6, 3), (3, 3), (1, 2))])
def test_restatement_without_wrap_is_the_section_12_restatement(shape, window, stride):
  B, H, W, c = shape
  off = (False, False)
  g = np.random.default_rng(0)
  x = g.standard_normal(shape).astype(np.float32)
  x[0, 0, 0, 0] = -0.0
  assert Q.windows(H, W, window, stride, off) == P.windows(H, W, window, stride)
  assert np.array_equal(Q.counts(H, W, window, stride, off), P.counts(H, W, window, stride))
  win = Q.gather(x, window, stride, off)
  assert np.array_equal(win.view(np.uint32), P.gather(x, window, stride).view(np.uint32))
  e = (g.standard_normal(win.shape) * 10. ** g.integers(-3, 4, size=win.shape[:3] + (1, 1, 1))).astype(np.float32)
  e[0, 0, 0, 0, 0, 0] = -0.0
  want = P.fold(e, H, W, window, stride)
  got = Q.fold(e, H, W, window, stride, off)
  assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
  ones = Q.fold(e, H, W, window, stride, off, np.ones(window[0], np.float32), np.ones(window[1], np.float32))
  assert np.array_equal(ones.view(np.uint32), want.view(np.uint32))    # a table of ones is the plain mean's bits
  assert np.array_equal(Q.fold64(e, H, W, window, stride, off), P.fold64(e, H, W, window, stride))
  assert np.array_equal(Q.fold_abs(e, H, W, window, stride, off), P.fold_abs(e, H, W, window, stride))


def test_restatement_wrapped_gather_and_fold():
  """A 1x6 canvas, window 4, stride 4, wrapped: windows at 0 and 4, the second on cells 4, 5, 0, 1."""
  x = np.arange(6, dtype=np.float32).reshape(1, 1, 6, 1)
  wrap = (False, True)
  assert Q.windows(1, 6, (1, 4), (1, 4), wrap) == [(0, 0), (0, 4)]
  win = Q.gather(x, (1, 4), (1, 4), wrap)
  assert win.shape == (2, 1, 2, 1, 4, 1) and win[0, 0, :, 0, :, 0].tolist() == [[0, 1, 2, 3], [4, 5, 0, 1]]
  assert Q.counts(1, 6, (1, 4), (1, 4), wrap).tolist() == [[2, 2, 1, 1, 1, 1]]
  back = Q.fold(win, 1, 6, (1, 4), (1, 4), wrap)
  assert np.array_equal(back, np.stack([x, x]))
  # tent weights 1 2 2 1: cell 0 = (1 * a + 2 * b) / 3 with a from window 0 (element 0), b from window 1 (element 2)
  e = np.zeros((1, 1, 2, 1, 4, 1), dtype=np.float32)
  e[0, 0, 0, 0, 0, 0], e[0, 0, 1, 0, 2, 0] = 3., 6.
  out = Q.fold(e, 1, 6, (1, 4), (1, 4), wrap, np.ones(1, np.float32), Q.tent(4))
  assert out[0, 0, 0, 0, 0] == np.float32(5.) and np.count_nonzero(out) == 1
  assert Q.fold_den(1, 6, (1, 4), (1, 4), wrap, np.ones(1, np.float32), Q.tent(4)).tolist() == [[3, 3, 2, 1, 1, 2]]
  assert np.array_equal(Q.wrap_pad(x, (0, 2))[0, 0, :, 0], [4, 5, 0, 1, 2, 3, 4, 5, 0, 1])


@pytest.mark.parametrize("l", [1, 2, 3, 4, 7, 16, 32])
def test_profile_tables(l):
  from ldm_tf2_amd.model_runners import WINDOW_WEIGHTS, window_profile, window_weight_tables
  assert WINDOW_WEIGHTS == ("uniform", "tent", "gaussian")
  for kind, want in (("tent", Q.tent(l)), ("gaussian", Q.gaussian(l)), ("uniform", np.ones(l, np.float32))):
    p = window_profile(kind, l)
    assert p.dtype == np.float32 and p.shape == (l,) and np.array_equal(p, want), (kind, l)
    assert (p > 0).all() and np.isfinite(p).all() and np.array_equal(p, p[::-1]), (kind, l)
  t = window_profile("tent", l)
  assert np.array_equal(t, np.round(t)) and t[0] == 1 and t.max() == (l + 1) // 2
  g = window_profile("gaussian", l)
  assert g.max() <= 1 and g.argmax() in ((l - 1) // 2, l // 2)
  assert window_weight_tables("uniform", (l, l)) == ("uniform", None)
  kind, (wy, wx) = window_weight_tables("tent", (l, l + 1))
  assert kind == "tent" and np.array_equal(wy, Q.tent(l)) and np.array_equal(wx, Q.tent(l + 1))
  kind, (wy, wx) = window_weight_tables(([2.] * l, np.arange(1, l + 2)), (l, l + 1))
  assert kind == "tables" and wy.dtype == wx.dtype == np.float32 and wx.tolist() == list(range(1, l + 2))


@pytest.mark.parametrize("bad", ["box", ([1., 1.], [1., 1., 1.]), ([1., 0., 1.], [1., 1.]), ([1., -1., 1.], [1., 1.]),
                                 ([1., np.nan, 1.], [1., 1.]), ([1., 1e39, 1.], [1., 1.]), ([1., 1., 1.],),
                                 ([[1., 1., 1.]], [1., 1.]), 3])
def test_profile_rejections(bad):
  from ldm_tf2_amd.model_runners import window_weight_tables
  with pytest.raises(ValueError):
    window_weight_tables(bad, (3, 2))


def _cfg(**keys):
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  return yaml.safe_load(yaml.safe_dump(dict(cfg, ldm_sampling=dict(cfg["ldm_sampling"], **keys))))


PANO = dict(sample_save_progress=False, latent_shape=[4, 32, 128, 4], window=[32, 32])


def test_yaml_keys_bind():
  from ldm_tf2_amd import run_ldm_sampler as R
  ids = np.zeros((8, 77), dtype=np.int64)
  assert R.sampling_call(_cfg(**PANO), ids, 5)[2] == dict(window=(32, 32), stride=(16, 16), seed=5)     # as before
  cfg = _cfg(**PANO, window_wrap=[False, True], window_weights="tent", wrap_decode_margin=2)
  method, args, kwargs = R.sampling_call(cfg, ids, 5)
  assert method == "ddim_p_sample_loop_panorama" and args[1] == [4, 32, 128, 4]
  assert kwargs == dict(window=(32, 32), stride=(16, 16), seed=5, wrap=(False, True), window_weights="tent",
                        wrap_decode_margin=2)
  assert R.sampling_call(_cfg(**PANO, window_weights="gaussian"), ids, 5)[2]["window_weights"] == "gaussian"
  assert R.sampling_call(_cfg(**PANO, wrap_decode_margin=0), ids, 5)[2]["wrap_decode_margin"] == 0
  import inspect
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  params = inspect.signature(LatentDiffusionModelSampler.ddim_p_sample_loop_panorama).parameters
  assert set(kwargs) <= set(params)
  assert params["wrap"].default == (False, False) and params["window_weights"].default == "uniform"
  assert params["wrap_decode_margin"].default == 0
  assert list(params)[1:6] == ["cond_model_inputs", "shape", "window", "stride", "guidance_scale"]


@pytest.mark.parametrize("extra,match", [
    (dict(window_wrap=[True]), "window_wrap"), (dict(window_wrap=[0, 1]), "window_wrap"),
    (dict(window_wrap=True), "window_wrap"), (dict(window_weights="box"), "window_weights"),
    (dict(window_weights=[1., 2.]), "window_weights"), (dict(wrap_decode_margin=-1), "wrap_decode_margin"),
    (dict(wrap_decode_margin=1.5), "wrap_decode_margin"), (dict(wrap_decode_margin=True), "wrap_decode_margin"),
    (dict(window_wrap=[False, True], init_image="x.npy"), "init_image"),
    (dict(window_weights="tent", guidance_interval=[200, 600]), "guidance_interval")])
def test_yaml_rejected_values(extra, match):
  from ldm_tf2_amd import run_ldm_sampler as R
  with pytest.raises(ValueError, match=match):
    R.sampling_call(_cfg(**dict(PANO, **extra)), np.zeros((8, 77), dtype=np.int64), 5)


@pytest.mark.parametrize("extra", [dict(window_wrap=[False, True]), dict(window_weights="tent"),
                                   dict(wrap_decode_margin=2), dict(window_weights="uniform"),
                                   dict(wrap_decode_margin=0)])
def test_yaml_keys_need_a_window(extra):
  from ldm_tf2_amd import run_ldm_sampler as R
  (key,) = extra
  with pytest.raises(ValueError, match=f"{key} needs ldm_sampling.window"):
    R.sampling_call(_cfg(sample_save_progress=False, **extra), np.zeros((8, 77), dtype=np.int64), 5)


class _FakeModel:
  device = torch.device("cpu")


def test_loop_rejections_need_no_gpu():
  """Raised before anything touches a model or the device."""
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  s = LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), num_steps=1000, beta_start=0.00085,
                                  beta_end=0.012, num_ddim_steps=10)
  ids = np.zeros((4, 77), dtype=np.int64)
  run = lambda **kw: s.ddim_p_sample_loop_panorama(ids, [2, 16, 24, 4], (16, 16), **kw)
  for bad in (True, (True,), (0, 1), "xy", (True, False, True)):
    with pytest.raises(ValueError, match="wrap"):
      run(wrap=bad)
  with pytest.raises(ValueError, match="window_weights"):
    run(window_weights="box")
  with pytest.raises(ValueError, match="wy has shape"):
    run(window_weights=(np.ones(8), np.ones(16)))
  with pytest.raises(ValueError, match="positive"):
    run(window_weights=(np.ones(16), np.zeros(16)))
  with pytest.raises(ValueError, match="wrap_decode_margin"):
    run(wrap=(False, True), wrap_decode_margin=-1)
  with pytest.raises(ValueError, match="wrap_decode_margin"):
    run(wrap=(False, True), wrap_decode_margin=1.5)
  with pytest.raises(ValueError, match="wrap_decode_margin"):
    run(wrap=(False, True), wrap_decode_margin=25)
  with pytest.raises(ValueError, match="guidance"):
    run(wrap=(False, True), guidance_scale=[5.] * 10)
  with pytest.raises(ValueError, match="stride"):                   # a wrapped axis takes the same strides
    run(wrap=(False, True), stride=(8, 17))
  with pytest.raises(ValueError, match="window extent"):
    s.ddim_p_sample_loop_panorama(ids, [2, 16, 24, 4], (16, 32), wrap=(False, True))
  assert not hasattr(s, "_win_key") and not hasattr(s, "_win_wy")      # nothing was allocated


def test_the_new_entries_are_declared_bound_and_exported():
  import ctypes
  from ldm_tf2_amd import _lib, ops
  src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldm_hip.h")).read(), flags=re.S)
  ctype = {"int": _lib.c_i32, "void*": _lib.c_vp, "const float*": _lib.c_vp, "float*": _lib.c_vp}
  want = {"ldm_window_gather_ex": 14, "ldm_window_fold_ex": 16, "ldm_wrap_pad_nhwc": 9}
  for name, n_args in want.items():
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    ps = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    types = [ctype[p.rsplit(" ", 1)[0]] for p in ps]
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_i32 and args == types and len(args) == n_args, (name, ps)
    assert isinstance(getattr(_lib.lib, name), ctypes._CFuncPtr)
  # the existing pair's arguments are a prefix of the _ex pair's
  for name in ("ldm_window_gather", "ldm_window_fold"):
    assert _lib.SIGNATURES[name + "_ex"][1][:11] == _lib.SIGNATURES[name][1][:11]
  for name in ("window_gather_ex", "window_fold_ex", "wrap_pad", "window_gather", "window_fold"):
    assert name in ops.__all__ and callable(getattr(ops, name))
  assert _lib.lib.ldm_version() == 100
