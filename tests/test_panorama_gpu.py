"""Panorama sampling on the GPU, all through the C ABI: ldm_window_gather and ldm_window_fold
against the NumPy restatement (tests/panorama_ref.py) bit for bit, fold's rounding against float64, every window
element accounted for, the launcher's rejections; then ddim_p_sample_loop_panorama: a window equal to the canvas is
ddim_p_sample_loop bit for bit, canvases of several windows against the oracle composition, graph replay, the calls
of a step, and the loop's rejections.

Gates.  Kernels: bit equality with the restatement; against float64 per element
|err| <= m * 2^-24 * sum_k |v_k| / count, m the number of covering windows (m - 1 additions and one division, each
within 2^-24 relative of a partial result that sum_k |v_k| bounds).  Loops: the rule of tests/test_deis_gpu.py, for
latents and for decoded images alike (the images inherit the latents' error): the uniform-table DDIM txt2img loop's
error against O.ddim_p_sample_loop measured in the same run, times 20/3, and the project's loop gates (1.3e-5 f32 /
8e-2 bf16); the decoded images, compared with the oracle's decoder run on the oracle's canvas, also meet the gate of
a single decoder pass (T.REL: 5e-5 f32 / 4e-2 bf16).  Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.

A pointer aligned to its element only (c = 4) is not rejected: the launcher takes the element-wise path, whose
results are the same bits (test_launcher_takes_a_misaligned_pointer_element_wise).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deis_ref as D  # noqa: E402
import panorama_ref as P  # noqa: E402
import plms_ref  # noqa: E402
import test_deis_gpu as G  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import _lib, ops  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, N, LDM, GS = T.B, T.N, T.LDM, 5.
# (H, W, h, w, sy, sx, c): odd sizes with both axes clamped; one window row with a clamped last column; nW = 1;
# stride == window (no overlap); the element-wise path (c = 3) at stride 1 with counts up to 9
SHAPES = [(5, 7, 3, 4, 2, 3, 4), (16, 28, 16, 16, 8, 8, 4), (8, 8, 8, 8, 4, 4, 4), (6, 8, 3, 4, 3, 4, 4),
          (5, 6, 3, 3, 1, 2, 3)]
SHAPE_IDS = ["odd-clamped", "row-clamped", "one-window", "no-overlap", "scalar-stride1"]
GUARD = 64                                       # elements of NaN on either side (keeps 16-byte alignment)


def _geom(shape):
  H, W, h, w, sy, sx, c = shape
  return H, W, (h, w), (sy, sx), c, len(P.windows(H, W, (h, w), (sy, sx)))


def _guarded(dev, shape, dtype=torch.float32):
  """(whole NaN buffer, the view of `shape` inside it)."""
  n = int(np.prod(shape))
  buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
  return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
  return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def _bits(a):
  return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- 1. ldm_window_gather --------------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gather(dev, shape, nb, x_dtype):
  H, W, window, stride, c, n_win = _geom(shape)
  x = np.random.default_rng(3).standard_normal((nb, H, W, c)).astype(np.float32)
  x[0, 0, 0, 0] = -0.0
  want = torch.from_numpy(P.gather(x, window, stride))
  assert want.shape[2] == n_win == len(P.origins(H, window[0], stride[0])) * len(P.origins(W, window[1], stride[1]))
  buf, x_win = _guarded(dev, (2, nb, n_win, window[0], window[1], c), x_dtype)
  assert ops.window_gather(torch.from_numpy(x).to(dev), x_win, window, stride) is x_win
  got = x_win.cpu()
  assert _guards_intact(buf)
  assert torch.equal(got[0], got[1])
  if x_dtype == torch.float32:
    assert np.array_equal(_bits(got.numpy()), _bits(want.numpy()))
  else:
    assert torch.equal(got.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))


# ---- 2. ldm_window_fold ----------------------------------------------------------------------------------
@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fold(dev, shape, nb, halves):
  H, W, window, stride, c, n_win = _geom(shape)
  g = np.random.default_rng(4)
  e = (g.standard_normal((halves, nb, n_win, window[0], window[1], c)) *
       10. ** g.integers(-3, 4, size=(halves, nb, n_win, 1, 1, 1))).astype(np.float32)
  e[0, 0, 0, 0, 0, 0] = -0.0
  buf, out = _guarded(dev, (2, nb, H, W, c))                         # always a two-half buffer
  assert ops.window_fold(torch.from_numpy(e).to(dev), out[:halves], window, stride).data_ptr() == out.data_ptr()
  got = out.cpu().numpy()
  assert _guards_intact(buf)
  if halves == 1:
    assert np.isnan(got[1]).all()                                    # the other half is not this launch's
  got = got[:halves]
  want = P.fold(e, H, W, window, stride)
  assert np.array_equal(_bits(got), _bits(want))
  # against float64: m - 1 additions and one division
  m = P.counts(H, W, window, stride)[None, None, :, :, None]
  err = np.abs(got.astype(np.float64) - P.fold64(e, H, W, window, stride))
  bound = m * 2.0 ** -24 * P.fold_abs(e, H, W, window, stride)
  print(f"fold {shape} B={nb} halves={halves}: counts {sorted(set(m.ravel().tolist()))}, worst err / bound = "
        f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}")
  assert (err <= bound).all()
  if m.max() == 1:                                                   # nothing is summed: the input's bits, moved
    assert np.array_equal(np.sort(_bits(got).ravel()), np.sort(_bits(e).ravel()))
    if n_win == 1:
      assert np.array_equal(_bits(got).ravel(), _bits(e).ravel())


@pytest.mark.parametrize("shape", [(16, 24, 8, 8, 4, 4, 4), (12, 8, 4, 6, 2, 3, 3)], ids=["wide", "scalar"])
def test_fold_of_gather_is_the_identity(dev, shape):
  """Stride = window / 2, nothing clamped: every count is 1, 2 or 4 and all addends of a cell are equal."""
  H, W, window, stride, c, n_win = _geom(shape)
  assert set(np.unique(P.counts(H, W, window, stride))) == {1, 2, 4}
  x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, H, W, c)).astype(np.float32)).to(dev)
  x_win = torch.empty(2, B, n_win, window[0], window[1], c, device=dev)
  out = torch.empty(2, B, H, W, c, device=dev)
  ops.window_fold(ops.window_gather(x, x_win, window, stride), out, window, stride)
  assert torch.equal(out[0].view(torch.int32), x.view(torch.int32))
  assert torch.equal(out[1].view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fold_accounts_for_every_window_element(dev, shape):
  """A one-hot batch per window: canvas e of the batch has its single 1.0 at element e of window k.  Every such canvas
  comes back with exactly one nonzero, 1 / count, at the cell that element covers."""
  H, W, window, stride, c, n_win = _geom(shape)
  h, w = window
  n = h * w * c
  cnt = P.counts(H, W, window, stride)
  ys, xs, chs = np.unravel_index(np.arange(n), (h, w, c))
  out = torch.empty(1, n, H, W, c, device=dev)
  for k, (oy, ox) in enumerate(P.windows(H, W, window, stride)):
    e = torch.zeros(1, n, n_win, n, device=dev)
    e[0, torch.arange(n, device=dev), k, torch.arange(n, device=dev)] = 1.
    ops.window_fold(e.view(1, n, n_win, h, w, c), out, window, stride)
    got = out[0].cpu().numpy()
    assert (np.count_nonzero(got.reshape(n, -1), axis=1) == 1).all(), (shape, k)
    want = (np.float32(1.) / cnt[oy + ys, ox + xs].astype(np.float32)).astype(np.float32)
    assert np.array_equal(got[np.arange(n), oy + ys, ox + xs, chs], want), (shape, k)


# ---- 3. the launcher -------------------------------------------------------------------------------------
def test_launcher_rejections(dev):
  x = torch.zeros(1, 8, 8, 4, device=dev)
  win = torch.zeros(2, 1, 9, 4, 4, 4, device=dev)
  can = torch.zeros(2, 1, 8, 8, 4, device=dev)
  s = torch.cuda.current_stream().cuda_stream
  gather = lambda cp, wp, dt, *a: _lib.lib.ldm_window_gather(cp, wp, dt, *a, s)
  fold = lambda wp, cp, hv, *a: _lib.lib.ldm_window_fold(wp, cp, hv, *a, s)
  ok = (1, 8, 8, 4, 4, 4, 2, 2)                                      # B, H, W, c, h, w, sy, sx
  cases = [("within the canvas", (1, 8, 8, 4, 9, 4, 2, 2)), ("within the canvas", (1, 8, 8, 4, 4, 9, 2, 2)),  # h > H, w > W
           ("stride", (1, 8, 8, 4, 4, 4, 2, 5)), ("stride", (1, 8, 8, 4, 4, 4, 0, 2)),       # sx > w, sy = 0
           ("stride", (1, 8, 8, 4, 4, 4, 5, 2)), ("bad args", (0, 8, 8, 4, 4, 4, 2, 2)),
           ("bad args", (1, 8, 8, 0, 4, 4, 2, 2))]
  for word, a in cases:
    for name, call in (("ldm_window_gather", lambda: gather(x.data_ptr(), win.data_ptr(), _lib.F32, *a)),
                       ("ldm_window_fold", lambda: fold(win.data_ptr(), can.data_ptr(), 2, *a))):
      assert call() == _lib.ERR_ARG, (name, a)
      assert name in _lib.last_error() and word in _lib.last_error(), (_lib.last_error(), a)
  for call, word in ((lambda: gather(None, win.data_ptr(), _lib.F32, *ok), "null pointer"),
                     (lambda: gather(x.data_ptr(), None, _lib.F32, *ok), "null pointer"),
                     (lambda: fold(None, can.data_ptr(), 2, *ok), "null pointer"),
                     (lambda: fold(win.data_ptr(), None, 2, *ok), "null pointer"),
                     (lambda: gather(x.data_ptr(), win.data_ptr(), 7, *ok), "x_dtype"),
                     (lambda: fold(win.data_ptr(), can.data_ptr(), 0, *ok), "halves"),
                     (lambda: fold(win.data_ptr(), can.data_ptr(), 3, *ok), "halves")):
    assert call() == _lib.ERR_ARG
    assert word in _lib.last_error(), _lib.last_error()
  assert gather(x.data_ptr(), win.data_ptr(), _lib.F32, *ok) == _lib.OK
  # the wrappers pass the launcher's message on
  with pytest.raises(_lib.LdmHipError, match="within the canvas"):
    ops.window_gather(x, win, (9, 4), (2, 2))
  with pytest.raises(_lib.LdmHipError, match="stride"):
    ops.window_fold(win, can, (4, 4), (0, 2))
  with pytest.raises(TypeError):
    ops.window_fold(win.to(torch.bfloat16), can, (4, 4), (2, 2))
  torch.cuda.synchronize()


@pytest.mark.parametrize("x_dtype", T.DT, ids=["f32", "bf16"])
def test_launcher_takes_a_misaligned_pointer_element_wise(dev, x_dtype):
  """c = 4 with pointers aligned to their element only: not rejected, same bits as the aligned launch."""
  H, W, window, stride, c, n_win = _geom(SHAPES[0])
  x = np.random.default_rng(6).standard_normal((B, H, W, c)).astype(np.float32)
  n_can, n_w = B * H * W * c, 2 * B * n_win * window[0] * window[1] * c
  off = lambda n, dt=torch.float32: torch.full((n + GUARD + 1,), float("nan"), dtype=dt, device=dev)
  xb = off(n_can)
  xd = xb[1:1 + n_can].view(B, H, W, c)
  xd.copy_(torch.from_numpy(x))
  wb = off(n_w, x_dtype)
  x_win = wb[1:1 + n_w].view(2, B, n_win, window[0], window[1], c)
  assert xd.data_ptr() % 16 and x_win.data_ptr() % (8 if x_dtype == torch.bfloat16 else 16)
  ops.window_gather(xd, x_win, window, stride)
  want = torch.from_numpy(P.gather(x, window, stride)).to(x_dtype)
  assert torch.equal(x_win.cpu(), want) and bool(torch.isnan(wb[:1]).all() and torch.isnan(wb[1 + n_w:]).all())
  e = np.random.default_rng(7).standard_normal((2, B, n_win, window[0], window[1], c)).astype(np.float32)
  eb, ob = off(n_w), off(2 * n_can)
  ed = eb[1:1 + n_w].view(2, B, n_win, window[0], window[1], c)
  ed.copy_(torch.from_numpy(e))
  out = ob[1:1 + 2 * n_can].view(2, B, H, W, c)
  ops.window_fold(ed, out, window, stride)
  assert np.array_equal(_bits(out.cpu().numpy()), _bits(P.fold(e, H, W, window, stride)))
  assert bool(torch.isnan(ob[:1]).all() and torch.isnan(ob[1 + 2 * n_can:]).all())


# ---- 4. a window equal to the canvas is txt2img, bit for bit ------------------------------------------------
def _x_T(H, W):
  return np.random.default_rng(9).standard_normal((B, H, W, 4)).astype(np.float32)


def _noises(H, W):
  return np.random.default_rng(33).standard_normal((N, B, H, W, 4)).astype(np.float32)


# (sampler, eta, noise source, whether the caller gives x_T and the eta-noise table)
ONE_WINDOW = {"ddim": ("ddim", 0., "host", True), "ddim-eta1": ("ddim", 1., "host", True),
              "plms": ("plms", 0., "host", True), "deis": ("deis", 0., "host", True),
              "ddim-device": ("ddim", 1., "device", False)}


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("form", list(ONE_WINDOW))
def test_one_window_equals_txt2img_bit_for_bit(dev, form, dtype, unet_w, txt_w, kl_w):
  name, eta, source, given = ONE_WINDOW[form]
  s = G._sampler(dev, dtype, unet_w, txt_w, kl_w, sampler=name, spacing="uniform", eta=eta, noise_source=source)
  kw = dict(x_T=_x_T(T.HW, T.HW), noises=_noises(T.HW, T.HW) if eta else None) if given else {}
  kw.update(seed=G.SEED, first_sample_index=3)
  shape = [B, T.HW, T.HW, 4]
  want = s.ddim_p_sample_loop(T._ids(), shape, GS, **kw).clone()
  want_lat = s._xt.clone()
  got = s.ddim_p_sample_loop_panorama(T._ids(), shape, (T.HW, T.HW), guidance_scale=GS, **kw)
  assert s._win_key == (B, 1, T.HW, T.HW, 4)
  assert bool(torch.isfinite(got).all())
  assert torch.equal(s._xt, want_lat) and torch.equal(got, want)
  # and back: the txt2img loop after the panorama one
  assert torch.equal(s.ddim_p_sample_loop(T._ids(), shape, GS, **kw), want)


# ---- 5. several windows against the oracle composition ------------------------------------------------------
# (sampler, step table, eta)
FORMS = {"ddim": ("ddim", "uniform", 1.), "plms": ("plms", "logsnr", 0.), "deis": ("deis", "karras", 0.)}
CANVASES = {"16x28": (16, 28), "24x24": (24, 24)}                    # window 16, stride 8: 3 (clamped) and 4 windows
WINDOW, STRIDE = (16, 16), (8, 8)
_CACHE = {}


def _oracle(form, canvas, w):
  key = (form, canvas)
  if key not in _CACHE:
    name, spacing, eta = FORMS[form]
    H, W = CANVASES[canvas]
    sched = G._schedule(spacing, eta)
    context = O.text_encoder(T._ids(), w["cond_stage_model"], torch.float32)
    wtab = D.weight_table(G.AB, sched["ddim_steps"]).astype(np.float32) if name == "deis" else None
    lat = P.loop(O, context, w["unet"], _x_T(H, W), WINDOW, STRIDE, sched, GS, sampler=name,
                 noises=_noises(H, W) if eta else None, weights=wtab, ms_update=D.ms_update,
                 plms_weights=plms_ref.WEIGHTS)
    _CACHE[key] = (lat, O.decoder_forward(lat / LDM["scale_factor"], w["autoencoder"]))
  return _CACHE[key]


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("canvas", list(CANVASES))
@pytest.mark.parametrize("form", list(FORMS))
def test_loops_against_oracle(dev, form, canvas, dtype, unet_w, txt_w, kl_w):
  name, spacing, eta = FORMS[form]
  H, W = CANVASES[canvas]
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = G._ddim_loop_error(dev, dtype, w)
  s = G._sampler(dev, dtype, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, eta=eta)
  got = s.ddim_p_sample_loop_panorama(T._ids(), [B, H, W, 4], WINDOW, STRIDE, GS, x_T=_x_T(H, W),
                                      noises=_noises(H, W) if eta else None)
  n_win = {"16x28": 3, "24x24": 4}[canvas]
  assert s._win_key == (B, n_win, 16, 16, 4) and tuple(s._x_win.shape) == (2 * B * n_win, 16, 16, 4)
  assert tuple(got.shape) == (B, 8 * H, 8 * W, 3) and bool(torch.isfinite(got).all())
  lat, images = _oracle(form, canvas, w)
  G._loop_check(f"{form}/{spacing} panorama {canvas} latents", s._xt, lat, dtype, base)
  G._loop_check(f"{form}/{spacing} panorama {canvas} images", got, images, dtype, base)
  T.check(got, images, dtype, f"{form}/{spacing} panorama {canvas} images")      # and the gate of a decoder pass


def test_the_windows_matter(dev, unet_w, txt_w, kl_w):
  """The same canvas denoised as one oversized U-Net input lands elsewhere: the loop gate can tell the two apart."""
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler="ddim", spacing="uniform", eta=0.)
  x_T = _x_T(24, 24)
  pano = s.ddim_p_sample_loop_panorama(T._ids(), [B, 24, 24, 4], WINDOW, STRIDE, GS, x_T=x_T).clone()
  whole = s.ddim_p_sample_loop(T._ids(), [B, 24, 24, 4], GS, x_T=x_T)
  assert T.rel_err(whole, pano.cpu())[0] > 10 * T.LOOP_REL[torch.float32]


# ---- 6. graph and calls -----------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_graphs_are_keyed(dev, unet_w, txt_w, kl_w):
  ids, x_T = T._ids(), _x_T(16, 28)
  shape = [B, 16, 28, 4]
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=True)
  e = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  got = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T).clone()
  g = s._graph
  assert g is not None and s._graph_key[0] == "panorama" and (16, 16) in s._graph_key and (8, 8) in s._graph_key
  assert s.last_loop_ms_per_step() > 0.
  assert torch.equal(got, e.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T)) and e._graph is None
  assert torch.equal(s._xt, e._xt) and torch.equal(s._ring, e._ring)
  rec = []
  assert torch.equal(got, s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T, record=rec))
  assert len(rec) == N and torch.equal(rec[-1], s._xt) and s._graph is g
  # the same key replays the same graph; another stride is another graph and another result
  assert torch.equal(got, s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T)) and s._graph is g
  other = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, (8, 4), GS, x_T=x_T).clone()
  assert s._graph is not g and not torch.equal(other, got)
  assert torch.equal(other, e.ddim_p_sample_loop_panorama(ids, shape, WINDOW, (8, 4), GS, x_T=x_T))
  # the default stride is half the window
  g = s._graph
  assert torch.equal(got, s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, guidance_scale=GS, x_T=x_T))
  assert s._graph is not g and (8, 8) in s._graph_key
  # device noise: one graph for every seed
  d = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler="ddim", spacing="uniform", eta=1.,
                 noise_source="device")
  de = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler="ddim", spacing="uniform", eta=1.,
                  noise_source="device", use_graph=False)
  a = d.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, seed=1).clone()
  gd = d._graph
  b_ = d.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, seed=2).clone()
  assert d._graph is gd and not torch.equal(a, b_) and not hasattr(d, "_noise_buf")
  assert torch.equal(a, de.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, seed=1))
  assert torch.equal(b_, de.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, seed=2))


UPDATES = {("ddim", False): "ldm_cfg_ddim_update", ("ddim", True): "ldm_cfg_ddim_update_rng",
           ("plms", False): "ldm_cfg_plms_update", ("deis", False): "ldm_cfg_ms_update"}


@pytest.mark.parametrize("temb_table", [True, False])
@pytest.mark.parametrize("name,rng", list(UPDATES))
def test_a_step_adds_one_gather_and_one_fold(dev, unet_w, txt_w, kl_w, monkeypatch, name, rng, temb_table):
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing="uniform", use_graph=False,
                 temb_table=temb_table, noise_source="device" if rng else "host")
  ids, shape = T._ids(), [B, 16, 28, 4]
  s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, seed=1)

  def count(step):
    s._index_dev.fill_(s._loop_start_index(4))
    s._set_loop_start(3)
    proxy = T._CountingLib(ops.lib)
    monkeypatch.setattr(ops, "lib", proxy)
    step()
    monkeypatch.setattr(ops, "lib", proxy._lib)
    torch.cuda.synchronize()
    return proxy.calls
  pano = count(lambda: s._step_panorama(GS, None, True, WINDOW, STRIDE, rng=rng))
  assert pano[0] == "ldm_window_gather" and pano.count("ldm_window_gather") == 1
  assert pano.count("ldm_window_fold") == 1 and pano.count(UPDATES[name, rng]) == 1
  assert sum(c.startswith("ldm_cfg_") for c in pano) == 1
  # gather, the U-Net's calls, fold, update: in that order, nothing after
  assert pano.index("ldm_window_fold") == len(pano) - 2 > 1 and pano[-1] == UPDATES[name, rng]
  # txt2img on the same sampler: none of the new calls, and the calls of a sampler that never ran a panorama
  s.ddim_p_sample_loop(ids, [B, 16, 16, 4], GS, seed=1)
  plain = count(lambda: s._step(GS, False, None, dec_index=True, rng=rng))
  assert not any("window" in c for c in plain) and plain.count(UPDATES[name, rng]) == 1
  fresh = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing="uniform", use_graph=False,
                     temb_table=temb_table, noise_source="device" if rng else "host")
  fresh.ddim_p_sample_loop(ids, [B, 16, 16, 4], GS, seed=1)
  s = fresh                                                          # (count() steps `s`)
  assert count(lambda: fresh._step(GS, False, None, dec_index=True, rng=rng)) == plain
  print({"panorama": len(pano), "txt2img": len(plain)})


# ---- 7. rejections ----------------------------------------------------------------------------------------
def test_rejections(dev, unet_w, txt_w, kl_w):
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  ids, shape = T._ids(), [B, 16, 28, 4]
  with pytest.raises(ValueError, match="guidance"):
    s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, [GS] * N)
  with pytest.raises(ValueError, match="guidance"):
    s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, guidance_interval=(200, 600))
  with pytest.raises(ValueError, match="window extent"):
    s.ddim_p_sample_loop_panorama(ids, shape, (32, 16), STRIDE, GS)
  with pytest.raises(ValueError, match="stride"):
    s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, (8, 17), GS)
  assert s._graph is None and not hasattr(s, "_win_key")               # nothing was allocated or captured
