"""Seamless panoramas on the GPU: ldm_window_gather_ex, ldm_window_fold_ex and
ldm_wrap_pad_nhwc against the NumPy restatement (tests/panorama_wrap_ref.py) bit for bit, the weighted fold's rounding
against float64, every window element accounted for, the launchers' rejections; then ddim_p_sample_loop_panorama with
`wrap`, `window_weights` and `wrap_decode_margin`: the defaults are the section 12 loop and its calls, a wrapped canvas
with tent weights against the restated loop, the seam property, graph replay, the calls of a step, the wrapped decode.

Gates.  Kernels: bit equality with the restatement; against float64 (from the same float32 tables) per element
|err| <= (2m + 1) * 2^-24 * sum_k |w_k v_k| / sum_k w_k, m the number of covering windows: one rounding per product
and m - 1 per sum give at most m u on the numerator, the denominator takes (m - 1) u and the division u -- 2m u to
first order, the extra u covers second order.  Loops: the rule of tests/test_panorama_gpu.py (the plain txt2img
loop's error measured in the same run x 20/3, capped by the project's loop gates), for latents and decoded images.
Tiny models, fixtures and inputs are those of tests/test_panorama_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deis_ref as D  # noqa: E402
import panorama_ref as P  # noqa: E402
import panorama_wrap_ref as Q  # noqa: E402
import plms_ref  # noqa: E402
import test_deis_gpu as G  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
import test_panorama_gpu as PG  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import _lib, ops  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, N, LDM, GS = T.B, T.N, T.LDM, 5.
# (H, W, h, w, sy, sx, wrap_y, wrap_x, c)
SHAPES = [(6, 10, 4, 4, 3, 3, False, True, 4),      # L % s != 0 on the wrapped axis; y clamped as in section 12
          (8, 8, 4, 4, 2, 2, True, True, 4),        # four covering windows per cell
          (5, 7, 3, 3, 1, 1, True, True, 3),        # the element-wise path; up to 9 covering windows
          (4, 6, 4, 6, 4, 2, False, True, 4),       # l == L with s < L: every window covers every column
          (4, 8, 4, 4, 4, 4, False, True, 4)]       # no overlap
SHAPE_IDS = ["x-odd", "both-4", "scalar-9", "full-window", "no-overlap"]
GUARD = PG.GUARD
_guarded, _guards_intact, _bits = PG._guarded, PG._guards_intact, PG._bits


def _geom(shape):
  H, W, h, w, sy, sx, wy, wx, c = shape
  return H, W, (h, w), (sy, sx), (wy, wx), c, len(Q.windows(H, W, (h, w), (sy, sx), (wy, wx)))


def _tables(kind, window):
  """(wy, wx) float32 host tables of `kind`, None for "uniform"."""
  h, w = window
  if kind == "uniform":
    return None
  if kind == "ones":
    return np.ones(h, np.float32), np.ones(w, np.float32)
  if kind == "tent":
    return Q.tent(h), Q.tent(w)
  g = np.random.default_rng(11)                                       # "random": positive, a decade apart
  return (np.exp(g.uniform(-1.2, 1.2, h)).astype(np.float32), np.exp(g.uniform(-1.2, 1.2, w)).astype(np.float32))


def _dev_tables(dev, tables):
  return None if tables is None else tuple(torch.from_numpy(t).to(dev) for t in tables)


def _eps(shape, seed=4):
  g = np.random.default_rng(seed)
  e = (g.standard_normal(shape) * 10. ** g.integers(-3, 4, size=tuple(shape[:3]) + (1, 1, 1))).astype(np.float32)
  e[0, 0, 0, 0, 0, 0] = -0.0
  return e


# ---- 1. ldm_window_gather_ex -----------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gather_ex(dev, shape, nb, x_dtype):
  H, W, window, stride, wrap, c, n_win = _geom(shape)
  x = np.random.default_rng(3).standard_normal((nb, H, W, c)).astype(np.float32)
  x[0, 0, 0, 0] = -0.0
  want = torch.from_numpy(np.ascontiguousarray(Q.gather(x, window, stride, wrap)))
  assert want.shape[2] == n_win
  buf, x_win = _guarded(dev, (2, nb, n_win, window[0], window[1], c), x_dtype)
  assert ops.window_gather_ex(torch.from_numpy(x).to(dev), x_win, window, stride, wrap) is x_win
  got = x_win.cpu()
  assert _guards_intact(buf)
  assert torch.equal(got[0], got[1])
  if x_dtype == torch.float32:
    assert np.array_equal(_bits(got.numpy()), _bits(want.numpy()))
  else:
    assert torch.equal(got.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("x_dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PG.SHAPES, ids=PG.SHAPE_IDS)
def test_gather_ex_without_wrap_is_gather(dev, shape, x_dtype):
  H, W, window, stride, c, n_win = PG._geom(shape)
  x = torch.from_numpy(np.random.default_rng(3).standard_normal((B, H, W, c)).astype(np.float32)).to(dev)
  a = torch.empty(2, B, n_win, window[0], window[1], c, dtype=x_dtype, device=dev)
  b = torch.full_like(a, float("nan"))
  ops.window_gather(x, a, window, stride)
  ops.window_gather_ex(x, b, window, stride, (False, False))
  bits = torch.int32 if x_dtype == torch.float32 else torch.int16
  assert torch.equal(a.view(bits), b.view(bits))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] % s[5] == 0],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[1] % s[5] == 0])
def test_gather_ex_shift_property(dev, shape):
  """W % sx == 0 on a wrapped x axis: rolling the canvas by one stride permutes the window columns cyclically."""
  H, W, window, stride, wrap, c, n_win = _geom(shape)
  assert wrap[1] and W % stride[1] == 0
  n_x = W // stride[1]
  x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, H, W, c)).astype(np.float32)).to(dev)
  a = torch.empty(2, B, n_win // n_x, n_x, window[0], window[1], c, device=dev)
  b = torch.empty_like(a)
  ops.window_gather_ex(x, a, window, stride, wrap)
  ops.window_gather_ex(torch.roll(x, stride[1], dims=2).contiguous(), b, window, stride, wrap)
  assert torch.equal(b.view(torch.int32), torch.roll(a, 1, dims=3).view(torch.int32))
  assert n_x == 1 or not torch.equal(a, b)


# ---- 2. ldm_window_fold_ex -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "tent", "random"])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fold_ex(dev, shape, nb, kind):
  H, W, window, stride, wrap, c, n_win = _geom(shape)
  tables = _tables(kind, window)
  tab = tables or (None, None)
  for halves in (2, 1):
    e = _eps((halves, nb, n_win, window[0], window[1], c))
    buf, out = _guarded(dev, (2, nb, H, W, c))                       # always a two-half buffer
    got = ops.window_fold_ex(torch.from_numpy(e).to(dev), out[:halves], window, stride, wrap, _dev_tables(dev, tables))
    assert got.data_ptr() == out.data_ptr()
    got = out.cpu().numpy()
    assert _guards_intact(buf)
    if halves == 1:
      assert np.isnan(got[1]).all()                                  # the other half is not this launch's
    got = got[:halves]
    assert np.array_equal(_bits(got), _bits(Q.fold(e, H, W, window, stride, wrap, *tab)))
    m = Q.counts(H, W, window, stride, wrap)[None, None, :, :, None]
    err = np.abs(got.astype(np.float64) - Q.fold64(e, H, W, window, stride, wrap, *tab))
    bound = (2 * m + 1) * 2.0 ** -24 * Q.fold_abs(e, H, W, window, stride, wrap, *tab)
    print(f"fold_ex {shape} {kind} B={nb} halves={halves}: counts {sorted(set(m.ravel().tolist()))}, worst err / "
          f"bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    if m.max() == 1 and kind != "random":                            # nothing is summed: the input's bits, moved
      assert np.array_equal(np.sort(_bits(got).ravel()), np.sort(_bits(e).ravel()))


@pytest.mark.parametrize("shape", PG.SHAPES, ids=PG.SHAPE_IDS)
def test_fold_ex_without_wrap_and_tables_is_fold(dev, shape):
  H, W, window, stride, c, n_win = PG._geom(shape)
  e = torch.from_numpy(_eps((2, B, n_win, window[0], window[1], c))).to(dev)
  a = torch.empty(2, B, H, W, c, device=dev)
  b = torch.full_like(a, float("nan"))
  ops.window_fold(e, a, window, stride)
  ops.window_fold_ex(e, b, window, stride, (False, False))
  assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fold_ex_ones_equal_no_tables(dev, shape):
  H, W, window, stride, wrap, c, n_win = _geom(shape)
  e = torch.from_numpy(_eps((2, B, n_win, window[0], window[1], c))).to(dev)
  a = torch.empty(2, B, H, W, c, device=dev)
  b = torch.full_like(a, float("nan"))
  ops.window_fold_ex(e, a, window, stride, wrap)
  ops.window_fold_ex(e, b, window, stride, wrap, _dev_tables(dev, _tables("ones", window)))
  assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_fold_ex_of_gather_ex_is_the_identity(dev):
  """8x8, window 4, stride 2, both axes wrapped: every cell is covered four times by copies of one value; the sums
  and the division by 4 are exact."""
  H, W, window, stride, wrap, c, n_win = _geom(SHAPES[1])
  assert set(np.unique(Q.counts(H, W, window, stride, wrap))) == {4}
  x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, H, W, c)).astype(np.float32)).to(dev)
  x_win = torch.empty(2, B, n_win, window[0], window[1], c, device=dev)
  out = torch.empty(2, B, H, W, c, device=dev)
  ops.window_fold_ex(ops.window_gather_ex(x, x_win, window, stride, wrap), out, window, stride, wrap)
  assert torch.equal(out[0].view(torch.int32), x.view(torch.int32))
  assert torch.equal(out[1].view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("kind", ["uniform", "random"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[SHAPE_IDS[0], SHAPE_IDS[2]])
def test_fold_ex_accounts_for_every_window_element(dev, shape, kind):
  """A one-hot batch per window: canvas e of the batch has its single 1.0 at element e of window k.  Every such canvas
  comes back with exactly one nonzero, the restated ww / den, at the cell that element lies on."""
  H, W, window, stride, wrap, c, n_win = _geom(shape)
  h, w = window
  n = h * w * c
  tables = _tables(kind, window)
  den = Q.fold_den(H, W, window, stride, wrap, *(tables or (None, None)))
  ww = np.ones((h, w), np.float32) if tables is None else tables[0][:, None] * tables[1][None, :]
  assert ww.dtype == den.dtype == np.float32
  ys, xs, chs = np.unravel_index(np.arange(n), (h, w, c))
  out = torch.empty(1, n, H, W, c, device=dev)
  dt = _dev_tables(dev, tables)
  for k, (oy, ox) in enumerate(Q.windows(H, W, window, stride, wrap)):
    e = torch.zeros(1, n, n_win, n, device=dev)
    e[0, torch.arange(n, device=dev), k, torch.arange(n, device=dev)] = 1.
    ops.window_fold_ex(e.view(1, n, n_win, h, w, c), out, window, stride, wrap, dt)
    got = out[0].cpu().numpy()
    assert (np.count_nonzero(got.reshape(n, -1), axis=1) == 1).all(), (shape, k)
    cy, cx = (oy + ys) % H, (ox + xs) % W
    want = (ww[ys, xs] / den[cy, cx]).astype(np.float32)
    assert np.array_equal(got[np.arange(n), cy, cx, chs], want), (shape, k)


# ---- 3. ldm_wrap_pad_nhwc --------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", [(4, 6, 4), (5, 7, 3)], ids=["4x6c4", "5x7c3"])
def test_wrap_pad(dev, shape, nb):
  H, W, c = shape
  x = np.random.default_rng(8).standard_normal((nb, H, W, c)).astype(np.float32)
  x[0, 0, 0, 0] = -0.0
  xd = torch.from_numpy(x).to(dev)
  for pad in ((0, 2), (1, 1), (H, W), (0, 0)):
    buf, out = _guarded(dev, (nb, H + 2 * pad[0], W + 2 * pad[1], c))
    assert ops.wrap_pad(xd, pad, out=out) is out
    assert _guards_intact(buf)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(Q.wrap_pad(x, pad))), pad
    assert torch.equal(ops.wrap_pad(xd, pad), out)                   # (allocating its own output)


# ---- 4. the launchers ------------------------------------------------------------------------------------
def test_launcher_rejections(dev):
  x = torch.zeros(1, 8, 8, 4, device=dev)
  win = torch.zeros(2, 1, 16, 4, 4, 4, device=dev)
  can = torch.zeros(2, 1, 8, 8, 4, device=dev)
  wy = torch.ones(4, device=dev)
  s = torch.cuda.current_stream().cuda_stream
  gather = lambda cp, wp, dt, *a: _lib.lib.ldm_window_gather_ex(cp, wp, dt, *a, s)
  fold = lambda wp, cp, hv, *a: _lib.lib.ldm_window_fold_ex(wp, cp, hv, *a, s)
  ok = (1, 8, 8, 4, 4, 4, 2, 2, 1, 1)                                # B, H, W, c, h, w, sy, sx, wrap_y, wrap_x
  cases = [("within the canvas", (1, 8, 8, 4, 9, 4, 2, 2, 1, 1)), ("within the canvas", (1, 8, 8, 4, 4, 9, 2, 2, 0, 1)),
           ("stride", (1, 8, 8, 4, 4, 4, 2, 5, 1, 1)), ("stride", (1, 8, 8, 4, 4, 4, 0, 2, 1, 0)),
           ("stride", (1, 8, 8, 4, 4, 4, 5, 2, 1, 1)), ("bad args", (0, 8, 8, 4, 4, 4, 2, 2, 1, 1)),
           ("bad args", (1, 8, 8, 0, 4, 4, 2, 2, 1, 1)), ("wrap flags", (1, 8, 8, 4, 4, 4, 2, 2, 2, 0)),
           ("wrap flags", (1, 8, 8, 4, 4, 4, 2, 2, 0, -1))]
  for word, a in cases:
    for name, call in (("ldm_window_gather_ex", lambda: gather(x.data_ptr(), win.data_ptr(), _lib.F32, *a)),
                       ("ldm_window_fold_ex", lambda: fold(win.data_ptr(), can.data_ptr(), 2, *a, None, None))):
      assert call() == _lib.ERR_ARG, (name, a)
      assert name in _lib.last_error() and word in _lib.last_error(), (_lib.last_error(), a)
  t = wy.data_ptr()
  for call, word in ((lambda: gather(None, win.data_ptr(), _lib.F32, *ok), "null pointer"),
                     (lambda: gather(x.data_ptr(), None, _lib.F32, *ok), "null pointer"),
                     (lambda: fold(None, can.data_ptr(), 2, *ok, None, None), "null pointer"),
                     (lambda: fold(win.data_ptr(), None, 2, *ok, t, t), "null pointer"),
                     (lambda: gather(x.data_ptr(), win.data_ptr(), 7, *ok), "x_dtype"),
                     (lambda: fold(win.data_ptr(), can.data_ptr(), 0, *ok, None, None), "halves"),
                     (lambda: fold(win.data_ptr(), can.data_ptr(), 3, *ok, t, t), "halves"),
                     (lambda: fold(win.data_ptr(), can.data_ptr(), 2, *ok, t, None), "both"),
                     (lambda: fold(win.data_ptr(), can.data_ptr(), 2, *ok, None, t), "both")):
    assert call() == _lib.ERR_ARG
    assert word in _lib.last_error(), _lib.last_error()
  assert gather(x.data_ptr(), win.data_ptr(), _lib.F32, *ok) == _lib.OK
  assert fold(win.data_ptr(), can.data_ptr(), 2, *ok, t, t) == _lib.OK
  assert fold(win.data_ptr(), can.data_ptr(), 2, *ok, None, None) == _lib.OK
  # ldm_wrap_pad_nhwc
  out = torch.zeros(1, 24, 24, 4, device=dev)
  pad = lambda xp, op, *a: _lib.lib.ldm_wrap_pad_nhwc(xp, op, *a, s)
  for word, xp, op, a in (("null pointer", None, out.data_ptr(), (1, 8, 8, 4, 1, 1)),
                          ("null pointer", x.data_ptr(), None, (1, 8, 8, 4, 1, 1)),
                          ("bad args", x.data_ptr(), out.data_ptr(), (0, 8, 8, 4, 1, 1)),
                          ("bad args", x.data_ptr(), out.data_ptr(), (1, 8, 8, 0, 1, 1)),
                          ("bad args", x.data_ptr(), out.data_ptr(), (1, 0, 8, 4, 0, 1)),
                          ("margin", x.data_ptr(), out.data_ptr(), (1, 8, 8, 4, 9, 1)),
                          ("margin", x.data_ptr(), out.data_ptr(), (1, 8, 8, 4, 1, 9)),
                          ("margin", x.data_ptr(), out.data_ptr(), (1, 8, 8, 4, -1, 1))):
    assert pad(xp, op, *a) == _lib.ERR_ARG, a
    assert "ldm_wrap_pad_nhwc" in _lib.last_error() and word in _lib.last_error(), (_lib.last_error(), a)
  assert pad(x.data_ptr(), out.data_ptr(), 1, 8, 8, 4, 8, 8) == _lib.OK
  # the wrappers pass the launcher's message on
  with pytest.raises(_lib.LdmHipError, match="within the canvas"):
    ops.window_gather_ex(x, win, (9, 4), (2, 2), (True, True))
  with pytest.raises(_lib.LdmHipError, match="stride"):
    ops.window_fold_ex(win, can, (4, 4), (0, 2), (True, True))
  with pytest.raises(_lib.LdmHipError, match="margin"):
    ops.wrap_pad(x, (9, 0))
  with pytest.raises(TypeError):
    ops.window_fold_ex(win, can, (4, 4), (2, 2), (True, True), (wy.to(torch.bfloat16), wy))
  with pytest.raises(TypeError):
    ops.wrap_pad(x.to(torch.bfloat16), (1, 1))
  torch.cuda.synchronize()


@pytest.mark.parametrize("x_dtype", T.DT, ids=["f32", "bf16"])
def test_launchers_take_a_misaligned_pointer_element_wise(dev, x_dtype):
  """c = 4 with pointers aligned to their element only: not rejected, same bits as the aligned launch."""
  H, W, window, stride, wrap, c, n_win = _geom(SHAPES[0])
  x = np.random.default_rng(6).standard_normal((B, H, W, c)).astype(np.float32)
  n_can, n_w = B * H * W * c, 2 * B * n_win * window[0] * window[1] * c
  off = lambda n, dt=torch.float32: torch.full((n + GUARD + 1,), float("nan"), dtype=dt, device=dev)
  clean = lambda buf, n: bool(torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + n:]).all())
  xb = off(n_can)
  xd = xb[1:1 + n_can].view(B, H, W, c)
  xd.copy_(torch.from_numpy(x))
  wb = off(n_w, x_dtype)
  x_win = wb[1:1 + n_w].view(2, B, n_win, window[0], window[1], c)
  assert xd.data_ptr() % 16 and x_win.data_ptr() % (8 if x_dtype == torch.bfloat16 else 16)
  ops.window_gather_ex(xd, x_win, window, stride, wrap)
  want = torch.from_numpy(np.ascontiguousarray(Q.gather(x, window, stride, wrap))).to(x_dtype)
  assert torch.equal(x_win.cpu(), want) and clean(wb, n_w)
  e = np.random.default_rng(7).standard_normal((2, B, n_win, window[0], window[1], c)).astype(np.float32)
  tables = _tables("random", window)
  eb, ob = off(n_w), off(2 * n_can)
  ed = eb[1:1 + n_w].view(2, B, n_win, window[0], window[1], c)
  ed.copy_(torch.from_numpy(e))
  out = ob[1:1 + 2 * n_can].view(2, B, H, W, c)
  ops.window_fold_ex(ed, out, window, stride, wrap, _dev_tables(dev, tables))
  assert np.array_equal(_bits(out.cpu().numpy()), _bits(Q.fold(e, H, W, window, stride, wrap, *tables)))
  assert clean(ob, 2 * n_can)
  n_pad = B * (H + 2) * (W + 4) * c
  pb = off(n_pad)
  padded = pb[1:1 + n_pad].view(B, H + 2, W + 4, c)
  ops.wrap_pad(xd, (1, 2), out=padded)
  assert np.array_equal(_bits(padded.cpu().numpy()), _bits(Q.wrap_pad(x, (1, 2)))) and clean(pb, n_pad)


# ---- 5. the defaults are the section 12 loop -----------------------------------------------------------------
def _x_T(H, W):
  return np.random.default_rng(9).standard_normal((B, H, W, 4)).astype(np.float32)


def _noises(H, W):
  return np.random.default_rng(33).standard_normal((N, B, H, W, 4)).astype(np.float32)


WINDOW, STRIDE, WRAP = (16, 16), (8, 8), (False, True)
H_, W_ = 16, 24                                                      # 3 windows, the last on columns 16 .. 23, 0 .. 7


def test_defaults_are_the_section_12_loop_bit_for_bit(dev, unet_w, txt_w, kl_w):
  """wrap all false, uniform weights, margin 0: the existing loop's latents and images; and the _ex kernels, forced by
  tables of ones on an unwrapped grid, give those bits too."""
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler="ddim", spacing="uniform", eta=0.)
  ids, shape, x_T = T._ids(), [B, 16, 28, 4], _x_T(16, 28)
  want = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T).clone()
  want_lat = s._xt.clone()
  g = s._graph
  got = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T, wrap=(False, False),
                                      window_weights="uniform", wrap_decode_margin=0)
  assert torch.equal(got, want) and torch.equal(s._xt, want_lat) and s._graph is g and not hasattr(s, "_win_wy")
  # a margin without a wrapped axis pads nothing
  assert torch.equal(s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T, wrap_decode_margin=2), want)
  ones = (np.ones(16, np.float32), np.ones(16, np.float32))
  got = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T, window_weights=ones)
  assert s._graph is not g and s._graph_key[-1] == "tables" and s._graph_key[-2] == (False, False)
  assert torch.equal(got, want) and torch.equal(s._xt, want_lat)


# ---- 6. a wrapped canvas with tent weights against the restated loop ------------------------------------------
FORMS = PG.FORMS                                                     # ddim/uniform eta = 1, plms/logsnr, deis/karras
_CACHE = {}


def _oracle(form, w):
  if form not in _CACHE:
    name, spacing, eta = FORMS[form]
    sched = G._schedule(spacing, eta)
    context = O.text_encoder(T._ids(), w["cond_stage_model"], torch.float32)
    wtab = D.weight_table(G.AB, sched["ddim_steps"]).astype(np.float32) if name == "deis" else None
    lat = Q.loop(O, context, w["unet"], _x_T(H_, W_), WINDOW, STRIDE, WRAP, Q.tent(16), Q.tent(16), sched, GS,
                 sampler=name, noises=_noises(H_, W_) if eta else None, weights=wtab, ms_update=D.ms_update,
                 plms_weights=plms_ref.WEIGHTS)
    _CACHE[form] = (lat, O.decoder_forward(lat / LDM["scale_factor"], w["autoencoder"]))
  return _CACHE[form]


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_wrapped_loops_against_oracle(dev, form, dtype, unet_w, txt_w, kl_w):
  name, spacing, eta = FORMS[form]
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = G._ddim_loop_error(dev, dtype, w)
  s = G._sampler(dev, dtype, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, eta=eta)
  got = s.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, x_T=_x_T(H_, W_),
                                      noises=_noises(H_, W_) if eta else None, wrap=WRAP, window_weights="tent")
  assert s._win_key == (B, 3, 16, 16, 4) and tuple(s._x_win.shape) == (6 * B, 16, 16, 4)
  assert np.array_equal(s._win_wy.cpu().numpy(), Q.tent(16)) and np.array_equal(s._win_wx.cpu().numpy(), Q.tent(16))
  assert s._graph_key[-2:] == (WRAP, "tent")
  assert tuple(got.shape) == (B, 8 * H_, 8 * W_, 3) and bool(torch.isfinite(got).all())
  lat, images = _oracle(form, w)
  G._loop_check(f"{form}/{spacing} wrapped panorama latents", s._xt, lat, dtype, base)
  G._loop_check(f"{form}/{spacing} wrapped panorama images", got, images, dtype, base)


def test_the_wrap_and_the_weights_matter(dev, unet_w, txt_w, kl_w):
  """The same canvas with clamped windows, or wrapped with the plain mean, lands elsewhere: the gate tells them
  apart."""
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler="ddim", spacing="uniform", eta=0.)
  run = lambda **kw: s.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, x_T=_x_T(H_, W_),
                                                   **kw).clone()
  tent = run(wrap=WRAP, window_weights="tent")
  for other in (run(), run(wrap=WRAP), run(window_weights="tent"), run(wrap=WRAP, window_weights="gaussian")):
    assert T.rel_err(other, tent.cpu())[0] > 10 * T.LOOP_REL[torch.float32]


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_seam_property(dev, dtype, unet_w, txt_w, kl_w):
  """x_T rolled by one stride along the wrapped axis gives the latents rolled by one stride: the canvas has no edge.
  Within the loop gate, not bit for bit -- the window permutation changes the U-Net's row order."""
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = G._ddim_loop_error(dev, dtype, w)
  s = G._sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="plms", spacing="logsnr", eta=0.)
  x_T = _x_T(H_, W_)
  run = lambda x, **kw: s.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, x_T=x, wrap=WRAP,
                                                      window_weights="tent", **kw)
  run(x_T)
  lat = s._xt.clone()
  run(np.roll(x_T, 8, axis=2))
  G._loop_check("seam: rolled x_T against rolled latents", s._xt, torch.roll(lat, 8, dims=2).cpu(), dtype, base)
  if dtype != torch.float32:
    return
  # with clamped windows the canvas has edges: the same roll lands elsewhere
  c = G._sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="plms", spacing="logsnr", eta=0.)
  c.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, x_T=x_T)
  lat = c._xt.clone()
  c.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, x_T=np.roll(x_T, 8, axis=2))
  assert T.rel_err(c._xt, torch.roll(lat, 8, dims=2).cpu())[0] > base * 20. / 3.


# ---- 7. graph and calls -----------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_graphs_are_keyed(dev, unet_w, txt_w, kl_w):
  ids, x_T, shape = T._ids(), _x_T(H_, W_), [B, H_, W_, 4]
  kw = dict(x_T=x_T, wrap=WRAP, window_weights="tent")
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=True)
  e = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  got = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, **kw).clone()
  g = s._graph
  assert g is not None and s._graph_key[0] == "panorama" and s._graph_key[-2:] == (WRAP, "tent")
  assert torch.equal(got, e.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, **kw)) and e._graph is None
  assert torch.equal(s._xt, e._xt)
  assert torch.equal(got, s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, **kw)) and s._graph is g
  # other weights: another graph; given tables reuse theirs, whatever the values (the buffers are the sampler's)
  wy, wx = s._win_wy, s._win_wx
  gauss = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, **dict(kw, window_weights="gaussian")).clone()
  assert s._graph is not g and not torch.equal(gauss, got) and s._win_wy is wy and s._win_wx is wx
  t1 = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS,
                                     **dict(kw, window_weights=(Q.gaussian(16), Q.gaussian(16)))).clone()
  g = s._graph
  assert torch.equal(t1, gauss) and s._graph_key[-1] == "tables"
  t2 = s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS,
                                     **dict(kw, window_weights=(Q.tent(16), Q.tent(16))))
  assert s._graph is g and torch.equal(t2, got)
  # the other axis, no wrap: other graphs
  s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, x_T=x_T, wrap=(True, True), window_weights="tent")
  assert s._graph_key[-2:] == ((True, True), "tent") and s._win_key == (B, 6, 16, 16, 4)
  assert torch.equal(got, s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, **kw))


@pytest.mark.parametrize("name,rng", list(PG.UPDATES))
def test_a_step_is_one_gather_one_fold_and_one_update(dev, unet_w, txt_w, kl_w, monkeypatch, name, rng):
  s = G._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing="uniform", use_graph=False,
                 noise_source="device" if rng else "host")
  ids, shape = T._ids(), [B, H_, W_, 4]

  def count(**kw):
    """The library calls of one step, after a loop of the same form has allocated the window batch and the tables."""
    loop_kw = dict(wrap=kw.get("wrap", (False, False)), window_weights="tent" if kw.get("tent") else "uniform")
    s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, seed=1, **loop_kw)
    step_kw = dict(wrap=loop_kw["wrap"], weights=(s._win_wy, s._win_wx) if kw.get("tent") else None) if kw else {}
    s._index_dev.fill_(s._loop_start_index(4))
    s._set_loop_start(3)
    proxy = T._CountingLib(ops.lib)
    monkeypatch.setattr(ops, "lib", proxy)
    s._step_panorama(GS, None, True, WINDOW, STRIDE, rng=rng, **step_kw)
    monkeypatch.setattr(ops, "lib", proxy._lib)
    torch.cuda.synchronize()
    return proxy.calls
  update = PG.UPDATES[name, rng]
  plain = count()                                                    # section 12's step, called as section 12 calls it
  assert plain[0] == "ldm_window_gather" and plain[-2] == "ldm_window_fold" and not any("_ex" in c for c in plain)
  calls = {}
  for kw in (dict(wrap=WRAP, tent=True), dict(wrap=WRAP), dict(wrap=(False, False), tent=True)):
    ex = calls[len(calls)] = count(**kw)
    assert ex[0] == "ldm_window_gather_ex" and ex.count("ldm_window_gather_ex") == 1, kw
    assert ex.count("ldm_window_fold_ex") == 1 and ex.count(update) == 1, kw
    assert sum(c.startswith("ldm_cfg_") for c in ex) == 1 and sum("window" in c for c in ex) == 2, kw
    assert ex.index("ldm_window_fold_ex") == len(ex) - 2 > 1 and ex[-1] == update, kw
  # the section 12 step with the pair's names exchanged, nothing else launched: on the same grid (2 windows) with
  # tent weights, and on the wrapped grid (3 windows) with and without them
  assert [c.replace("_ex", "") for c in calls[2]] == plain and calls[0] == calls[1]
  # the loop with its defaults makes the section 12 calls
  rec = T._CountingLib(ops.lib)
  monkeypatch.setattr(ops, "lib", rec)
  s.ddim_p_sample_loop_panorama(ids, shape, WINDOW, STRIDE, GS, seed=1)
  monkeypatch.setattr(ops, "lib", rec._lib)
  assert rec.calls.count("ldm_window_gather") == rec.calls.count("ldm_window_fold") == N
  assert not any("_ex" in c or "wrap_pad" in c for c in rec.calls)


# ---- 8. the wrapped decode --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_wrapped_decode(dev, dtype, unet_w, txt_w, kl_w):
  """Margin 2 on the wrapped x axis: the decoder runs on 16x28 latents (a shape section 12 decodes) and 16 pixel
  columns are cropped from either side."""
  s = G._sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="ddim", spacing="uniform", eta=0.)
  kw = dict(x_T=_x_T(H_, W_), wrap=WRAP, window_weights="tent")
  plain = s.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, **kw).clone()
  lat = s._xt.clone()
  got = s.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, wrap_decode_margin=2, **kw)
  assert torch.equal(s._xt, lat)                                      # the margin only touches the decode
  assert tuple(got.shape) == tuple(plain.shape) == (B, 8 * H_, 8 * W_, 3) and got.is_contiguous()
  padded = ops.wrap_pad(lat, (0, 2))
  assert tuple(padded.shape) == (B, 16, 28, 4)
  assert np.array_equal(padded.cpu().numpy(), Q.wrap_pad(lat.cpu().numpy(), (0, 2)))
  want = s.decode_first_stage(padded)[:, :, 16:16 + 8 * W_]
  assert torch.equal(got, want) and not torch.equal(got, plain)
  assert s._pixel_factor() == 8
  with pytest.raises(ValueError, match="wrap_decode_margin"):
    s.ddim_p_sample_loop_panorama(T._ids(), [B, H_, W_, 4], WINDOW, STRIDE, GS, wrap_decode_margin=25, **kw)
