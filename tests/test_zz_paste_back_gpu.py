"""Pixel-space paste-back on the GPU: ldm_mask_feather, ldm_keep_stats and ldm_paste_back
against the float64 restatement (tests/paste_ref.py), their exact properties, the LDS-tiled feather against the four
launches, and the two loops as compositions of the loop as it was and the three ops.

Shapes (B,H,W,c), the smallest at which each thing can go wrong: 1x1 (degenerate), 1x9 (one row, r larger than the
image), 5x7 (odd extents), 33x31 and 65x40 (a 32-pixel tile edge + 1), 37x53 (channel quads; 2 x 2 tiles with ragged
edges), 64x48 (element path).  Sigmas 0, 0.5, 1.5, 4 (r = 0, 2, 5, 12: the LDS tile) and 6 (r = 18: past the tile's 16,
the four launches either way).  Masks (test_paste_back_cpu.masks): sample 0 keeps a centred box, sample 1 all but a
sparse 5 % and a corner, its holes holding 0, 0.5 and NaN -- the samples differ, so a wrong sample stride shows.

Gates.
  Feather against float64: max |got - ref64| <= (4r + 6) 2^-24 -- two chains of 2r + 1 fmas over non-negative terms of
    total at most 1, each rounding at most 2^-24, and the final subtraction (test_paste_back_cpu's docstring).  A wrong
    or missing tap moves a value by at least the smallest tap, 2.6e-4 at sigma 0.5 and 1.1e-3 at sigma 4; the gate is
    8.3e-7 and 3.2e-6 there.
  Statistics on uniform inputs: |sum - sum64| <= n 2^-24 sum |term|, which holds for any order of n float32 additions.
    On the exact probes (values k/8: every product and partial sum is exact in float32) the sums are torch.equal.
  Gain and offset: within 2^-23 max(|value|, |mean_o|) of the float64 formulas, one float32 ulp.
  Paste with gain and offset: max |got - ref64| <= 6 2^-24 max(1, max |o|, max |d'|): the fma of d', the subtraction
    and the blend's fma round once each at magnitudes up to twice that maximum.
  Everything else is torch.equal.
Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import paste_ref as P  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
import test_paste_back_cpu as C  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import _lib, ops  # noqa: E402
from ldm_tf2_amd.feather import feather_radius  # noqa: E402

SHAPES, IDS, SIGMAS, EPS = C.SHAPES, C.IDS, C.SIGMAS, C.EPS
B, HW, N = T.B, T.HW, T.N
_REF = {}


def _feather_case(shape, sigma):
  """(m, ref64) of a shape and sigma, computed once and left unchanged."""
  key = (shape, sigma)
  if key not in _REF:
    m = C.masks(shape)
    ref = P.feather_ref(m, sigma, np.float64)
    m.setflags(write=False)
    ref.setflags(write=False)
    _REF[key] = (m, ref)
  return _REF[key]


def _t(dev, a, dtype=np.float32):
  return torch.tensor(np.asarray(a, dtype=dtype), device=dev)


# ---- 1. the feather ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_feather_against_float64_and_its_exact_properties(dev, shape):
  Bs, H, W, _ = shape
  ws = ops.mask_feather_workspace(Bs, H, W, dev)
  for sigma in SIGMAS:
    m, ref = _feather_case(shape, sigma)
    r = feather_radius(sigma)
    md = _t(dev, m)
    got = ops.mask_feather(md, sigma)
    err = (got.cpu().double() - torch.tensor(ref)).abs().max().item()
    print(f"{shape} sigma {sigma}: max |got - ref64| = {err:.3e}, gate {(4 * r + 6) * EPS:.3e}")
    assert err <= (4 * r + 6) * EPS, sigma
    g = got.cpu().numpy()
    hole = ~P.kept(m)
    assert torch.equal(got.cpu()[torch.tensor(hole)], torch.zeros(int(hole.sum())))
    deep = C.far_from_holes(m, r)
    assert torch.equal(got.cpu()[torch.tensor(deep)], torch.ones(int(deep.sum())))
    assert g.min() >= 0 and g.max() <= 1
    if sigma == 0:
      assert torch.equal(got.cpu(), torch.tensor(P.kept(m).astype(np.float32)))
    # the two launch structures, run to run, a workspace full of NaN, an `out` of the caller's
    ws.fill_(float("nan"))
    assert ops.mask_feather_workspace(Bs, H, W, dev) is ws
    four = ops.mask_feather(md, sigma, lds_tile=False)
    assert torch.equal(four, got), sigma
    assert torch.equal(ops.mask_feather(md, sigma, lds_tile=True), got)
    ws.fill_(float("nan"))
    buf = torch.full((Bs, H, W), float("nan"), device=dev)
    assert ops.mask_feather(md, sigma, out=buf, lds_tile=False) is buf and torch.equal(buf, got)


def test_feather_degenerate_masks_and_one_mask_for_the_batch(dev):
  shape = (2, 37, 53, 4)
  m = C.masks(shape)
  for sigma in (0., 1.5, 6.):
    for tile in (True, False):
      ones = ops.mask_feather(_t(dev, np.ones_like(m)), sigma, lds_tile=tile)
      assert torch.equal(ones, torch.ones_like(ones))                            # the border does not fade
      assert not ops.mask_feather(_t(dev, np.zeros_like(m)), sigma, lds_tile=tile).any()
      odd = m.copy()
      odd[~P.kept(m)] = np.nan
      odd[P.kept(m)] = 7.
      want = ops.mask_feather(_t(dev, m), sigma, lds_tile=tile)
      assert torch.equal(ops.mask_feather(_t(dev, odd), sigma, lds_tile=tile), want)
      # each sample alone is the sample in the batch: no sample reads another's mask
      for b in range(2):
        assert torch.equal(ops.mask_feather(_t(dev, m[b:b + 1]), sigma, lds_tile=tile), want[b:b + 1])


# ---- 2. the statistics -------------------------------------------------------------------------------------
def _probe_images(shape, m, seed):
  """o, d with values k/8, k in -8 .. 8, and NaN in every hole."""
  g = np.random.default_rng([seed, 2, *shape])
  o = (g.integers(-8, 9, shape) / 8).astype(np.float32)
  d = (g.integers(-8, 9, shape) / 8).astype(np.float32)
  hole = np.broadcast_to(~P.kept(m), shape[:3])
  o[hole], d[hole] = np.nan, np.nan
  return o, d


def _check_gain_offset(stats, gain, offset):
  a, b = P.gain_offset_ref(stats)
  n = np.maximum(stats[..., 0], 1.)
  mo = np.abs(stats[..., 1] / n)
  ea = np.abs(gain.cpu().double().numpy() - a)
  eb = np.abs(offset.cpu().double().numpy() - b)
  print(f"gain err {ea.max():.3e}, offset err {eb.max():.3e}")
  assert (ea <= 2. ** -23 * np.maximum(np.abs(a), mo)).all(), (ea, a)
  assert (eb <= 2. ** -23 * np.maximum(np.abs(b), mo)).all(), (eb, b)
  assert (gain.cpu().numpy() >= 0.5).all() and (gain.cpu().numpy() <= 2.).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stats_exact_probes(dev, shape):
  m = C.masks(shape)
  o, d = _probe_images(shape, m, 0)
  want = P.keep_stats_ref(o, d, m)
  assert np.isfinite(want).all()
  stats, gain, offset = ops.keep_stats(_t(dev, o), _t(dev, d), _t(dev, m))
  assert stats.dtype == torch.float64 and tuple(stats.shape) == (shape[0], shape[3], 5)
  assert torch.equal(stats.cpu(), torch.tensor(want))
  _check_gain_offset(want, gain, offset)
  again = ops.keep_stats(_t(dev, o), _t(dev, d), _t(dev, m))
  assert all(torch.equal(x, y) for x, y in zip(again, (stats, gain, offset)))       # run to run


def test_stats_several_chunks_and_one_mask_for_the_batch(dev):
  """2 x 96 x 128 x 3: three workgroup chunks of 4096 pixels per sample, still exact on the probes; a [1,H,W] mask is
  the mask tiled over the batch."""
  shape = (2, 96, 128, 3)
  assert _lib.lib.ldm_keep_stats_partials(96, 128) == 3
  m = C.masks(shape)
  for mm in (m, m[1:2]):
    o, d = _probe_images(shape, mm, 1)
    want = P.keep_stats_ref(o, d, mm)
    stats, gain, offset = ops.keep_stats(_t(dev, o), _t(dev, d), _t(dev, mm))
    assert torch.equal(stats.cpu(), torch.tensor(want))
    _check_gain_offset(want, gain, offset)
    tiled = ops.keep_stats(_t(dev, o), _t(dev, d), _t(dev, np.broadcast_to(mm, shape[:3]).copy()))
    assert all(torch.equal(x, y) for x, y in zip(tiled, (stats, gain, offset)))


@pytest.mark.parametrize("shape", [(2, 37, 53, 4), (1, 64, 48, 3), (2, 96, 128, 3)], ids=["2x37x53x4", "1x64x48x3",
                                                                                          "2x96x128x3"])
def test_stats_uniform_inputs(dev, shape):
  m = C.masks(shape)
  o, d = C.images(shape)
  keep = np.broadcast_to(P.kept(m), shape[:3])
  stats = ops.keep_stats(_t(dev, o), _t(dev, d), _t(dev, m))[0].cpu().numpy()
  want = P.keep_stats_ref(o, d, m)
  assert np.array_equal(stats[..., 0], want[..., 0])
  for b in range(shape[0]):
    n = want[b, 0, 0]
    for j, x in ((1, o), (2, o.astype(np.float64) ** 2), (3, d), (4, d.astype(np.float64) ** 2)):
      mag = np.abs(x[b][keep[b]].astype(np.float64)).sum(axis=0)                    # per channel
      err = np.abs(stats[b, :, j] - want[b, :, j])
      print(f"{shape} sample {b} sum {j}: err {err.max():.3e}, bound {(n * EPS * mag).min():.3e}")
      assert (err <= n * EPS * mag).all(), (b, j)


def test_stats_degenerate_cases_are_the_identity(dev):
  shape = (2, 33, 31, 3)
  m = C.masks(shape)
  o, d = C.images(shape)
  od, dd = _t(dev, o), _t(dev, d)
  stats, gain, offset = ops.keep_stats(od, dd, _t(dev, np.zeros_like(m)))           # n = 0
  assert not stats.any() and torch.equal(gain, torch.ones_like(gain)) and not offset.any()
  one = np.zeros_like(m)
  one[:, 3, 4] = 1.
  stats, gain, offset = ops.keep_stats(od, dd, _t(dev, one))                        # n = 1
  assert torch.equal(stats[..., 0].cpu(), torch.ones(2, 3, dtype=torch.float64))
  assert torch.equal(gain, torch.ones_like(gain))
  assert torch.equal(offset.cpu(), torch.tensor(o[:, 3, 4].astype(np.float64) - d[:, 3, 4]).float())
  flat = np.full_like(d, 0.25)
  stats, gain, offset = ops.keep_stats(od, _t(dev, flat), _t(dev, m))               # var_d = 0
  assert torch.equal(gain, torch.ones_like(gain))
  _check_gain_offset(P.keep_stats_ref(o, flat, m), gain, offset)


# ---- 3. the paste ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_paste(dev, shape):
  m = C.masks(shape)
  o, d = C.images(shape)
  hole = ~P.kept(m)
  d[hole] = np.where(np.arange(int(hole.sum()) * shape[3]).reshape(int(hole.sum()), shape[3]) % 2, d[hole], np.float32(-0.))
  on = o.copy()
  on[hole] = np.nan                                                               # o in a hole is never used
  od, dd = _t(dev, on), _t(dev, d)
  g = np.random.default_rng([3, *shape])
  gain = g.uniform(0.5, 2., (shape[0], shape[3])).astype(np.float32)
  offset = g.uniform(-0.5, 0.5, (shape[0], shape[3])).astype(np.float32)
  for sigma in (0., 1.5):
    w = ops.mask_feather(_t(dev, m), sigma)
    wn = w.cpu().numpy()
    full = torch.tensor(wn >= 1)
    # without gain: the kept pixels are o's bits, the holes d's (-0 stays -0)
    got = ops.paste_back(od, dd, w)
    assert torch.equal(got.cpu()[full], torch.tensor(o)[full])
    hd, hg = torch.tensor(d)[torch.tensor(hole)], got.cpu()[torch.tensor(hole)]
    assert torch.equal(hg, hd) and torch.equal(torch.signbit(hg), torch.signbit(hd))
    assert torch.isfinite(got).all()
    ref = P.paste_ref(on, d, wn)
    assert (got.cpu().double() - torch.tensor(ref)).abs().max().item() <= 6 * EPS * max(1., np.abs(o).max(),
                                                                                        np.abs(d).max())
    # with gain and offset
    got_g = ops.paste_back(od, dd, w, _t(dev, gain), _t(dev, offset))
    ref_g = P.paste_ref(on, d, wn, gain, offset)
    dref = gain.astype(np.float64)[:, None, None, :] * d + offset.astype(np.float64)[:, None, None, :]
    bound = 6 * EPS * max(1., np.abs(o).max(), np.abs(dref).max())
    err = (got_g.cpu().double() - torch.tensor(ref_g)).abs().max().item()
    print(f"{shape} sigma {sigma}: with gain, max |got - ref64| = {err:.3e}, gate {bound:.3e}")
    assert err <= bound
    assert torch.equal(got_g.cpu()[full], torch.tensor(o)[full])
    # in place, and run to run
    for kw, want in ((dict(), got), (dict(gain=_t(dev, gain), offset=_t(dev, offset)), got_g)):
      buf = dd.clone()
      assert ops.paste_back(od, buf, w, out=buf, **kw) is buf and torch.equal(buf, want)
      assert torch.equal(ops.paste_back(od, dd, w, **kw), want)


def test_paste_one_map_for_the_batch_and_unaligned_pointers(dev):
  shape = (2, 37, 53, 4)
  m = C.masks(shape)
  o, d = C.images(shape)
  od, dd = _t(dev, o), _t(dev, d)
  gain, offset = _t(dev, np.full((2, 4), 1.25)), _t(dev, np.full((2, 4), -0.125))
  w1 = ops.mask_feather(_t(dev, m[1:2]), 1.5)                                     # [1,H,W]
  assert tuple(w1.shape) == (1, 37, 53)
  want = ops.paste_back(od, dd, w1.expand(2, 37, 53).contiguous(), gain, offset)
  assert torch.equal(ops.paste_back(od, dd, w1, gain, offset), want)
  # 4 bytes past a 16-byte boundary: the element path, with the channel quads' bits
  n = int(np.prod(shape))
  views = []
  for src in (od, dd, None):
    flat = torch.empty(n + 1, dtype=torch.float32, device=dev)
    v = flat[1:].view(shape)
    if src is not None:
      v.copy_(src)
    assert v.data_ptr() % 16 == 4
    views.append(v)
  for kw in (dict(), dict(gain=gain, offset=offset)):
    quad = ops.paste_back(od, dd, w1, **kw)
    assert torch.equal(ops.paste_back(views[0], views[1], w1, out=views[2], **kw), quad)
  stats = ops.keep_stats(od, dd, _t(dev, m))
  assert all(torch.equal(x, y) for x, y in zip(ops.keep_stats(views[0], views[1], _t(dev, m)), stats))


def test_rejections(dev):
  x = torch.zeros(1, 4, 4, 3, device=dev)
  k = torch.ones(1, 4, 4, device=dev)
  taps = torch.ones(1, device=dev)
  ws = ops.mask_feather_workspace(1, 4, 4, dev)
  part = torch.zeros(64, device=dev)
  st = torch.zeros(1, 5, 5, dtype=torch.float64, device=dev)
  ga, of = torch.ones(1, 5, device=dev), torch.zeros(1, 5, device=dev)
  L = _lib.lib
  for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(r=-1), dict(r=49), dict(lds=2), dict(kb=3), dict(keep=None),
              dict(taps=None), dict(out=None), dict(ws=None, lds=0), dict(ws=None, r=17)):
    a = dict(keep=k.data_ptr(), kb=16, taps=taps.data_ptr(), r=0, out=k.data_ptr(), ws=ws.data_ptr(), B=1, H=4, W=4, lds=1)
    a.update(bad)
    s = L.ldm_mask_feather(a["keep"], a["kb"], a["taps"], a["r"], a["out"], a["ws"], a["B"], a["H"], a["W"], a["lds"], None)
    assert s == _lib.ERR_ARG and "ldm_mask_feather" in _lib.last_error(), bad
  for bad in (dict(c=5), dict(c=0), dict(B=0), dict(H=0), dict(kb=3), dict(o=None), dict(part=None), dict(gain=None)):
    a = dict(o=x.data_ptr(), part=part.data_ptr(), gain=ga.data_ptr(), kb=16, B=1, H=4, W=4, c=3)
    a.update(bad)
    s = L.ldm_keep_stats(a["o"], x.data_ptr(), k.data_ptr(), a["kb"], a["part"], st.data_ptr(), a["gain"], of.data_ptr(),
                         a["B"], a["H"], a["W"], a["c"], None)
    assert s == _lib.ERR_ARG and "ldm_keep_stats" in _lib.last_error(), bad
  for bad in (dict(c=0), dict(B=0), dict(W=0), dict(wb=3), dict(o=None), dict(w=None), dict(gain=None),
              dict(offset=None)):
    a = dict(o=x.data_ptr(), w=k.data_ptr(), wb=16, gain=ga.data_ptr(), offset=of.data_ptr(), B=1, H=4, W=4, c=3)
    a.update(bad)
    s = L.ldm_paste_back(a["o"], x.data_ptr(), a["w"], a["wb"], a["gain"], a["offset"], x.data_ptr(), a["B"], a["H"],
                         a["W"], a["c"], None)
    assert s == _lib.ERR_ARG and "ldm_paste_back" in _lib.last_error(), bad
  with pytest.raises(AssertionError):
    ops.paste_back(x, x, k[:, :3])
  with pytest.raises(TypeError):
    ops.mask_feather(k.double(), 1.)
  with pytest.raises(ValueError, match="mask_feather"):
    ops.mask_feather(k, 17.)
  with pytest.raises(_lib.LdmHipError, match="at most 4 channels"):
    ops.keep_stats(torch.zeros(1, 4, 4, 5, device=dev), torch.zeros(1, 4, 4, 5, device=dev), k)


# ---- 4. the loops ------------------------------------------------------------------------------------------
def _slots(s):
  return {n: getattr(s, n) for n in s._GRAPH_SLOTS}


def _same_slots(s, before):
  return all(getattr(s, n) == g if isinstance(g, dict) else getattr(s, n) is g for n, g in before.items())


def _compose(dev, images, originals, keep, sigma, color_match):
  """The three ops by hand on a clone of the loop's images."""
  o = _t(dev, originals) if not isinstance(originals, torch.Tensor) else originals
  m = _t(dev, keep)
  w = ops.mask_feather(m, sigma)
  gain = offset = None
  if color_match:
    _, gain, offset = ops.keep_stats(o, images, m)
  return ops.paste_back(o, images, w, gain, offset), w, gain, offset


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_img2img_paste_back_is_the_loop_then_the_three_ops(dev, dtype, unet_w, txt_w, kl_w):
  ids = T._ids()
  img, E, Q, _, mask = T._inputs(0.)
  s = T._sampler(dev, dtype, unet_w, txt_w, kl_w)
  kw = dict(strength=1.0, mask=mask, encode_noise=E, q_noises=Q)
  plain = s.ddim_p_sample_loop_img2img(ids, img, 5., **kw).clone()
  plain_xt, before, key = s._xt.clone(), _slots(s), s._graph_key
  assert s.last_paste_weights() is None
  # the keywords at their defaults are the call without them
  same = s.ddim_p_sample_loop_img2img(ids, img, 5., paste_back=False, mask_feather=0., color_match=False, **kw)
  assert torch.equal(same, plain) and _same_slots(s, before) and s.last_paste_weights() is None
  keep = np.repeat(np.repeat(mask, 8, axis=1), 8, axis=2)
  kept = torch.tensor(keep == 1)
  for sigma, cm in ((1.5, True), (0., False), (4., False)):
    got = s.ddim_p_sample_loop_img2img(ids, img, 5., paste_back=True, mask_feather=sigma, color_match=cm, **kw).clone()
    want, w, gain, offset = _compose(dev, plain.clone(), img, keep, sigma, cm)
    assert torch.equal(got, want), (sigma, cm)
    assert torch.equal(s._xt, plain_xt) and _same_slots(s, before) and s._graph_key == key
    assert torch.equal(s.last_paste_weights(), w)
    if cm:
      assert torch.equal(s.last_color_match()[0], gain) and torch.equal(s.last_color_match()[1], offset)
      assert not torch.equal(gain, torch.ones_like(gain))
    else:
      assert s.last_color_match() == (None, None)
    assert not torch.equal(got, plain)
    full = (w >= 1).cpu()
    assert full.any() and torch.equal(got.cpu()[full], torch.tensor(img)[full])
    if sigma == 0:                               # everything the mask keeps is the init image, bit for bit
      assert torch.equal(got.cpu()[kept], torch.tensor(img)[kept])
      assert torch.equal(got.cpu()[~kept], plain.cpu()[~kept])
  # masked_content="fill": the originals are the images before the fill
  filled = s.ddim_p_sample_loop_img2img(ids, img, 5., masked_content="fill", **kw).clone()
  got = s.ddim_p_sample_loop_img2img(ids, img, 5., masked_content="fill", paste_back=True, **kw)
  assert torch.equal(got.cpu()[kept], torch.tensor(img)[kept]) and torch.equal(got.cpu()[~kept], filled.cpu()[~kept])


def test_paste_back_at_the_fitted_size_with_a_pixel_mask(dev, unet_w, txt_w, kl_w):
  """image_size=: the originals are the fitted images, the keep is the pixel mask brought there by fill_keep_mask, and
  nothing the latent mask keeps is left unpasted."""
  from ldm_tf2_amd.model_runners import fill_keep_mask
  ids = T._ids()
  _, E, Q, _, _ = T._inputs(0.)
  g = np.random.default_rng(8)
  src = g.uniform(-1., 1., (B, 80, 112, 3)).astype(np.float32)
  pm = np.ones((B, 80, 112), dtype=np.uint8)
  pm[:, 20:60, 30:90] = 0
  s = T._sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  kw = dict(strength=1.0, encode_noise=E, q_noises=Q, mask=pm, image_size=(128, 128), fit="stretch")
  plain = s.ddim_p_sample_loop_img2img(ids, src, 5., **kw).clone()
  got = s.ddim_p_sample_loop_img2img(ids, src, 5., paste_back=True, mask_feather=1.5, color_match=True, **kw).clone()
  fitted = s._fit_images(s._init_images(src, B), (128, 128), "stretch", "lanczos3")
  keep = fill_keep_mask(pm, (80, 112), (128, 128), 8, "stretch")
  want, _, _, _ = _compose(dev, plain.clone(), fitted, keep, 1.5, True)
  assert torch.equal(got, want)
  sharp = s.ddim_p_sample_loop_img2img(ids, src, 5., paste_back=True, **kw)
  lm = np.repeat(np.repeat(s._fit_mask(pm, (80, 112), (128, 128), "stretch"), 8, axis=1), 8, axis=2) == 1
  assert lm.any() and (lm <= (keep == 1)).all()
  assert torch.equal(sharp[torch.tensor(lm, device=dev)], fitted[torch.tensor(lm, device=dev)])


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_outpaint_paste_back_is_the_loop_then_the_three_ops(dev, use_graph, unet_w, txt_w, kl_w):
  ids = T._ids()
  img, E, Q, _, _ = T._inputs(0.)
  small = np.ascontiguousarray(img[:, :96, :96])
  s = T._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=use_graph)
  pad = (0, 32, 8, 24)
  canvas = np.zeros((B, 128, 128, 3), dtype=np.float32)
  keep = np.zeros((1, 128, 128), dtype=np.float32)
  canvas[:, :96, 8:104] = small
  keep[:, :96, 8:104] = 1.
  kw = dict(encode_noise=E, q_noises=Q)
  plain = s.ddim_p_sample_loop_outpaint(ids, small, pad, 5., **kw).clone()
  plain_xt, before = s._xt.clone(), _slots(s)
  same = s.ddim_p_sample_loop_outpaint(ids, small, pad, 5., paste_back=False, mask_feather=0., color_match=False, **kw)
  assert torch.equal(same, plain)
  got = s.ddim_p_sample_loop_outpaint(ids, small, pad, 5., paste_back=True, mask_feather=1.5, color_match=True,
                                      **kw).clone()
  want, w, gain, offset = _compose(dev, plain.clone(), canvas, keep, 1.5, True)
  assert torch.equal(got, want) and torch.equal(s._xt, plain_xt) and _same_slots(s, before)
  assert tuple(s.last_paste_weights().shape) == (1, 128, 128) and torch.equal(s.last_paste_weights(), w)
  assert torch.equal(s.last_color_match()[0], gain) and torch.equal(s.last_color_match()[1], offset)
  sharp = s.ddim_p_sample_loop_outpaint(ids, small, pad, 5., paste_back=True, **kw)
  assert torch.equal(sharp[:, :96, 8:104].cpu(), torch.tensor(small))
  box = torch.zeros(B, 128, 128, dtype=torch.bool)
  box[:, :96, 8:104] = True
  assert torch.equal(sharp.cpu()[~box], plain.cpu()[~box])


def test_the_defaults_make_the_calls_they_made(dev, unet_w, txt_w, kl_w, monkeypatch):
  """Eager loops through a counting proxy of the library: the keywords at their defaults add no call, paste_back adds
  exactly its three (two without color_match), after everything else."""
  ids = T._ids()
  img, E, Q, _, mask = T._inputs(0.)
  s = T._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  kw = dict(strength=0.5, mask=mask, encode_noise=E, q_noises=Q)
  s.ddim_p_sample_loop_img2img(ids, img, 5., **kw)                                # (warm: buffers, tables)
  s.ddim_p_sample_loop_img2img(ids, img, 5., paste_back=True, mask_feather=1.5, color_match=True, **kw)
  calls = []
  for extra in (dict(), dict(paste_back=False, mask_feather=0., color_match=False),
                dict(paste_back=True, mask_feather=1.5, color_match=True), dict(paste_back=True)):
    proxy = T._CountingLib(ops.lib)
    monkeypatch.setattr(ops, "lib", proxy)
    s.ddim_p_sample_loop_img2img(ids, img, 5., **kw, **extra)
    monkeypatch.setattr(ops, "lib", proxy._lib)
    torch.cuda.synchronize()
    calls.append(proxy.calls)
  print([len(c) for c in calls])
  assert len(calls[0]) > 10 and calls[1] == calls[0]
  assert calls[2] == calls[0] + ["ldm_mask_feather", "ldm_keep_stats", "ldm_paste_back"]
  assert calls[3] == calls[0] + ["ldm_mask_feather", "ldm_paste_back"]
