"""Outpainting and masked-content fill on the GPU: ldm_pushpull_fill against the float64
restatement (tests/pushpull_ref.py), its exact properties, the LDS tail against the per-level launches, and the two
loops as compositions of the fill and the masked img2img loop.

Shapes (B,H,W,c), the smallest at which each thing can go wrong: 1x1 (no level at all), 1x9 (one row), 5x7 (odd in
both axes), 16x16 (tail only), 33x31 (one launched level, then a 17x16 tail), 37x53 (channel quads; one launched level
and a 19x27 tail, two without the tail), 64x48 (element path) and 65x40 (channel quads, two launched levels, then a
17x10 tail).  Masks: sample 0 keeps a centred block, the outpaint shape; sample 1 a sparse 5 % of the cells plus the
corner, with weight 0.5 on one quadrant (the fma branch) -- the samples differ, so a wrong sample stride shows.

Gates.
  Against float64: max |got - ref64| <= 8 x max |ref32 - ref64|, the gap between the restatement in float32 and in
    float64 on the same inputs, computed here on the CPU -- the reference's own error, never the kernel's; the factor
    covers a different but legal order of roundings, not a wrong tap (a tap off by one cell moves a value by the
    image's contrast, 1e-1 and more).  The gaps on these inputs, x in [-1, 1]:
      1x1x1x3 0 (the output is x or 0), 1x1x9x4 1.68e-8, 2x5x7x3 6.15e-8, 2x16x16x4 9.48e-8, 2x33x31x3 1.11e-7,
      2x37x53x4 1.25e-7, 1x64x48x3 3.27e-8, 1x65x40x4 3.03e-8.
  Everything else is torch.equal: kept cells, the two launch structures, the probes (every product of the rule is exact
    for k/8 on 0 / 1 weights), the degenerate masks, in place, run to run, and the loops against their compositions.
Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pushpull_ref as P  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
import test_outpaint_cpu as C  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402

SHAPES, IDS = C.SHAPES, C.IDS
B, HW, N = T.B, T.HW, T.N
_REF = {}


def _case(shape):
  """(x, m, ref64, the float32-against-float64 gap of the restatement), computed once per shape and left unchanged."""
  if shape not in _REF:
    x, m = C.inputs(shape)
    r64 = P.pushpull_ref(x, m, np.float64)
    gap = np.abs(P.pushpull_ref(x, m, np.float32).astype(np.float64) - r64).max()
    for a in (x, m, r64):
      a.setflags(write=False)
    _REF[shape] = (x, m, r64, gap)
  return _REF[shape]


def _fill(dev, x, m, **kw):
  return ops.pushpull_fill(torch.tensor(np.asarray(x, dtype=np.float32), device=dev),
                           torch.tensor(np.asarray(m, dtype=np.float32), device=dev), **kw)


# ---- 1. the kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_float64_kept_cells_and_launch_structures(dev, shape):
  x, m, r64, gap = _case(shape)
  got = _fill(dev, x, m)
  err = (got.cpu().double() - torch.tensor(r64)).abs().max().item()
  print(f"{shape}: max |got - ref64| = {err:.3e}, restatement's float32-float64 gap {gap:.3e}, gate {8 * gap:.3e}")
  assert err <= 8 * gap
  kept = torch.tensor(m == 1)
  assert torch.equal(got.cpu()[kept], torch.tensor(x)[kept])
  assert torch.equal(_fill(dev, x, m, lds_tail=False), got)
  assert torch.equal(_fill(dev, x, m), got)                                      # run to run
  xd, md = torch.tensor(x, device=dev), torch.tensor(m, device=dev)
  for tail in (True, False):
    buf = xd.clone()
    assert ops.pushpull_fill(buf, md, out=buf, lds_tail=tail) is buf
    assert torch.equal(buf, got)                                                 # in place


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_probes(dev, shape):
  """One kept pixel per sample, NaN in every hole of x and all over the workspace: the probe's value everywhere."""
  Bs, H, W, c = shape
  ws = ops.pushpull_workspace(Bs, H, W, c, dev)
  for pos in C.probe_positions(H, W):
    x, m, val = C.probe_inputs(shape, pos)
    want = torch.tensor(np.broadcast_to(val[:, None, None, :], shape))
    for tail in (True, False):
      if ws is not None:
        ws.fill_(float("nan"))
      assert ops.pushpull_workspace(Bs, H, W, c, dev) is ws
      assert torch.equal(_fill(dev, x, m, lds_tail=tail).cpu(), want), (pos, tail)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_degenerate_masks(dev, shape):
  x, m, _, _ = _case(shape)
  for tail in (True, False):
    zeros = _fill(dev, x, np.zeros_like(m), lds_tail=tail)
    assert not zeros.any() and not torch.signbit(zeros).any()
    assert torch.equal(_fill(dev, x, np.ones_like(m), lds_tail=tail).cpu(), torch.tensor(x))
    # NaN and out-of-range weights: clamp(m, 0, 1), a NaN counting as 0
    odd = m.copy()
    odd[m == 0] = np.nan
    odd[m == 1] = 7.
    assert torch.equal(_fill(dev, x, odd, lds_tail=tail), _fill(dev, x, m, lds_tail=tail))


def test_unaligned_pointers_take_the_element_path_with_the_same_bits(dev):
  shape = (2, 37, 53, 4)
  x, m, _, _ = _case(shape)
  want = _fill(dev, x, m, lds_tail=False)
  n = int(np.prod(shape))
  flat = torch.empty(n + 1, dtype=torch.float32, device=dev)
  xs = flat[1:].view(shape)                                                      # 4 bytes past a 16-byte boundary
  xs.copy_(torch.tensor(x))
  assert xs.data_ptr() % 16 == 4
  assert torch.equal(ops.pushpull_fill(xs, torch.tensor(m, device=dev), lds_tail=False), want)


def test_rejections(dev):
  from ldm_tf2_amd import _lib
  x = torch.zeros(1, 4, 4, 3, device=dev)
  k = torch.ones(1, 4, 4, device=dev)
  for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(c=0), dict(lds_tail=2), dict(ws=None), dict(x=None), dict(k=None)):
    a = dict(x=x.data_ptr(), k=k.data_ptr(), ws=ops.pushpull_workspace(1, 4, 4, 3, dev).data_ptr(), B=1, H=4, W=4, c=3,
             lds_tail=1)
    a.update(bad)
    st = _lib.lib.ldm_pushpull_fill(a["x"], a["k"], x.data_ptr(), a["ws"], a["B"], a["H"], a["W"], a["c"], a["lds_tail"],
                                    None)
    assert st == _lib.ERR_ARG and "ldm_pushpull_fill" in _lib.last_error(), bad
  with pytest.raises(AssertionError):
    ops.pushpull_fill(x, k[:, :3])
  with pytest.raises(TypeError):
    ops.pushpull_fill(x, k.double())


# ---- 2. the loops ----------------------------------------------------------------------------------------------
def _slots(s):
  return {n: getattr(s, n) for n in s._GRAPH_SLOTS}


def _same_slots(s, before):
  return all(getattr(s, n) == g if isinstance(g, dict) else getattr(s, n) is g for n, g in before.items())


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_outpaint_is_fill_then_masked_img2img(dev, dtype, use_graph, unet_w, txt_w, kl_w):
  from ldm_tf2_amd.model_runners import latent_mask
  ids = T._ids()
  img, E, Q, _, _ = T._inputs(0.)
  small = np.ascontiguousarray(img[:, :96, :96])
  s = T._sampler(dev, dtype, unet_w, txt_w, kl_w, use_graph=use_graph)
  for pad in ((16, 16, 16, 16), (0, 32, 8, 24)):
    canvas = np.zeros((B, 128, 128, 3), dtype=np.float32)
    keep = np.zeros((B, 128, 128), dtype=np.float32)
    canvas[:, pad[0]:pad[0] + 96, pad[2]:pad[2] + 96] = small
    keep[:, pad[0]:pad[0] + 96, pad[2]:pad[2] + 96] = 1.
    filled = _fill(dev, canvas, keep)
    assert torch.equal(filled.cpu()[:, pad[0]:pad[0] + 96, pad[2]:pad[2] + 96], torch.from_numpy(small))
    lm = latent_mask(keep, 8)
    assert 0 < lm.sum() < lm.size
    want = s.ddim_p_sample_loop_img2img(ids, filled, 5., strength=1.0, mask=lm, encode_noise=E, q_noises=Q).clone()
    want_xt, before, key = s._xt.clone(), _slots(s), s._graph_key
    assert (s._graph is not None) == use_graph
    got = s.ddim_p_sample_loop_outpaint(ids, small, pad, 5., encode_noise=E, q_noises=Q)
    assert tuple(got.shape) == (B, 128, 128, 3)
    assert torch.equal(got, want) and torch.equal(s._xt, want_xt)
    assert _same_slots(s, before) and s._graph_key == key
    # the grey border instead: the same loop from another start
    grey = s.ddim_p_sample_loop_outpaint(ids, small, pad, 5., masked_content="original", encode_noise=E,
                                         q_noises=Q).clone()
    assert not torch.equal(grey, want) and _same_slots(s, before)
    hand = s.ddim_p_sample_loop_img2img(ids, canvas, 5., strength=1.0, mask=lm, encode_noise=E, q_noises=Q)
    assert torch.equal(grey, hand)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_masked_content_on_the_img2img_loop(dev, dtype, unet_w, txt_w, kl_w):
  ids = T._ids()
  img, E, Q, _, mask = T._inputs(0.)
  s = T._sampler(dev, dtype, unet_w, txt_w, kl_w)
  kw = dict(strength=1.0, mask=mask, encode_noise=E, q_noises=Q)
  plain = s.ddim_p_sample_loop_img2img(ids, img, 5., **kw).clone()
  plain_xt, before = s._xt.clone(), _slots(s)
  orig = s.ddim_p_sample_loop_img2img(ids, img, 5., masked_content="original", **kw)
  assert torch.equal(orig, plain) and torch.equal(s._xt, plain_xt) and _same_slots(s, before)
  fill = s.ddim_p_sample_loop_img2img(ids, img, 5., masked_content="fill", **kw).clone()
  fill_xt = s._xt.clone()
  assert not torch.equal(fill, plain) and _same_slots(s, before)
  keep = np.repeat(np.repeat(mask, 8, axis=1), 8, axis=2)
  filled = _fill(dev, img, keep)
  hand = s.ddim_p_sample_loop_img2img(ids, filled, 5., masked_content="original", **kw)
  assert torch.equal(s._xt, fill_xt) and torch.equal(hand, fill)


def test_fill_at_the_fitted_size_with_a_pixel_mask(dev, unet_w, txt_w, kl_w):
  """image_size=: the fill runs after the fit, on the canvas the encoder sees, with the pixel mask brought there by
  fill_keep_mask."""
  from ldm_tf2_amd.model_runners import fill_keep_mask
  ids = T._ids()
  _, E, Q, _, _ = T._inputs(0.)
  g = np.random.default_rng(8)
  src = g.uniform(-1., 1., (B, 80, 112, 3)).astype(np.float32)
  pm = np.ones((B, 80, 112), dtype=np.uint8)
  pm[:, 20:60, 30:90] = 0
  s = T._sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  kw = dict(strength=1.0, encode_noise=E, q_noises=Q)
  for fit in ("stretch", "crop"):
    s.ddim_p_sample_loop_img2img(ids, src, 5., mask=pm, image_size=(128, 128), fit=fit, masked_content="fill", **kw)
    got = s._xt.clone()
    fitted = s._fit_images(s._init_images(src, B), (128, 128), fit, "lanczos3")
    keep = fill_keep_mask(pm, (80, 112), (128, 128), 8, fit)
    filled = ops.pushpull_fill(fitted, torch.from_numpy(keep).to(dev))
    s.ddim_p_sample_loop_img2img(ids, filled, 5., mask=s._fit_mask(pm, (80, 112), (128, 128), fit), **kw)
    assert torch.equal(s._xt, got), fit


# ---- 3. CLI ----------------------------------------------------------------------------------------------------
def test_cli_outpaint(dev, tmp_path):
  """`ldm_sampling.outpaint` through main(): the images file holds what the loop returns for the same config and seed."""
  import yaml
  from ldm_tf2_amd import run_ldm_sampler as R
  from ldm_tf2_amd.tokenizer import get_token_ids
  unet = dict(model_channels=64, out_channels=4, num_blocks=2, attention_resolutions=[4, 2, 1], dropout_rate=0.1,
              channel_mult=[1, 2, 4, 4], num_heads=8)
  txt = dict(vocab_size=200, encoder_stack_size=2, hidden_size=128, num_heads=4, size_per_head=32,
             max_seq_len=77, filter_size=256, dropout_rate=0.1)
  kl = dict(latent_channels=4, channels=64, num_blocks=2, attention_resolutions=[], dropout_rate=0.,
            multipliers=[1, 2, 4, 4], resample_with_conv=True)
  prompt = "a painting of a virus monster playing guitar"
  words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "painting", "of", "virus", "monster", "play", "##ing",
           "guitar", "the", ","]
  words += [f"tok{i}" for i in range(200 - len(words))]
  (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n", encoding="utf-8")
  img = np.random.default_rng(5).integers(0, 256, size=(96, 112, 3)).astype(np.uint8)
  np.save(tmp_path / "init.npy", img)
  pad = [16, 16, 0, 16]
  cfg = {
      "ldm_sampling": {"autoencoder_type": "kl", "latent_shape": [2, 16, 16, 4], "guidance_scale": 5.0,
                       "text_prompt": prompt, "vocab_dir": str(tmp_path), "sample_save_progress": False,
                       "init_image": str(tmp_path / "init.npy"), "outpaint": pad},
      "pre_ckpt_paths": {"cond_stage_model": None, "unet": None, "autoencoder": None},
      "cond_stage_model": txt, "autoencoder_kl": kl, "unet": unet, "ldm": T.LDM,
  }
  path = tmp_path / "config.yaml"
  path.write_text(yaml.safe_dump(cfg))
  out = tmp_path / "images.npy"
  R.main(["--config_path", str(path), "--dtype", "f32", "--seed", "7", "--out", str(out)])
  got = np.load(out)
  assert got.dtype == np.uint8 and got.shape == (2, 128, 128, 3)
  s = R.build_from_config(cfg, dtype=torch.float32, verbose=False)
  ids = get_token_ids(prompt, 2, str(tmp_path), 77)
  images = img.astype(np.float32) / np.float32(127.5) - np.float32(1.0)
  want = R.tensor_to_image(s.ddim_p_sample_loop_outpaint(ids, images, tuple(pad), 5.0, seed=7))
  assert np.array_equal(got, want)
  grey = R.tensor_to_image(s.ddim_p_sample_loop_outpaint(ids, images, tuple(pad), 5.0, seed=7,
                                                         masked_content="original"))
  assert not np.array_equal(got, grey)
