"""Two-pass high-resolution sampling on the GPU: ldm_resize_nhwc against the float64 restatement
(tests/hires_ref.py), every output element and every tap accounted for, and ddim_p_sample_loop_hires against the loop
composed from the oracle, its graphs, its seeds and its solvers.

Gates.
  Kernel, nearest and the identity size: bit for bit.
  Kernel, bilinear and bicubic: max |got - float64 restatement| <= max(2 * e32, 2^-23 * max|x|), where e32 is the same
    error of the float32 NumPy emulation of the same formula (hires_ref.resize32) on the same inputs, computed in the
    test; the factor 2 covers fma contraction and the order of the sum.
  Probes: the same gate on the per-source-pixel sums, with max|x| = 1.
  Loop: the error of ddim_p_sample_loop_img2img against its composed oracle at 32x32 latents, same weights, dtype,
    strength and scale, measured in the same run, times LOOP_MARGIN = 1.  Between a float32 and a float64 run of the two
    restatements on the oracle's models at these shapes the two-pass loop drifts 0.79 (nearest), 0.87 (bilinear) and
    0.84 (bicubic) times as far as img2img at 32x32 in the latents (3.33e-6, 3.67e-6, 3.53e-6 against 4.22e-6) and 0.73,
    0.73, 0.78 times in the images (4.68e-6, 4.71e-6, 5.02e-6 against 6.45e-6): below 1, so rounded up to a power of
    two the margin is 1.
Tiny models, ids and LDM are those of tests/test_img2img_gpu.py: B = 2, N = 10, 16x16 -> 32x32 latents, strength 0.5.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hires_ref as H  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import _lib, ops  # noqa: E402
from ldm_tf2_amd._lib import LdmHipError  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, N, LDM = T.B, T.N, T.LDM
LO, HI = [B, 16, 16, 4], [B, 32, 32, 4]
STRENGTH, K, GS = 0.5, 5, 5.
FLOOR = 2.0 ** -23
LOOP_MARGIN = 1.                               # (the drift ratio 0.73 .. 0.87 rounded up to a power of two, see above)
CANARY = -12288.
PAD = 64                                       # floats around every output (a multiple of 4: the view stays aligned)
CASES = [(4, (5, 7), (16, 9), 0), (4, (16, 16), (32, 32), 0), (4, (16, 24), (8, 12), 0), (4, (1, 1), (4, 4), 0),
         (4, (16, 16), (16, 16), 0), (3, (8, 8), (12, 20), 0), (4, (5, 7), (16, 9), 1)]
CASE_IDS = ["c4-5x7-16x9", "c4-16x16-32x32", "c4-16x24-8x12", "c4-1x1-4x4", "c4-16x16-16x16", "c3-8x8-12x20",
            "c4-5x7-16x9-offset1"]


def _x(shape, seed=0):
  x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
  x.flat[0] = -0.0
  return x


def _resize_padded(dev, x, size, mode, offset=0):
  """The entry on `x` into a view `offset` floats into a canary-filled buffer -> the result (CPU), pads checked."""
  b, c = x.shape[0], x.shape[3]
  numel = b * size[0] * size[1] * c
  buf = torch.full((numel + 2 * PAD + offset,), CANARY, dtype=torch.float32, device=dev)
  out = buf[PAD + offset:PAD + offset + numel].view(b, size[0], size[1], c)
  assert out.data_ptr() % 16 == (4 * offset) % 16
  ops.resize_nhwc(torch.from_numpy(x).to(dev), size, mode, out=out)
  assert (buf[:PAD + offset] == CANARY).all() and (buf[PAD + offset + numel:] == CANARY).all()   # nothing outside
  assert torch.isfinite(out).all() and not (out == CANARY).any()                                 # everything inside
  return out.cpu().numpy()


def _gate(x, size, mode, scale=None):
  e32 = np.abs(H.resize32(x, size, mode).astype(np.float64) - H.resize64(x, size, mode)).max()
  return max(2 * e32, FLOOR * (np.abs(x).max() if scale is None else scale)), e32


# ---- 1. the kernel against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("c,src,dst,offset", CASES, ids=CASE_IDS)
def test_kernel_against_restatement(dev, c, src, dst, offset, mode):
  """Nearest and the identity size: the source bits.  Bilinear, bicubic: max(2 * e32, 2^-23 max|x|), e32 the float32
  emulation's error on the same inputs (printed)."""
  x = _x((B,) + src + (c,))
  got = _resize_padded(dev, x, dst, mode, offset)
  want = H.resize64(x, dst, mode)
  if mode == "nearest" or src == dst:
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.signbit(got.flat[0])
    return
  gate, e32 = _gate(x, dst, mode)
  err = np.abs(got.astype(np.float64) - want).max()
  print(f"{mode} c={c} {src}->{dst} offset={offset}: err {err:.3e}, emulation {e32:.3e}, gate {gate:.3e}")
  assert err <= gate, (err, gate)


@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("src,dst", [((5, 7), (16, 9)), ((16, 16), (32, 32)), ((16, 24), (8, 12))])
def test_both_paths_give_the_same_bits(dev, src, dst, mode):
  """c = 4: 16-byte accesses on aligned pointers, the element-wise path on an output (or an input) one float off."""
  x = _x((B,) + src + (4,), seed=3)
  quad = _resize_padded(dev, x, dst, mode, 0)
  elem = _resize_padded(dev, x, dst, mode, 1)
  assert np.array_equal(quad.view(np.uint32), elem.view(np.uint32))
  xin = torch.zeros(x.size + 1, device=dev)[1:].view(x.shape)
  xin.copy_(torch.from_numpy(x))
  assert xin.data_ptr() % 16 == 4
  elem_in = ops.resize_nhwc(xin, dst, mode).cpu().numpy()
  assert np.array_equal(quad.view(np.uint32), elem_in.view(np.uint32))
  again = _resize_padded(dev, x, dst, mode, 0)                      # deterministic
  assert np.array_equal(quad.view(np.uint32), again.view(np.uint32))


# ---- 2. exact probes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("c,src,dst,offset", [(4, (5, 7), (16, 9), 0), (4, (16, 24), (8, 12), 0), (4, (1, 1), (4, 4), 0),
                                              (3, (3, 5), (7, 4), 0), (4, (2, 2), (3, 3), 1)])
def test_one_hot_probes(dev, c, src, dst, offset, mode):
  """Image p of the batch is 1 at source pixel p and 0 elsewhere: the outputs that are not zero are the output pixels
  with a tap on p, and their sum is the total weight p receives -- every tap of every output pixel and both borders
  (where several clamped taps fall on one pixel) are counted."""
  n = src[0] * src[1]
  x = np.zeros((n,) + src + (c,), dtype=np.float32)
  x.reshape(n, n, c)[np.arange(n), np.arange(n)] = 1.
  got = _resize_padded(dev, x, dst, mode, offset)
  want = H.resize64(x, dst, mode)
  assert np.array_equal(got != 0, want != 0)
  if mode == "nearest":
    assert np.array_equal(got, want.astype(np.float32))
    return
  gate, e32 = _gate(x, dst, mode, scale=1.)
  sums, want_sums = got.astype(np.float64).sum(axis=(1, 2)), want.sum(axis=(1, 2))
  err = np.abs(sums - want_sums).max()
  terms = np.count_nonzero(want, axis=(1, 2)).max()
  print(f"probe {mode} c={c} {src}->{dst}: sums err {err:.3e} over up to {terms} outputs, per-output gate {gate:.3e}")
  assert np.abs(got.astype(np.float64) - want).max() <= gate
  assert err <= terms * gate
  assert np.abs(want_sums.sum(axis=0) - dst[0] * dst[1]).max() <= 1e-9     # (every output's weights sum to 1)


def test_bad_arguments(dev):
  x = torch.zeros(2, 4, 4, 4, device=dev)
  out = torch.zeros(2, 8, 8, 4, device=dev)
  with pytest.raises(LdmHipError, match="unknown mode"):
    ops.resize_nhwc(x, (8, 8), 3, out=out)
  with pytest.raises(LdmHipError, match="unknown mode"):
    ops.resize_nhwc(x, (8, 8), -1, out=out)
  for size in ((0, 8), (8, 0), (-1, 8)):
    with pytest.raises(LdmHipError, match="bad args"):
      ops.resize_nhwc(x, size, "bilinear", out=out)
  s = torch.cuda.current_stream().cuda_stream
  lib = _lib.lib
  for args in ((None, out.data_ptr(), 2, 4, 4, 4, 8, 8, 1, s), (x.data_ptr(), None, 2, 4, 4, 4, 8, 8, 1, s)):
    assert lib.ldm_resize_nhwc(*args) == _lib.ERR_ARG and "null pointer" in _lib.last_error()
  for bad in ((0, 4, 4, 4), (2, 0, 4, 4), (2, 4, 0, 4), (2, 4, 4, 0)):
    assert lib.ldm_resize_nhwc(x.data_ptr(), out.data_ptr(), *bad, 8, 8, 1, s) == _lib.ERR_ARG
  with pytest.raises(ValueError, match="resize mode"):
    ops.resize_nhwc(x, (8, 8), "area", out=out)
  torch.cuda.synchronize()
  assert (out == 0).all()


# ---- 3. the loop ------------------------------------------------------------------------------------------
def _sampler(dev, dtype, unet_w, txt_w, kl_w, use_graph=True, **kw):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  ldm = dict(LDM, **kw.pop("ldm", {}))
  unet = UNet(**T.UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=T.CTX_DIM)
  ae = AutoencoderKL(**T.KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**T.TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, **kw, **ldm)


def _inputs():
  g = np.random.default_rng(31)
  return dict(x_T=g.standard_normal(tuple(LO)).astype(np.float32),
              Q=g.standard_normal((N,) + tuple(HI)).astype(np.float32),
              img=(g.random((B, 256, 256, 3), dtype=np.float32) * 2 - 1).astype(np.float32),
              E=g.standard_normal(tuple(HI)).astype(np.float32))


_ORACLE = {}


def _oracle(w):
  """Computed once, shared, never written to: the two-pass loop (bilinear) and img2img at 32x32 latents, float32."""
  if not _ORACLE:
    t, ids = _inputs(), T._ids()
    _ORACLE["hires"] = H.hires_loop(O, ids, t["x_T"], w, LDM, K, HI[1:3], "bilinear", t["Q"], GS)
    ctx = O.text_encoder(ids, w["cond_stage_model"], torch.float32)
    _, _, sample = O.diagonal_gaussian(O.encoder_forward(torch.from_numpy(t["img"]), w["autoencoder"]), t["E"])
    x = H.sdedit_loop(O, ctx, np.float32(LDM["scale_factor"]) * sample, w, LDM, K, t["Q"], GS)
    _ORACLE["img2img"] = (O.decoder_forward(x / LDM["scale_factor"], w["autoencoder"]), x)
  return _ORACLE


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_loop_against_the_composed_oracle(dev, dtype, unet_w, txt_w, kl_w):
  """Gate: LOOP_MARGIN times the error of ddim_p_sample_loop_img2img against its oracle at 32x32 latents, same run."""
  ref = _oracle(dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w))
  t, ids = _inputs(), T._ids()
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  base_img = T.rel_err(s.ddim_p_sample_loop_img2img(ids, t["img"], GS, strength=STRENGTH, encode_noise=t["E"],
                                                    q_noises=t["Q"]), ref["img2img"][0])[0]
  base_lat = T.rel_err(s._xt, ref["img2img"][1])[0]
  got = s.ddim_p_sample_loop_hires(ids, LO, HI, strength=STRENGTH, resize="bilinear", guidance_scale=GS, x_T=t["x_T"],
                                   q_noises=t["Q"])
  images, first, z0, last = ref["hires"]
  assert tuple(got.shape) == (B, 256, 256, 3) and tuple(s._xt.shape) == tuple(HI)
  r_first, r_lat, r_img = (T.rel_err(a, b)[0] for a, b in ((s.hires_first_latents, first), (s._xt, last),
                                                           (got, images)))
  print(f"hires [{dtype}]: pass 1 {r_first:.3e}, latents {r_lat:.3e} (img2img@32 {base_lat:.3e}, gate "
        f"{LOOP_MARGIN * base_lat:.3e}), images {r_img:.3e} (img2img@32 {base_img:.3e}, gate "
        f"{LOOP_MARGIN * base_img:.3e})")
  assert r_lat <= LOOP_MARGIN * base_lat and r_img <= LOOP_MARGIN * base_img


def test_graph_eager_first_pass_and_recording(dev, unet_w, txt_w, kl_w):
  t, ids = _inputs(), T._ids()
  kw = dict(strength=STRENGTH, resize="bicubic", guidance_scale=GS, x_T=t["x_T"], q_noises=t["Q"])
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  got = s.ddim_p_sample_loop_hires(ids, LO, HI, **kw)
  lat, first = s._xt.clone(), s.hires_first_latents.clone()
  e = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  rec = []
  got_e = e.ddim_p_sample_loop_hires(ids, LO, HI, record=rec, **kw)
  assert e._graph is None and len(rec) == N + K
  assert [tuple(r.shape) for r in rec] == [tuple(LO)] * N + [tuple(HI)] * K
  assert torch.equal(e._xt, lat) and torch.equal(got_e, got)          # eager == graph replay
  assert torch.equal(rec[N - 1], first) and torch.equal(rec[-1], lat)
  # pass 1 is ddim_p_sample_loop, bit for bit
  p = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  p.ddim_p_sample_loop(ids, LO, GS, x_T=t["x_T"])
  assert torch.equal(p._xt, first)
  # pass 2 is the resize and the unmasked img2img loop from it
  z0 = ops.resize_nhwc(first, HI[1:3], "bicubic")
  assert torch.equal(p._sdedit(p._cond_stage_model(ids), z0, K, GS, None, None, t["Q"], None, 0, 0, None), got)
  assert s.last_hires_ms()[0] > 0 and s.last_hires_ms()[1] > 0


def test_two_shapes_keep_their_graphs(dev, unet_w, txt_w, kl_w):
  t, ids = _inputs(), T._ids()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  a = s.ddim_p_sample_loop_hires(ids, LO, HI, strength=STRENGTH, guidance_scale=GS, seed=3)
  g_hi, g_lo = s._graph, s._states[tuple(LO)]["_graph"]
  assert g_hi is not None and g_lo is not None and g_hi is not g_lo and s._state_key == tuple(HI)
  xt_hi, xt_lo = s._xt.data_ptr(), s._states[tuple(LO)]["_xt"].data_ptr()
  b_ = s.ddim_p_sample_loop_hires(ids, LO, HI, strength=STRENGTH, guidance_scale=GS, seed=4)
  assert s._graph is g_hi and s._states[tuple(LO)]["_graph"] is g_lo            # another seed: nothing captured
  assert s._xt.data_ptr() == xt_hi and s._states[tuple(LO)]["_xt"].data_ptr() == xt_lo
  assert not torch.equal(a, b_)
  assert torch.equal(a, s.ddim_p_sample_loop_hires(ids, LO, HI, strength=STRENGTH, guidance_scale=GS, seed=3))
  # a plain loop at the first shape replays the graph pass 1 captured, and computes what a fresh sampler does
  plain = s.ddim_p_sample_loop(ids, LO, GS, x_T=t["x_T"])
  assert s._graph is g_lo and s._state_key == tuple(LO) and s._states[tuple(HI)]["_graph"] is g_hi
  fresh = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  assert torch.equal(plain, fresh.ddim_p_sample_loop(ids, LO, GS, x_T=t["x_T"]))
  # ... and so does one at the second shape
  x_hi = np.random.default_rng(5).standard_normal(tuple(HI)).astype(np.float32)
  plain_hi = s.ddim_p_sample_loop(ids, HI, GS, x_T=x_hi)
  assert s._graph is g_hi
  assert torch.equal(plain_hi, fresh.ddim_p_sample_loop(ids, HI, GS, x_T=x_hi))
  s.release_shapes()
  assert not s._states and s._graph is g_hi


def test_device_noise_with_eta(dev, unet_w, txt_w, kl_w, monkeypatch):
  """noise_source="device", eta = 1: both passes draw inside their update launches; pass 2 under hires_seed(seed)."""
  from ldm_tf2_amd.model_runners import ETA_STREAM, Q_STREAM, hires_seed
  ids = T._ids()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, noise_source="device", ldm=dict(eta=1.))
  seeds = []
  set_rng = s._set_rng
  monkeypatch.setattr(s, "_set_rng", lambda seed, first: (seeds.append(int(seed)), set_rng(seed, first))[1])
  got = s.ddim_p_sample_loop_hires(ids, LO, HI, strength=STRENGTH, guidance_scale=GS, seed=11)
  lat = s._xt.clone()
  assert torch.isfinite(got).all() and tuple(got.shape) == (B, 256, 256, 3)
  assert set(seeds) == {11, hires_seed(11)} and seeds[-1] == hires_seed(11) and seeds[0] == 11
  assert not hasattr(s, "_noise_buf") and not hasattr(s, "_q_buf")            # no table was built
  again = s.ddim_p_sample_loop_hires(ids, LO, HI, strength=STRENGTH, guidance_scale=GS, seed=11)
  assert torch.equal(again, got)
  assert not torch.equal(s.ddim_p_sample_loop_hires(ids, LO, HI, strength=STRENGTH, guidance_scale=GS, seed=12), got)
  # pass 2 is the img2img loop under the derived seed, bit for bit
  p = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, noise_source="device", ldm=dict(eta=1.))
  p.ddim_p_sample_loop(ids, LO, GS, seed=11)
  z0 = ops.resize_nhwc(p._xt, HI[1:3], "bilinear")
  assert torch.equal(p._sdedit(p._cond_stage_model(ids), z0, K, GS, None, None, None, None, hires_seed(11), 0, None),
                     got)
  assert torch.equal(p._xt, lat)
  # the draws of the two passes at every index they share (eta noise of indices 0 .. K-1; Q of index K-1) differ
  a, b_ = torch.empty(tuple(HI), device=dev), torch.empty(tuple(HI), device=dev)
  for stream in [ETA_STREAM + i for i in range(K)] + [Q_STREAM + K - 1]:
    ops.normal_fill(a, set_rng(11, 0), stream)
    ops.normal_fill(b_, set_rng(hires_seed(11), 0), stream)
    same = (a == b_).float().mean().item()
    assert same < 1e-3, (stream, same)


def test_plms_runs_end_to_end(dev, unet_w, txt_w, kl_w):
  t, ids = _inputs(), T._ids()
  kw = dict(strength=STRENGTH, guidance_scale=GS, x_T=t["x_T"], q_noises=t["Q"])
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler="plms")
  got = s.ddim_p_sample_loop_hires(ids, LO, HI, **kw)
  assert torch.isfinite(got).all() and tuple(got.shape) == (B, 256, 256, 3)
  assert tuple(s._ring.shape) == (4,) + tuple(HI) and tuple(s._states[tuple(LO)]["_ring"].shape) == (4,) + tuple(LO)
  e = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler="plms", use_graph=False)
  assert torch.equal(e.ddim_p_sample_loop_hires(ids, LO, HI, **kw), got)
  assert torch.equal(s.ddim_p_sample_loop_hires(ids, LO, HI, **kw), got)
  d = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  assert not torch.equal(d.ddim_p_sample_loop_hires(ids, LO, HI, **kw), got)  # (the multistep solver is in use)
  # a guidance schedule runs in both passes too
  sched = s.ddim_p_sample_loop_hires(ids, LO, HI, guidance_interval=(200, 800), **kw)
  assert torch.isfinite(sched).all() and not torch.equal(sched, got)
