"""Cross-attention heat maps at model level: the launches UNet.capture_attention adds, checked
teacher-forced against tests/attn_map_ref.py and against the CPU oracle, and the txt2img / img2img loops with attn_maps.

The models, ids and LDM section are those of tests/test_zz_preview_gpu.py: B = 2, 16 x 16 latents, so the transformer
blocks see T = 256, 64, 16 and 4 queries.  The gate of the teacher-forced checks is the kernel tests' (delta = max(2 e32,
8 * 2^-24 w), tests/test_zz_attn_map_kernel_gpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_map_ref as A  # noqa: E402
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

UNET_CFG = dict(model_channels=64, out_channels=4, num_blocks=2, channel_mult=(1, 2, 4, 4), num_heads=8)
CTX_DIM = 128
TXT_CFG = dict(vocab_size=1000, encoder_stack_size=2, hidden_size=CTX_DIM, num_heads=4,
               size_per_head=32, max_seq_len=77, filter_size=256)
KL_CFG = dict(latent_channels=4, channels=64, num_blocks=2, multipliers=(1, 2, 4, 4))
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012, v_posterior=0., scale_factor=0.18215,
           eta=0., num_ddim_steps=10)
B, HW, N, TK = 2, 16, 10, 77
SHAPE = [B, HW, HW, 4]


@pytest.fixture(scope="module")
def unet_w():
  return Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **UNET_CFG), seed=2, mode="random", scope="unet")


@pytest.fixture(scope="module")
def txt_w():
  return Wt.init_weights(Wt.transformer_manifest(**TXT_CFG), seed=2, mode="random", scope="cond_stage_model")


@pytest.fixture(scope="module")
def kl_w():
  m = Wt.decoder_manifest(**KL_CFG)
  m.update(Wt.encoder_manifest(**KL_CFG, image_size=8 * HW, double_z=True))
  return Wt.init_weights(m, seed=2, mode="random", scope="autoencoder")


def _unet(dev, unet_w, dtype=torch.float32, **kw):
  from ldm_tf2_amd.unet import UNet
  return UNet(**UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=CTX_DIM, **kw)


def _sampler(dev, unet_w, txt_w, kl_w, use_graph=True, **kw):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  return LatentDiffusionModelSampler(_unet(dev, unet_w), AutoencoderKL(**KL_CFG, weights=kl_w, device=dev),
                                     TransformerModel(**TXT_CFG, weights=txt_w, device=dev), use_graph=use_graph,
                                     verbose=False, **dict(LDM, **kw))


def _ids():
  g = np.random.default_rng(1)
  cond = g.integers(0, 1000, size=(1, 77))
  uncond = np.array([[101, 102] + [0] * 75])
  return np.concatenate([np.tile(uncond, (B, 1)), np.tile(cond, (B, 1))], 0)


def _img_inputs():
  g = np.random.default_rng(21)
  img = (g.random((B, 8 * HW, 8 * HW, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
  E = g.standard_normal((B, HW, HW, 4), dtype=np.float32)
  mask = np.zeros((B, HW, HW), np.float32)
  mask[:, :, : HW // 2] = 1.
  return img, E, mask


def _x_ctx(R=2 * B, hw=HW, tk=TK, seed=0):
  g = np.random.default_rng(seed)
  return (g.standard_normal((R, hw, hw, 4)).astype(np.float32), g.standard_normal((R, tk, CTX_DIM)).astype(np.float32))


# ---- teacher-forced: every launch against the restatement of its own inputs ------------------------------
class _Recorder:
  """Stands in for ops.xattn_map: clones the inputs, calls the kernel, clones the result."""

  def __init__(self, fn):
    self.fn, self.calls = fn, []

  def __call__(self, q, k, acc, heads, s, sp, log2_scale, step_w=None, index=None, index_bias=0):
    rec = dict(q=q.float().cpu().numpy(), k=k.float().cpu().numpy(), before=acc.clone(), heads=heads, s=s, sp=sp,
               ls=log2_scale, rows=q.shape[0], q_offset=q.storage_offset(), k_offset=k.storage_offset(), acc=acc,
               step_w=step_w, index=index, index_bias=index_bias)
    out = self.fn(q, k, acc, heads, s, sp, log2_scale, step_w=step_w, index=index, index_bias=index_bias)
    rec["after"] = acc.clone()
    self.calls.append(rec)
    return out


def _teacher_forced(unet, calls, layers, rows, what):
  r0, r1 = rows
  assert len(calls) == len(layers), (len(calls), layers)
  accs = unet.attention_layers()
  assert [n for n, _, _, _ in accs] == list(layers)
  for c, (n, h, w, acc) in zip(calls, accs):
    st = unet.sts[n]
    assert (c["heads"], c["s"], c["sp"]) == (st.heads, st.s, st.sp) and c["acc"] is acc
    assert c["rows"] == r1 - r0 and tuple(acc.shape) == (r1 - r0, h, w, TK)
    assert c["q"].shape == (r1 - r0, h * w, st.heads * st.sp)
    # the conditional rows only: the slices start r0 rows into the query and key tensors
    assert c["q_offset"] == r0 * h * w * st.heads * st.sp and c["k_offset"] == r0 * TK * st.heads * st.sp
    before = c["before"].cpu().numpy().reshape(r1 - r0, h * w, TK)
    got = c["after"].cpu().numpy().reshape(r1 - r0, h * w, TK)
    want, e32, delta = A.gate(c["q"], c["k"], st.heads, st.s, st.sp, c["ls"], 1., before)
    err = float(np.abs(got - want).max())
    print(f"{what} layer {n} T={h * w} S={st.s} log2_scale={c['ls']:.4f}: e32={e32:.3e} delta={delta:.3e} max err={err:.3e}")
    assert err <= delta, f"{what} layer {n}: {err:.3e} above {delta:.3e}"
    assert np.abs(got.sum(-1) - before.sum(-1) - 1.).max() <= 1e-5


class _CountingLib:
  def __init__(self, lib):
    self._lib, self.calls = lib, []

  def __getattr__(self, name):
    fn = getattr(self._lib, name)

    def call(*args):
      self.calls.append(name)
      return fn(*args)
    return call


def _launches(monkeypatch, fn):
  proxy = _CountingLib(ops.lib)
  monkeypatch.setattr(ops, "lib", proxy)
  try:
    out = fn()
  finally:
    monkeypatch.setattr(ops, "lib", proxy._lib)
  torch.cuda.synchronize()
  return out, proxy.calls


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layers", [None, [1, 7, 12]])
def test_capture_teacher_forced(dev, unet_w, monkeypatch, dtype, layers):
  unet = _unet(dev, unet_w, dtype)
  assert len(unet.sts) == 16
  x, ctx = _x_ctx()
  xd = torch.from_numpy(x).to(dev)
  t = torch.full((2 * B,), 500, dtype=torch.int32, device=dev)
  unet.set_context(torch.from_numpy(ctx).to(dev))
  rec = _Recorder(ops.xattn_map)
  monkeypatch.setattr(ops, "xattn_map", rec)
  # off (the default): no call, and the launch list of a forward
  off, off_calls = _launches(monkeypatch, lambda: unet.forward(xd, t_rows=t, shared_t=True).clone())
  assert rec.calls == [] and unet.attention_layers() == [] and "ldm_xattn_map" not in off_calls
  unet.capture_attention(rows=(B, 2 * B), layers=layers)
  on, on_calls = _launches(monkeypatch, lambda: unet.forward(xd, t_rows=t, shared_t=True).clone())
  sel = list(range(16)) if layers is None else layers
  assert torch.equal(on, off)                                # (these configurations never take ldm_st_block)
  assert on_calls.count("ldm_xattn_map") == len(sel) and [c for c in on_calls if c != "ldm_xattn_map"] == off_calls
  _teacher_forced(unet, rec.calls, sel, (B, 2 * B), f"{dtype}")
  assert sorted({(h, w) for _, h, w, _ in unet.attention_layers()}, reverse=True)[0] == (HW, HW)
  if layers is None:
    assert {h * w for _, h, w, _ in unet.attention_layers()} == {256, 64, 16, 4}
  # a second evaluation accumulates; reset zeroes; off again leaves the launch list as it was
  rec.calls.clear()
  unet.forward(xd, t_rows=t, shared_t=True)
  _teacher_forced(unet, rec.calls, sel, (B, 2 * B), f"{dtype} second")
  for _, _, _, acc in unet.attention_layers():
    assert abs(float(acc.sum()) / (B * acc.shape[1] * acc.shape[2]) - 2.) <= 1e-4
  accs = unet.attention_layers()
  unet.reset_attention_maps()
  assert all(float(acc.abs().max()) == 0. for _, _, _, acc in accs)
  unet.capture_attention(None)
  rec.calls.clear()
  _, again = _launches(monkeypatch, lambda: unet.forward(xd, t_rows=t, shared_t=True))
  assert again == off_calls and rec.calls == []


def test_capture_errors(dev, unet_w):
  unet = _unet(dev, unet_w)
  x, ctx = _x_ctx(tk=88)
  with pytest.raises(ValueError, match="layers"):
    unet.capture_attention(rows=(B, 2 * B), layers=[16])
  with pytest.raises(ValueError, match="rows"):
    unet.capture_attention(rows=(2, 2))
  unet.set_context(torch.from_numpy(ctx).to(dev))
  with pytest.raises(ValueError, match="80 tokens"):          # Tk > 80
    unet.capture_attention(rows=(B, 2 * B))
  assert unet.attention_layers() == []
  x, ctx = _x_ctx()
  unet.set_context(torch.from_numpy(ctx).to(dev))
  unet.capture_attention(rows=(B, 2 * B))
  with pytest.raises(ValueError, match="80 tokens"):          # ... also when the longer context comes second
    unet.set_context(torch.from_numpy(_x_ctx(tk=88)[1]).to(dev))
  unet.set_context(torch.from_numpy(ctx).to(dev))
  xd = torch.from_numpy(x).to(dev)
  t = torch.full((B,), 500, dtype=torch.int32, device=dev)
  with pytest.raises(ValueError, match="context_rows"):
    unet.forward(xd[B:].contiguous(), t_rows=t, shared_t=True, context_rows=(B, 2 * B))


# ---- against the oracle (float32; bf16 is covered by the teacher-forced test above) ------------------------
def _oracle_maps(x, t, ctx, unet_w, dtype):
  """The head-averaged cross-attention probabilities [R,T,Tk] of every transformer block of one oracle evaluation,
  in call order, recorded by a wrapper around oracle.ldm_oracle.multihead_attention."""
  maps, orig = [], O.multihead_attention

  def wrapped(query, context, w, scale_dim):
    if query is not context:                                   # (self-attention passes the same tensor twice)
      q = O.projection_split(query, w("query/kernel"))
      k = O.projection_split(context, w("key/kernel"))
      logits = torch.einsum("nqhs,nchs->nhqc", q, k) * (q.shape[-1] ** -0.5)
      maps.append(torch.softmax(logits, dim=3).mean(1).double().numpy())
    return orig(query, context, w, scale_dim)

  O.multihead_attention = wrapped
  try:
    O.unet_forward(x, t, ctx, unet_w, dtype=dtype)
  finally:
    O.multihead_attention = orig
  return maps


def test_maps_against_oracle(dev, unet_w):
  """One U-Net evaluation, float32, all rows: per layer the rel-L2 distance of the maps to the oracle's float64 maps
  stays below 12 times the oracle's own float32-vs-float64 drift of the same maps -- the factor tests/test_models_gpu.py
  documents for one U-Net evaluation (everything upstream of q differs by summation order)."""
  x, ctx = _x_ctx()
  t = np.array([981, 981, 21, 500], dtype=np.int32)
  m64 = _oracle_maps(x, t, ctx, unet_w, torch.float64)
  m32 = _oracle_maps(x, t, ctx, unet_w, torch.float32)
  assert len(m64) == len(m32) == 16
  unet = _unet(dev, unet_w)
  unet.set_context(torch.from_numpy(ctx).to(dev))
  unet.capture_attention(rows=(0, 2 * B))
  unet.forward(torch.from_numpy(x).to(dev), t_rows=torch.from_numpy(t).to(dev))
  rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
  bad = []
  for (n, h, w, acc), a64, a32 in zip(unet.attention_layers(), m64, m32):
    got = acc.cpu().numpy().reshape(2 * B, h * w, TK).astype(np.float64)
    drift, ours = rel(a32, a64), rel(got, a64)
    print(f"layer {n} T={h * w}: oracle f32-vs-f64 drift {drift:.3e}, ours {ours:.3e} ({ours / drift:.2f}x)")
    if not ours < 12. * drift:
      bad.append((n, ours, drift))
  assert not bad, bad


# ---- the loops ---------------------------------------------------------------------------------------------
def _call(s, kind, ids, **kw):
  if kind == "img2img":
    img, E, mask = _img_inputs()
    images = s.ddim_p_sample_loop_img2img(ids, img, 5., strength=0.5, mask=mask, encode_noise=E, seed=3, **kw)
  else:
    images = s.ddim_p_sample_loop(ids, SHAPE, 5., seed=3, **kw)
  return images.clone(), s._xt.clone()


@pytest.mark.parametrize("kind", ["txt2img", "img2img"])
def test_loop_maps(dev, unet_w, txt_w, kl_w, kind):
  ids = _ids()
  k = 5 if kind == "img2img" else N
  s = _sampler(dev, unet_w, txt_w, kl_w)
  with pytest.raises(ValueError, match="no loop has run"):
    s.last_attention_maps()
  plain_images, plain_latents = _call(s, kind, ids)
  g_plain, key_plain = s._graph, s._graph_key
  assert g_plain is not None and s._am_graph is None
  images, latents = _call(s, kind, ids, attn_maps=True)
  assert torch.equal(images, plain_images) and torch.equal(latents, plain_latents)
  assert s._graph is g_plain and s._graph_key == key_plain and s._am_graph is not None
  assert s._am_graph_key[:-1] == key_plain and s._am_graph_key[-1] == ("attn", tuple(range(16)))
  assert s._unet._attn_cap is None                              # capture is off again after the loop
  m = s.last_attention_maps(raw=True)
  heat = m["heat"]
  assert heat.dtype == np.float32 and heat.shape == (B, TK, HW, HW) and m["layers"] == list(range(16))
  assert m["weight_sum"] == float(k)                            # img2img: the k indices run, not N
  assert np.abs(heat.sum(1) - 1.).max() <= 1e-5 and heat.min() >= 0.
  assert len(m["raw"]) == 16 and all(a.shape[0] == B and a.shape[3] == TK for a in m["raw"])
  assert {a.shape[1] * a.shape[2] for a in m["raw"]} == {256, 64, 16, 4}
  for a in m["raw"]:
    assert np.abs(a.sum(-1) - k).max() <= 1e-4
  # another size, a subset of the layers
  big = s.last_attention_maps(size=(40, 24), layers=[0, 15], mode="bilinear")
  assert big["heat"].shape == (B, TK, 40, 24) and big["layers"] == [0, 15]
  assert np.abs(big["heat"].sum(1) - 1.).max() <= 1e-5
  with pytest.raises(ValueError, match="layers"):
    s.last_attention_maps(layers=[16])
  # replayed a second time: the same accumulators (reset zeroes them outside the graph), no new capture
  g_am = s._am_graph
  _call(s, kind, ids, attn_maps=True)
  again = s.last_attention_maps(raw=True)
  assert s._am_graph is g_am and all(np.array_equal(a, b) for a, b in zip(again["raw"], m["raw"]))
  # without the keyword afterwards: the first images bit for bit, from the graph it had
  after_images, _ = _call(s, kind, ids)
  assert s._graph is g_plain and s._am_graph is g_am and torch.equal(after_images, plain_images)
  # an eager run: bit-identical accumulators
  e = _sampler(dev, unet_w, txt_w, kl_w, use_graph=False)
  e_images, _ = _call(e, kind, ids, attn_maps=True)
  em = e.last_attention_maps(raw=True)
  assert torch.equal(e_images, images) and e._am_graph is None
  assert all(np.array_equal(a, b) for a, b in zip(em["raw"], m["raw"])) and np.array_equal(em["heat"], heat)
  # a subset of layers has a graph key of its own
  _call(s, kind, ids, attn_maps=True, attn_layers=[3, 0])
  sub = s.last_attention_maps(raw=True)
  assert sub["layers"] == [0, 3] and s._am_graph_key[-1] == ("attn", (0, 3))
  assert np.array_equal(sub["raw"][0], m["raw"][0]) and np.array_equal(sub["raw"][1], m["raw"][3])


@pytest.mark.parametrize("opts", [dict(temb_table=True), dict(temb_table=False), dict(sampler="plms")],
                         ids=["temb_table", "no_temb_table", "plms"])
def test_one_hot_step_table(dev, unet_w, txt_w, kl_w, opts):
  """Weights 1 at DDIM index i and 0 elsewhere: the loop's accumulators equal, bit for bit, those of a single
  evaluation at index i on the latents the same trajectory (an eager run with record=) has before that step -- which
  pins the counter's position inside the U-Net (index_bias) for both places the counter can move."""
  ids = _ids()
  x_T = np.random.default_rng(8).standard_normal(SHAPE).astype(np.float32)
  e = _sampler(dev, unet_w, txt_w, kl_w, use_graph=False, **opts)
  rec = []
  e.ddim_p_sample_loop(ids, SHAPE, 5., x_T=x_T, record=rec)
  assert len(rec) == N
  context = e._cond_stage_model(ids)
  s = _sampler(dev, unet_w, txt_w, kl_w, **opts)
  assert s._loop_start_index(N) == (N if opts.get("temb_table", True) else N - 1)
  for i in (0, 4, N - 1):
    w = [0.] * N
    w[i] = 1.
    s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=x_T, attn_maps=w)
    m = s.last_attention_maps(raw=True)
    assert m["weight_sum"] == 1.
    before = torch.from_numpy(x_T).to(dev) if i == N - 1 else rec[N - 2 - i]
    e._unet.capture_attention(rows=(B, 2 * B))
    e._unet.reset_attention_maps()
    try:
      e.ddim_sample(before, context, i, guidance_scale=5.)
      single = [acc.cpu().numpy() for _, _, _, acc in e._unet.attention_layers()]
    finally:
      e._unet.capture_attention(None)
    assert len(single) == 16
    for n, (a, b) in enumerate(zip(m["raw"], single)):
      assert np.array_equal(a, b), f"index {i} layer {n}: {np.abs(a - b).max():.3e}"
    assert np.abs(m["heat"].sum(1) - 1.).max() <= 1e-5


def test_forbidden_combinations(dev, unet_w, txt_w, kl_w):
  s = _sampler(dev, unet_w, txt_w, kl_w)
  ids = _ids()
  img, E, mask = _img_inputs()
  s.set_preview((0.3 * np.random.default_rng(17).standard_normal((5, 3))).astype(np.float32), scale=2)
  for kw, what in ((dict(guidance_interval=(300, 700)), "guidance schedule"), (dict(preview_freq=3), "preview_freq"),
                   (dict(record=[]), "record=")):
    with pytest.raises(ValueError, match=f"attn_maps and .*{what}"):
      s.ddim_p_sample_loop(ids, SHAPE, 5., attn_maps=True, **kw)
    with pytest.raises(ValueError, match=f"attn_maps and .*{what}"):
      s.ddim_p_sample_loop_img2img(ids, img, 5., attn_maps=True, **kw)
  with pytest.raises(ValueError, match="attn_maps and .*guidance schedule"):
    s.ddim_p_sample_loop(ids, SHAPE, [5.] * N, attn_maps=True)
  with pytest.raises(ValueError, match="attn_layers needs attn_maps"):
    s.ddim_p_sample_loop(ids, SHAPE, 5., attn_layers=[0])
  with pytest.raises(ValueError, match="attn_layers"):
    s.ddim_p_sample_loop(ids, SHAPE, 5., attn_maps=True, attn_layers=[0, 0])
  with pytest.raises(ValueError, match="attn_maps"):
    s.ddim_p_sample_loop(ids, SHAPE, 5., attn_maps=[1.] * (N - 1))
  with pytest.raises(ValueError, match="attn_maps and the panorama loop"):
    s.ddim_p_sample_loop_panorama(ids, [B, HW, 2 * HW, 4], (HW, HW), attn_maps=True)
  with pytest.raises(ValueError, match="attn_maps and the hires loop"):
    s.ddim_p_sample_loop_hires(ids, SHAPE, [B, 2 * HW, 2 * HW, 4], attn_maps=True)
  with pytest.raises(ValueError, match="attn_maps and the inversion loop"):
    s.ddim_invert_loop(ids, init_images=img, attn_maps=True)
  with pytest.raises(ValueError, match="attn_maps and the edit loop"):
    s.ddim_p_sample_loop_edit(ids, ids, img, attn_maps=True)
  with pytest.raises(ValueError, match="attn_maps and the progressive sampler"):
    s.ddim_p_sample_loop_progressive(ids, SHAPE, attn_maps=True)
  assert s._unet._attn_cap is None and s._am_graph is None and s._am_last is None


# ---- the ldm_st_block form ---------------------------------------------------------------------------------
BLK_CFG = dict(model_channels=320, out_channels=4, num_blocks=1, channel_mult=(1,), num_heads=8)


def test_capture_turns_st_block_off(dev, monkeypatch):
  """The smallest bf16 U-Net whose blocks take ldm_st_block (C = 320, heads of 40, T = 256 a multiple of 128, the row
  thresholds lowered): capture leaves that form, the output equals the U-Net built with fused_block=False bit for bit,
  and the launches' increments pass the teacher-forced check on the matrix-softmax layout (log2_scale = 1)."""
  from ldm_tf2_amd.unet import UNet
  w = Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **BLK_CFG), seed=2, mode="random", scope="unet")
  kw = dict(weights=w, dtype=torch.bfloat16, device=dev, context_dim=CTX_DIM, fold_min_rows=512, block_min_rows=512)
  fused, plain = UNet(**BLK_CFG, **kw), UNet(**BLK_CFG, fused_block=False, **kw)
  x, ctx = _x_ctx(R=B)
  xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(ctx).to(dev)
  t = torch.full((B,), 500, dtype=torch.int32, device=dev)
  calls = []
  orig = ops.st_block
  monkeypatch.setattr(ops, "st_block", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
  n_st = len(fused.sts)
  for u in (fused, plain):
    u.set_context(cd)
  out_fused = fused.forward(xd, t_rows=t, shared_t=True).clone()
  assert len(calls) == n_st and n_st >= 1                      # capture off: every block takes ldm_st_block
  out_plain = plain.forward(xd, t_rows=t, shared_t=True).clone()
  assert len(calls) == n_st
  rec = _Recorder(ops.xattn_map)
  monkeypatch.setattr(ops, "xattn_map", rec)
  fused.capture_attention(rows=(1, 2))
  out_cap = fused.forward(xd, t_rows=t, shared_t=True).clone()
  assert len(calls) == n_st and len(rec.calls) == n_st         # no ldm_st_block launch with capture on
  assert torch.equal(out_cap, out_plain)
  assert all(c["ls"] == 1.0 for c in rec.calls) and all(fused.sts[n].ms for n in range(n_st))
  _teacher_forced(fused, rec.calls, list(range(n_st)), (1, 2), "st_block form")
  # a subset: the other blocks keep ldm_st_block
  fused.capture_attention(rows=(1, 2), layers=[0])
  fused.forward(xd, t_rows=t, shared_t=True)
  assert len(calls) == 2 * n_st - 1
  fused.capture_attention(None)
  assert torch.equal(fused.forward(xd, t_rows=t, shared_t=True), out_fused) and len(calls) == 3 * n_st - 1


# ---- CLI -----------------------------------------------------------------------------------------------
def test_cli_writes_attention_maps(dev, tmp_path):
  import json
  import yaml
  from ldm_tf2_amd import run_ldm_sampler as R
  from ldm_tf2_amd.model_runners import word_heatmaps
  unet = dict(model_channels=64, out_channels=4, num_blocks=2, attention_resolutions=[4, 2, 1], dropout_rate=0.1,
              channel_mult=[1, 2, 4, 4], num_heads=8)
  txt = dict(vocab_size=200, encoder_stack_size=2, hidden_size=128, num_heads=4, size_per_head=32,
             max_seq_len=77, filter_size=256, dropout_rate=0.1)
  kl = dict(latent_channels=4, channels=64, num_blocks=2, attention_resolutions=[], dropout_rate=0.,
            multipliers=[1, 2, 4, 4], resample_with_conv=True)
  words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "painting", "of", "virus", "monster", "play", "##ing", "guitar"]
  words += [f"tok{i}" for i in range(200 - len(words))]
  (tmp_path / "vocab.txt").write_text("\n".join(words) + "\n", encoding="utf-8")
  samp = {"autoencoder_type": "kl", "latent_shape": [2, 16, 16, 4], "guidance_scale": 5.0,
          "text_prompt": "a painting of a virus monster playing guitar", "vocab_dir": str(tmp_path),
          "sample_save_progress": False}
  cfg = {"ldm_sampling": samp, "pre_ckpt_paths": {"cond_stage_model": None, "unet": None, "autoencoder": None},
         "cond_stage_model": txt, "autoencoder_kl": kl, "unet": unet, "ldm": LDM}

  def run(name, **keys):
    out = tmp_path / name
    out.mkdir()
    path = out / "config.yaml"
    path.write_text(yaml.safe_dump(dict(cfg, ldm_sampling=dict(samp, **keys))))
    R.main(["--config_path", str(path), "--dtype", "f32", "--seed", "7", "--out", str(out / "images.npy")])
    return out

  plain = run("plain")
  assert not (plain / "attention_maps.npy").exists() and not (plain / "attention_words.json").exists()
  on = run("on", attention_maps=True, attention_map_steps=[2, 6], attention_map_size=[32, 24])
  assert np.array_equal(np.load(on / "images.npy"), np.load(plain / "images.npy"))
  heat = np.load(on / "attention_maps.npy")
  assert heat.dtype == np.float32 and heat.shape == (2, 77, 32, 24) and np.abs(heat.sum(1) - 1.).max() <= 1e-5
  spans = json.load(open(on / "attention_words.json"))
  assert [s["word"] for s in spans] == ["a", "painting", "of", "a", "virus", "monster", "playing", "guitar"]
  assert [s["positions"] for s in spans] == [[1], [2], [3], [4], [5], [6], [7, 8], [9]]
  wh = word_heatmaps(heat, [(s["word"], s["positions"]) for s in spans])
  assert wh.shape == (2, 8, 32, 24) and np.array_equal(wh[:, 6], heat[:, 7] + heat[:, 8])
