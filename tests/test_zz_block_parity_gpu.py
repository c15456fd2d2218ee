"""Every U-Net and autoencoder stage on the HIP path against float64, stage by stage.

One evaluation per launch form with `taps`, then for every stage the figure of tests/block_ref.py: the GPU stage's
error against the float64 reference of THAT stage on the GPU's own input taps, in units of what the oracle loses on
the same stage in the same storage type.  Gates: block_ref.GATES, per stage kind and storage type.

Latents are 16x16 with R = 4 as a 2+2 CFG pair, the smallest size at which C = 320 has T = 256 (the row-panel forms
need T % 128 == 0) and C = 640 has T = 64 (the LayerNorm fold needs T % 32 == 0).  Model A (C = 320 and 640) runs
every launch form of `UNet._st`, the ResBlocks and the up convolutions; model B (four levels, blocks without
attention, T down to 4) the non-fold paths.  Each form proves through the call recorder that the entry point it is
named for was, or was no longer, called, that the evaluation with taps makes the calls of the one without (plus
copies), and that its output has the same bits.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import block_ref as BR  # noqa: E402
from ldm_tf2_amd import ops  # noqa: E402

from test_img2img_gpu import _CountingLib  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
SMALL = dict(ffn_min_rows=1, fold_min_rows=1, block_min_rows=1)
PANEL = ("ldm_st_block", "ldm_st_xtail", "ldm_st_tail", "ldm_ffn_geglu")
N_ST_A, N_SHORTCUT_A = 4, 5      # model A: transformer blocks; ResBlocks with a shortcut (320->640 and the 4 output blocks)


def _fewer_layernorms(calls, base):
  """LayerNorms come out of the producing GEMM's epilogue where its tile holds whole rows (C = 320): fewer launches
  than the three per block of the separate form."""
  assert calls.count("ldm_layernorm") < 3 * N_ST_A, calls.count("ldm_layernorm")


def _gemms(delta):
  """check(calls, default calls): the form launches `delta` more ldm_gemm than the default form."""
  def chk(calls, base):
    assert calls.count("ldm_gemm") == base.count("ldm_gemm") + delta, (calls.count("ldm_gemm"), base.count("ldm_gemm"))
  return chk


# name -> (constructor kwargs on top of SMALL, entry points that must / must not be called, extra check)
FORMS_BF16 = {
    "default": ({}, ("ldm_st_block", "ldm_attention_ms", "ldm_groupnorm_splitk", "ldm_groupnorm_fused"),
                ("ldm_st_xtail", "ldm_st_tail", "ldm_ffn_geglu", "ldm_layernorm"), None),
    "xtail": (dict(fused_block=False), ("ldm_st_xtail",), ("ldm_st_block", "ldm_st_tail", "ldm_ffn_geglu"), None),
    "tail": (dict(fused_block=False, fused_xattn=False), ("ldm_st_tail",),
             ("ldm_st_block", "ldm_st_xtail", "ldm_ffn_geglu"), None),
    "ffn": (dict(fused_block=False, fused_xattn=False, fused_tail=False), ("ldm_ffn_geglu",),
            ("ldm_st_block", "ldm_st_xtail", "ldm_st_tail"), None),
    "merged-ffproj": (dict(fused_ffn=False), ("ldm_attention_ms",), PANEL, None),
    # ... FF-out and proj_out as two launches: one more ldm_gemm per block than the merged form (checked against it)
    "split-ffproj": (dict(fused_ffn=False, merge_ffproj=False), ("ldm_attention_ms",), PANEL, "merged-ffproj"),
    "no-matrix-softmax": (dict(matrix_softmax=False), ("ldm_attention",), ("ldm_attention_ms", "ldm_st_block"), None),
    "split-qkv": (dict(merge_qkv=False), ("ldm_st_block",), (), _gemms(N_ST_A)),
    "no-fold": (dict(fold_layernorm=False), ("ldm_layernorm",), ("ldm_attention_ms",) + PANEL, None),
    "fuse-layernorm": (dict(fuse_layernorm=True), ("ldm_gemm_ln_supported",), ("ldm_attention_ms",) + PANEL,
                       _fewer_layernorms),
    "no-defer": (dict(defer_reduce=False), ("ldm_st_block",), ("ldm_groupnorm_splitk",), None),
    "gn-two-launch": (dict(gn_single_launch=False), ("ldm_groupnorm_partial", "ldm_groupnorm_apply"),
                      ("ldm_groupnorm_fused",), None),
    "two-launch-shortcut": (dict(merge_shortcut=False), ("ldm_st_block",), (), _gemms(N_SHORTCUT_A)),
    "gather-upsample": (dict(phase_upsample=False), ("ldm_st_block",), (), "conv3x3_up2"),
}
FORMS_F32 = {
    "default": ({}, ("ldm_layernorm", "ldm_attention"), ("ldm_attention_ms",) + PANEL, None),
    "fuse-layernorm": (dict(fuse_layernorm=True), ("ldm_gemm_ln_supported",), ("ldm_attention_ms",) + PANEL,
                       _fewer_layernorms),
    "two-launch-shortcut": (dict(merge_shortcut=False), (), ("ldm_attention_ms",) + PANEL, _gemms(N_SHORTCUT_A)),
}
# name -> {C: (norm, qkv, ms, rest)}: the StForm (ldm_tf2_amd/st_form.py) each of model A's blocks must pick at these
# shapes -- C = 320 at T = 256 (40-wide heads), C = 640 at T = 64 (no ldm_ffn_geglu weights: the per-layer rest)
_D320, _D640 = ("fold", "qkv_fold", True, "block"), ("fold", "qkv_fold", False, "ffproj")
PICKED_BF16 = {
    "default": {320: _D320, 640: _D640},
    "xtail": {320: _D320[:3] + ("xtail",), 640: _D640},
    "tail": {320: _D320[:3] + ("tail",), 640: _D640},
    "ffn": {320: _D320[:3] + ("ffn",), 640: _D640},
    "merged-ffproj": {320: _D320[:3] + ("ffproj",), 640: _D640},
    "split-ffproj": {320: _D320[:3] + ("layers",), 640: _D640[:3] + ("layers",)},
    "no-matrix-softmax": {320: ("fold", "qkv_fold", False, "tail"), 640: _D640},
    "split-qkv": {320: ("fold", "qk_v_fold", True, "block"), 640: ("fold", "qk_v_fold", False, "ffproj")},
    "no-fold": {320: ("separate", "qk_vt", False, "layers"), 640: ("separate", "qk_vt", False, "layers")},
    "fuse-layernorm": {320: ("epilogue", "qk_vt", False, "layers"), 640: ("separate", "qk_vt", False, "layers")},
    "no-defer": {320: _D320, 640: _D640}, "gn-two-launch": {320: _D320, 640: _D640},
    "two-launch-shortcut": {320: _D320, 640: _D640}, "gather-upsample": {320: _D320, 640: _D640},
}
_F32 = ("separate", "qkv_out2", False, "layers")
PICKED_F32 = {"default": {320: _F32, 640: _F32}, "fuse-layernorm": {320: ("epilogue",) + _F32[1:], 640: _F32},
              "two-launch-shortcut": {320: _F32, 640: _F32}}
CASES = [("A", BF16, n, "plain") for n in FORMS_BF16]
CASES += [("A", BF16, n, "paired") for n in ("default", "xtail", "tail", "ffn")]
CASES += [("A", BF16, "default", "context_rows")]
CASES += [("A", F32, n, "plain") for n in FORMS_F32] + [("A", F32, "default", "paired")]
CASES += [("B", F32, "default", "plain"), ("B", BF16, "default", "plain")]

_BASE = {}      # (model, dtype, call form) -> the calls of the default form; (.., name) -> those of a named form


def _record(monkeypatch, fn):
  proxy = _CountingLib(ops.lib)
  monkeypatch.setattr(ops, "lib", proxy)
  up2, n_up2 = ops.conv3x3_up2, []
  monkeypatch.setattr(ops, "conv3x3_up2", lambda *a, **k: (n_up2.append(1), up2(*a, **k))[1])
  try:
    fn()
  finally:
    monkeypatch.setattr(ops, "lib", proxy._lib)
    monkeypatch.setattr(ops, "conv3x3_up2", up2)
  torch.cuda.synchronize()
  return proxy.calls, len(n_up2)


def _launches(calls):
  return [c for c in calls if c != "ldm_cast"]


def _evaluate(dev, monkeypatch, model, dtype, kw, form):
  """(calls, number of phase-upsample launches, taps, env, [(block's C, st index, picked StForm)]): one model build,
  the evaluation without and with taps."""
  from ldm_tf2_amd.unet import UNet
  c = BR.unet_case(model)
  env = c["env"]
  x, t, ctx = env["x"].to(dev), torch.from_numpy(env["t"]).to(dev), env["ctx"].to(dev)
  u = UNet(**c["cfg"], context_dim=BR.CTX_DIM, weights=c["weights"], dtype=dtype, device=dev, **kw)
  u.set_context(ctx)
  fkw = dict(t_rows=t)
  if form == "paired":
    fkw["paired_rows"] = True
  elif form == "context_rows":
    x, fkw, env = x[2:].contiguous(), dict(t_rows=t[2:].contiguous(), context_rows=(2, 4)), BR.sub_env(env, (2, 4))
  out = torch.empty(x.shape[0], 16, 16, 4, device=dev)
  u.forward(x, out=out, **fkw)                      # the first evaluation allocates the model's scratch
  calls, n_up2 = _record(monkeypatch, lambda: u.forward(x, out=out, **fkw))
  plain = out.clone()
  taps = {}
  out.zero_()
  calls_t, _ = _record(monkeypatch, lambda: u.forward(x, out=out, taps=taps, **fkw))
  assert _launches(calls_t) == _launches(calls), "the evaluation with taps makes other calls than the one without"
  assert calls_t.count("ldm_cast") == calls.count("ldm_cast"), "taps are torch clones: no launch of the library"
  assert torch.equal(out, plain), "the evaluation with taps gives other bits than the one without"
  assert torch.equal(taps["out"], plain) and list(taps) and set(taps) == {s.name for s in c["stages"]}
  # eager only: refused, before any launch, while the stream is capturing
  monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
  with pytest.raises(ValueError):
    u.forward(x, out=out, taps={}, **fkw)
  monkeypatch.undo()
  assert [i for i, _ in u.forms()] == list(range(len(u.sts))), "every transformer block records the form it took"
  return calls, n_up2, taps, env, [(u.sts[i].c, i, f) for i, f in u.forms()]


def _figures(case, taps, env, dtype, what):
  """Prints every stage's figure; returns [(stage, kind, figure, gate)] of the stages over (or without) their gate."""
  noise, tag, over = BR.noise_table(case, dtype), BR.TAG[dtype], []
  worst = {}
  for s in case["stages"]:
    got = taps[s.name]
    ref = BR.local_ref(s, taps, case["weights"], BR.F64, env)
    assert got.shape[1:] == ref.shape[1:] and got.shape[0] in (ref.shape[0], ref.shape[0] // 2), (s.name, got.shape)
    assert bool(torch.isfinite(got).all()), s.name
    if s.kind == "temb":
      f = BR.temb_figure(got, ref, noise[s.name], dtype, case["slices"])
    else:
      f = BR.figure(got, ref, noise[s.name], dtype)
    kind = BR.gate_kind(s.kind)
    gate = BR.GATES.get(kind, {}).get(tag)
    print(f"FIG {what:44s} {s.name:40s} {kind:10s} rows {got.shape[0]} noise {noise[s.name]:.2e} figure {f:8.4f} "
          f"gate {gate}")
    worst[kind] = max(worst.get(kind, 0.0), f)
    if gate is None or not f <= gate:
      over.append((s.name, kind, round(f, 4), gate))
  print(f"WORST {what} " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
  return over


@pytest.mark.parametrize("model,dtype,name,form", CASES, ids=[f"{m}-{BR.TAG[d]}-{n}-{f}" for m, d, n, f in CASES])
def test_unet_stages(dev, monkeypatch, model, dtype, name, form):
  kw, must, must_not, extra = (FORMS_BF16 if dtype == BF16 else FORMS_F32)[name]
  if model == "B":
    # the constructor's own thresholds: 1024 rows are below every one, the per-layer launches without the fold
    must, must_not, extra = ("ldm_attention", "ldm_layernorm"), ("ldm_attention_ms",) + PANEL, None
  calls, n_up2, taps, env, picked = _evaluate(dev, monkeypatch, model, dtype,
                                              {} if model == "B" else dict(SMALL, **kw), form)
  hist = {c: calls.count(c) for c in sorted(set(calls))}
  print(f"CALLS {model}-{BR.TAG[dtype]}-{name}-{form}: {hist} conv3x3_up2={n_up2}")
  # ---- the form is the one it is named for
  for m in must:
    assert m in calls, f"{name}: {m} was not called"
  for m in must_not:
    assert m not in calls, f"{name}: {m} was called"
  assert (n_up2 > 0) == (name != "gather-upsample")
  print(f"FORMS {model}-{BR.TAG[dtype]}-{name}-{form}: " + " ".join(f"{i}:C{c}:{'/'.join(map(str, f))}" for c, i, f in picked))
  for c, i, f in picked:
    if model == "A":
      assert tuple(f[:4]) == (PICKED_BF16 if dtype == BF16 else PICKED_F32)[name][c], (name, c, i, f)
    else:
      assert (f.norm, f.ms, f.rest) == ("separate", False, "ffproj" if dtype == BF16 else "layers"), (c, i, f)
    # a pair leaves its common prefix in its first block, by copies unless that block is ONE launch over half the rows
    assert f.leave_prefix == (form == "paired" and i == 0 and f.rest != "block"), (name, form, c, i, f)
  key = (model, dtype, form)
  if name == "default":
    _BASE[key] = calls
  _BASE[key + (name,)] = calls
  if callable(extra) and key in _BASE:
    extra(calls, _BASE[key])
  if extra == "merged-ffproj" and key + (extra,) in _BASE:
    _gemms(N_ST_A)(calls, _BASE[key + (extra,)])
  if form == "paired":
    # the common prefix ran once: the first ResBlock's tap holds R/2 rows, the first transformer block's all
    assert taps["input_blocks/0/residual"].shape[0] == 2 and taps["input_blocks/0/spatial_transformer"].shape[0] == 4
    if name != "default":
      assert calls.count("ldm_cast") > 1             # per-layer forms leave the prefix by copying rows
  if form == "context_rows":
    assert all(t.shape[0] == 2 for t in taps.values())
  over = _figures(BR.unet_case(model), taps, env, dtype, f"{model}-{BR.TAG[dtype]}-{name}-{form}")
  assert not over, f"stages over their gate (stage, kind, figure, gate): {over}"


AE_CASES = [(m, d) for m in ("kl-dec", "kl-full-dec", "kl-full-enc") for d in (F32, BF16)]


@pytest.mark.parametrize("model,dtype", AE_CASES, ids=[f"{m}-{BR.TAG[d]}" for m, d in AE_CASES])
def test_autoencoder_stages(dev, monkeypatch, model, dtype):
  """KL_CFG's decoder on an 8x8 latent (c = 256: the blocked-logits attention) and the full-width KL decoder and
  encoder (channels=128; mid block at C = 512: attn_wide_kernel) on a 1x8x8 latent / a 1x64x64 image."""
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  c = BR.ae_case(model)
  x = c["env"]["x"].to(dev)
  ae = AutoencoderKL(**c["cfg"], weights=c["weights"], dtype=dtype, device=dev)
  run = ((lambda **k: ae.encode(x, **k)._moments) if model.endswith("enc") else (lambda **k: ae.decode(x, **k)))
  run()
  res = []
  calls, _ = _record(monkeypatch, lambda: res.append(run()))
  taps = {}
  calls_t, _ = _record(monkeypatch, lambda: res.append(run(taps=taps)))
  assert calls_t == calls and torch.equal(res[0], res[1]) and torch.equal(taps["out"], res[0])
  assert set(taps) == {s.name for s in c["stages"]}
  print(f"CALLS {model}-{BR.TAG[dtype]}: { {k: calls.count(k) for k in sorted(set(calls))} }")
  if model == "kl-dec":
    assert "ldm_softmax_rows" in calls and "ldm_attention" not in calls
  else:
    assert "ldm_attention" in calls and "ldm_softmax_rows" not in calls
  # a batch that needs more than one chunk, and a capturing stream, are refused
  side = ae._encoder if model.endswith("enc") else ae._decoder
  if model == "kl-dec":
    side.max_chunk = 1
    with pytest.raises(ValueError):
      run(taps={})
    side.max_chunk = 16
  monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
  with pytest.raises(ValueError):
    run(taps={})
  monkeypatch.undo()
  over = _figures(c, taps, c["env"], dtype, f"{model}-{BR.TAG[dtype]}")
  assert not over, f"stages over their gate (stage, kind, figure, gate): {over}"
