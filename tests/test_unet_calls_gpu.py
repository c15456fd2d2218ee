"""The C-ABI calls of one U-Net evaluation, pinned.

`UNet.forward` only walks the block structure; which entry points it reaches, and in which order, is the whole of
its behaviour on the host.  tests/golden/unet_call_order.json holds that order for every host path the walk has --
plain, the CFG pair's shared prefix (per-layer and ldm_st_block's in_rows form), the conditional half of a resident
context, the two-launch ResBlock shortcut -- recorded once through the `_CountingLib` proxy of
tests/test_img2img_gpu.py.  A change to the walk that is meant to keep the launches must reproduce the file; one
that is meant to change them regenerates it and says so.  Each case also checks that the evaluation captured in a
graph and replayed gives the bits of the eager one.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ldm_tf2_amd import ops, weights as Wt  # noqa: E402

from test_img2img_gpu import _CountingLib  # noqa: E402
from test_models_gpu import CTX_DIM, UNET_CFG  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_call_order.json")
R, HW = 4, 16
F32, BF16 = torch.float32, torch.bfloat16
# the model of test_round4_gpu.py::test_paired_rows_share_the_prefix that reaches ldm_st_block (bf16)
MC320_CFG = dict(model_channels=320, out_channels=4, num_blocks=1, channel_mult=(1, 2), num_heads=8)
MC320_KW = dict(ffn_min_rows=1, fold_min_rows=1)
# name -> (model, dtype, constructor kwargs, form of the call)
CASES = {
    "tiny-f32-plain": ("tiny", F32, {}, "plain"),
    "tiny-bf16-plain": ("tiny", BF16, {}, "plain"),
    "tiny-f32-paired": ("tiny", F32, {}, "paired"),
    "tiny-bf16-paired": ("tiny", BF16, {}, "paired"),
    "tiny-f32-context-rows": ("tiny", F32, {}, "context_rows"),
    "tiny-bf16-context-rows": ("tiny", BF16, {}, "context_rows"),
    "mc320-bf16-plain": ("mc320", BF16, MC320_KW, "plain"),
    "mc320-bf16-paired": ("mc320", BF16, MC320_KW, "paired"),
    "tiny-f32-two-launch-shortcut": ("tiny", F32, dict(merge_shortcut=False), "plain"),
}


@pytest.fixture(scope="module")
def model_w():
  cache = {}

  def get(model):
    if model not in cache:
      cfg, seed = (UNET_CFG, 2) if model == "tiny" else (MC320_CFG, 4)
      cache[model] = (cfg, Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **cfg), seed=seed, mode="random",
                                           scope="unet"))
    return cache[model]
  return get


def evaluation(dev, cfg, w, dtype, kw, form):
  """(call, out): `call()` is one forward of a fresh model into `out`, in the form the case names."""
  from ldm_tf2_amd.unet import UNet
  g = np.random.default_rng(7)
  xh = g.standard_normal((R // 2, HW, HW, 4)).astype(np.float32)
  x = torch.from_numpy(np.concatenate([xh, xh], 0)).to(dev)           # rows r and r + R/2 pair up
  ctx = torch.from_numpy(g.standard_normal((R, 77, CTX_DIM)).astype(np.float32)).to(dev)
  t = torch.full((R,), 481, dtype=torch.int32, device=dev)
  u = UNet(**cfg, context_dim=CTX_DIM, weights=w, dtype=dtype, device=dev, **kw)
  u.set_context(ctx)
  fkw = dict(t_rows=t, shared_t=True)
  if form == "paired":
    fkw["paired_rows"] = True
  elif form == "context_rows":
    x = x[:2].contiguous()
    fkw = dict(t_rows=t[:2].contiguous(), shared_t=True, context_rows=(2, 4))
  out = torch.empty(x.shape[0], HW, HW, 4, device=dev)
  return (lambda: u.forward(x, out=out, **fkw)), out


def record_calls(monkeypatch, fn):
  proxy = _CountingLib(ops.lib)
  monkeypatch.setattr(ops, "lib", proxy)
  try:
    fn()
  finally:
    monkeypatch.setattr(ops, "lib", proxy._lib)
  torch.cuda.synchronize()
  return proxy.calls


@pytest.mark.parametrize("case", list(CASES))
def test_the_calls_of_one_evaluation(dev, case, model_w, monkeypatch):
  model, dtype, kw, form = CASES[case]
  cfg, w = model_w(model)
  call, out = evaluation(dev, cfg, w, dtype, kw, form)
  call()                                      # the first evaluation allocates the model's scratch
  torch.cuda.synchronize()
  calls = record_calls(monkeypatch, call)
  eager = out.clone()
  with open(GOLDEN) as f:
    want = json.load(f)[case]
  print(f"{case}: {len(calls)} calls ({len(want)} recorded), {len(set(calls))} entry points")
  first = next((i for i, (a, b) in enumerate(zip(calls, want)) if a != b), min(len(calls), len(want)))
  assert calls == want, f"call {first}: {calls[first:first + 3]} where the record has {want[first:first + 3]}"
  if model == "mc320" and form == "paired":
    assert "ldm_st_block" in calls
  assert bool(torch.isfinite(eager).all())
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    call()
  out.zero_()
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out, eager), "the captured evaluation differs from the eager one"
