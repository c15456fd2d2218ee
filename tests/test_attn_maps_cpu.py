"""Cross-attention heat maps, host rules: the restatement against torch's softmax, the weight
table, the words' token positions, the aggregation formula and the CLI's keys.  Host-only: nothing runs on a GPU."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import attn_map_ref as A
from ldm_tf2_amd import run_ldm_sampler as R
from ldm_tf2_amd.model_runners import attention_step_weights, combine_attention_maps, word_heatmaps
from ldm_tf2_amd.tokenizer import BertWordPieceTokenizer

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = os.path.join(GOLD, "all_in_one_config.yaml")
VOCAB = os.path.join(GOLD, "bert_vocab.txt")


# ---- the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,T,Tk,heads,S,sp", [(2, 5, 77, 8, 40, 48), (1, 3, 5, 2, 8, 32), (1, 1, 1, 1, 32, 32)])
def test_maps64_is_the_head_averaged_softmax(R_, T, Tk, heads, S, sp):
  g = np.random.default_rng(T + Tk)
  q = g.standard_normal((R_, T, heads * sp)).astype(np.float32)
  k = g.standard_normal((R_, Tk, heads * sp)).astype(np.float32)
  pad = (np.arange(heads * sp) % sp) >= S
  scale = S ** -0.5
  acc0 = g.standard_normal((R_, T, Tk)).astype(np.float32)
  got = A.maps64(q, k, heads, S, sp, scale * np.log2(np.e), 0.75, acc0)
  q[..., pad] = np.nan                                              # the padded dims do not enter
  k[..., pad] = np.nan
  assert np.array_equal(A.maps64(q, k, heads, S, sp, scale * np.log2(np.e), 0.75, acc0), got)
  qh = torch.from_numpy(q).double().view(R_, T, heads, sp)[..., :S]
  kh = torch.from_numpy(k).double().view(R_, Tk, heads, sp)[..., :S]
  p = torch.softmax(scale * torch.einsum("rthd,rjhd->rhtj", qh, kh), -1).mean(1).numpy()
  assert np.abs(got - (acc0.astype(np.float64) + 0.75 * p)).max() <= 1e-13
  m32 = A.maps32(np.nan_to_num(q), np.nan_to_num(k), heads, S, sp, scale * np.log2(np.e), 0.75, acc0)
  assert m32.dtype == np.float32 and np.abs(m32 - got).max() <= 1e-5
  want, e32, delta = A.gate(np.nan_to_num(q), np.nan_to_num(k), heads, S, sp, scale * np.log2(np.e), 0.75, acc0)
  assert np.array_equal(want, got) and delta == max(2 * e32, 8 * 2. ** -24 * 0.75)


# ---- the weight table ----------------------------------------------------------------------------------
def test_attention_step_weights():
  assert attention_step_weights(5, None) is None
  w = attention_step_weights(5, True)
  assert w.dtype == np.float32 and np.array_equal(w, np.ones(5))
  w = attention_step_weights(3, [0, 2.5, 1])
  assert w.dtype == np.float32 and np.array_equal(w, [0., 2.5, 1.])
  assert np.array_equal(attention_step_weights(2, np.array([0., 1.], np.float64)), [0., 1.])
  assert np.array_equal(attention_step_weights(2, (1, 0)), [1., 0.])
  for bad in (False, [1., 2.], [1., 2., 3., 4.], [1., -0.5, 0.], [1., float("nan"), 0.], [1., float("inf"), 0.],
              [True, False, True], [0., 0., 0.], 3.0, "yes", [[1., 1., 1.]], [1e39, 0., 0.]):
    with pytest.raises(ValueError, match="attn_maps"):
      attention_step_weights(3, bad)


# ---- words ---------------------------------------------------------------------------------------------
def test_word_spans_follow_encode():
  tok = BertWordPieceTokenizer(VOCAB)
  pins = json.load(open(os.path.join(GOLD, "token_ids.json")))
  spans = tok.word_spans(pins["prompt"], 77)
  assert [w for w, _ in spans] == ["a", "virus", "monster", "is", "playing", "guitar", ",", "oil", "on", "canvas"]
  assert [p for _, p in spans] == [[i] for i in range(1, 11)]        # position 0 is [CLS]; the comma is a word
  assert tok.word_spans("", 77) == []
  # continuation pieces belong to their word
  text = "A corgi snowboarding, photorealistically!"
  ids = tok.encode(text, 77)
  spans = tok.word_spans(text, 77)
  assert [w for w, _ in spans] == ["a", "corgi", "snowboarding", ",", "photorealistically", "!"]
  assert any(len(p) > 1 for _, p in spans)
  flat = [p for _, pos in spans for p in pos]
  assert flat == list(range(1, len(flat) + 1)) and ids[flat[-1] + 1] == tok.sep_id
  inv = {i: t for t, i in tok.vocab.items()}
  for word, pos in spans:
    pieces = [inv[int(ids[p])] for p in pos]
    assert not pieces[0].startswith("##") and all(x.startswith("##") for x in pieces[1:])
    assert "".join(x[2:] if x.startswith("##") else x for x in pieces) == word


def test_word_spans_truncation():
  tok = BertWordPieceTokenizer(VOCAB)
  text = " ".join(["dog"] * 100)
  spans = tok.word_spans(text, 77)
  assert len(spans) == 75 and spans[-1][1] == [75]                   # 77 - [CLS] - [SEP]
  assert tok.encode(text, 77)[76] == tok.sep_id
  # a word the truncation cuts in the middle is dropped whole
  long = "photorealistically"
  n = len(tok._wordpiece(long))
  assert n > 1
  spans = tok.word_spans("dog " + long, 2 + 1 + n - 1)
  assert [w for w, _ in spans] == ["dog"]
  spans = tok.word_spans("dog " + long, 2 + 1 + n)
  assert [w for w, _ in spans] == ["dog", long] and spans[1][1] == list(range(2, 2 + n))
  assert tok.word_spans("dog", 2) == []


def test_word_heatmaps_sum_their_positions():
  g = np.random.default_rng(0)
  heat = g.random((2, 7, 3, 4)).astype(np.float32)
  spans = [("a", [1]), ("corgi", [2, 3, 4]), (",", [5])]
  wh = word_heatmaps(heat, spans)
  assert wh.shape == (2, 3, 3, 4) and wh.dtype == np.float32
  assert np.array_equal(wh[:, 0], heat[:, 1]) and np.array_equal(wh[:, 2], heat[:, 5])
  assert np.array_equal(wh[:, 1], heat[:, [2, 3, 4]].sum(1))
  assert word_heatmaps(heat, []).shape == (2, 0, 3, 4)
  with pytest.raises(ValueError):
    word_heatmaps(heat, [("x", [7])])
  with pytest.raises(ValueError):
    word_heatmaps(heat[0], spans)


# ---- the aggregation -------------------------------------------------------------------------------------
def _nearest(a, size):
  H, W = size
  ys, xs = np.arange(H) * a.shape[1] // H, np.arange(W) * a.shape[2] // W
  return a[:, ys][:, :, xs]


def test_aggregation_sums_to_one():
  """Every accumulator row sums to weight_sum (each of the steps that counted added a probability row times its
  weight): then sum_j heat = 1 at every pixel, whatever the layers' sizes, for a resize whose weights sum to 1."""
  g = np.random.default_rng(4)
  wsum, Tk, B = 3.5, 77, 2
  raw = []
  for h in (8, 4, 2, 8):
    p = g.random((B, h, h, Tk))
    raw.append((wsum * p / p.sum(-1, keepdims=True)).astype(np.float32))
  heat = combine_attention_maps(raw, wsum, size=(8, 8), resize=_nearest)
  assert heat.shape == (B, Tk, 8, 8) and heat.dtype == np.float32
  assert np.abs(heat.sum(1) - 1.).max() <= 1e-5
  want = sum(_nearest(a, (8, 8)).astype(np.float64) for a in raw) / (wsum * 4)
  assert np.abs(heat - want.transpose(0, 3, 1, 2)).max() <= 1e-6
  one = combine_attention_maps(raw[:1], wsum)                        # default size: the first layer's, no resize
  assert np.allclose(one, raw[0].transpose(0, 3, 1, 2) / wsum, rtol=1e-6)
  with pytest.raises(ValueError):
    combine_attention_maps(raw, wsum, size=(8, 8))                   # a smaller layer needs a resize
  with pytest.raises(ValueError):
    combine_attention_maps(raw[:1], 0.)
  with pytest.raises(ValueError):
    combine_attention_maps([], 1.)


# ---- the CLI's keys ----------------------------------------------------------------------------------------
def _cfg():
  with open(CFG) as f:
    return yaml.safe_load(f)


IDS = np.zeros((8, 77), dtype=np.int64)


def test_cli_attention_keys(tmp_path):
  cfg = _cfg()
  samp = cfg["ldm_sampling"]
  n = cfg["ldm"]["num_ddim_steps"]
  assert R.attention_map_settings(cfg) is None and R.sampling_call(cfg, IDS, 5)[2] == dict(seed=5)   # nothing changes
  samp["attention_maps"] = False
  assert R.attention_map_settings(cfg) is None and R.sampling_call(cfg, IDS, 5)[2] == dict(seed=5)
  samp["attention_maps"] = True
  method, _, kwargs = R.sampling_call(cfg, IDS, 5)
  assert method == "ddim_p_sample_loop" and kwargs == dict(seed=5, attn_maps=True)
  assert R.attention_map_settings(cfg) == dict(weights=True, size=None)
  samp.update(attention_map_steps=[2, 4], attention_map_size=[64, 48])
  am = R.attention_map_settings(cfg)
  assert am["size"] == (64, 48) and len(am["weights"]) == n
  assert [i for i, w in enumerate(am["weights"]) if w == 1.0] == [2, 3, 4] and set(am["weights"]) == {0.0, 1.0}
  assert np.array_equal(attention_step_weights(n, R.sampling_call(cfg, IDS, 5)[2]["attn_maps"]), am["weights"])
  # img2img takes it too
  np.save(tmp_path / "img.npy", np.zeros((64, 64, 3), np.uint8))
  samp["init_image"] = str(tmp_path / "img.npy")
  method, _, kwargs = R.sampling_call(cfg, IDS, 4)
  assert method == "ddim_p_sample_loop_img2img" and kwargs["attn_maps"] == am["weights"] and kwargs["seed"] == 4


@pytest.mark.parametrize("key,value", [("window", [16, 16]), ("hires_shape", [4, 16, 16, 4]), ("source_prompt", "a photo"),
                                       ("sample_save_progress", True), ("guidance_interval", [300, 700]),
                                       ("preview_freq", 2)])
def test_cli_attention_rejects_forbidden_pairs(tmp_path, key, value):
  cfg = _cfg()
  samp = cfg["ldm_sampling"]
  samp["sample_save_progress"] = False
  np.save(tmp_path / "img.npy", np.zeros((64, 64, 3), np.uint8))
  if key == "source_prompt":
    samp["init_image"] = str(tmp_path / "img.npy")
  samp[key] = value
  R.sampling_call(cfg, IDS, 0, source_ids=IDS)                       # the key alone is fine
  samp["attention_maps"] = True
  with pytest.raises(ValueError, match=f"attention_maps cannot be combined with ldm_sampling.{key}"):
    R.sampling_call(cfg, IDS, 0, source_ids=IDS)


def test_cli_attention_rejects_scale_lists_and_bad_values():
  cfg = _cfg()
  samp = cfg["ldm_sampling"]
  samp["attention_maps"] = True
  samp["guidance_scale"] = [5.] * cfg["ldm"]["num_ddim_steps"]
  with pytest.raises(ValueError, match="attention_maps cannot be combined with a list ldm_sampling.guidance_scale"):
    R.sampling_call(cfg, IDS, 0)
  n = cfg["ldm"]["num_ddim_steps"]
  for key, value in (("attention_maps", 1), ("attention_maps", "yes"), ("attention_map_steps", [3]),
                     ("attention_map_steps", [4, 2]), ("attention_map_steps", [-1, 2]), ("attention_map_steps", [0, n]),
                     ("attention_map_steps", [0.5, 2]), ("attention_map_steps", [True, 2]), ("attention_map_size", [0, 8]),
                     ("attention_map_size", [8]), ("attention_map_size", 8), ("attention_map_size", [8.0, 8])):
    cfg = _cfg()
    cfg["ldm_sampling"]["attention_maps"] = True
    cfg["ldm_sampling"][key] = value
    with pytest.raises(ValueError, match=key):
      R.sampling_call(cfg, IDS, 0)
  for key, value in (("attention_map_steps", [0, 2]), ("attention_map_size", [8, 8])):
    cfg = _cfg()
    cfg["ldm_sampling"][key] = value
    with pytest.raises(ValueError, match=f"{key} needs ldm_sampling.attention_maps"):
      R.sampling_call(cfg, IDS, 0)


def test_only_the_two_loops_run_with_attn_maps():
  import inspect
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler as S
  for name in ("ddim_p_sample_loop", "ddim_p_sample_loop_img2img"):
    params = inspect.signature(getattr(S, name)).parameters
    assert params["attn_maps"].default is None and params["attn_layers"].default is None
  for name in ("ddim_p_sample_loop_panorama", "ddim_p_sample_loop_hires", "ddim_p_sample_loop_edit", "ddim_invert_loop",
               "ddim_p_sample_loop_progressive"):
    params = inspect.signature(getattr(S, name)).parameters
    assert params["attn_maps"].default is None and "attn_layers" not in params
  with pytest.raises(ValueError, match="attn_maps and the panorama loop do not combine"):
    S._no_attn_maps(True, "the panorama loop")
  S._no_attn_maps(None, "the panorama loop")
