"""CPU tests (no GPU): the C-ABI library loads and exports every symbol the header
declares; host logic (schedule, tokenizer, weight re-layout, sharding) against the
oracle and the reference's pins; the N > 1 path over gloo with world_size 2."""
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REF_VOCAB = os.path.join(GOLD, "bert_vocab.txt")      # the reference's bert_model/vocab.txt, unchanged


# ---- C ABI --------------------------------------------------------------------------
def _header_functions():
  src = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
  return set(re.findall(r"\b(ldm_[a-z0-9_]+)\s*\(", src)) - {"ldm_gemm_params"}


def test_library_exports_every_declared_symbol():
  import ctypes
  from ldm_tf2_amd import _lib
  declared = _header_functions()
  assert declared, "no functions parsed from include/ldm_hip.h"
  assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
  lib = ctypes.CDLL(_lib.LIB_PATH)
  for name in declared:
    assert getattr(lib, name) is not None
  assert _lib.lib.ldm_version() >= 100


def test_gemm_params_struct_matches_header():
  """field order of the ctypes mirror == field order of ldm_gemm_params in the header."""
  from ldm_tf2_amd._lib import GemmParams
  src = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
  body = src[src.index("typedef struct {"):src.index("} ldm_gemm_params;")]
  body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
  names = []
  for decl in body.split(";"):
    decl = decl.replace("typedef struct {", "").strip()
    if not decl:
      continue
    for part in decl.split(","):
      names.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0])
  assert names == [f[0] for f in GemmParams._fields_]


def test_ops_refuse_cpu_tensors():
  """the product path has no CPU fallback: host tensors are rejected loudly."""
  from ldm_tf2_amd import ops
  with pytest.raises(ValueError):
    ops.layernorm(torch.zeros(4, 64), torch.ones(64), torch.zeros(64), torch.zeros(4, 64))


def test_product_does_not_import_oracle():
  pkg = os.path.join(ROOT, "ldm_tf2_amd")
  for fn in os.listdir(pkg):
    if fn.endswith(".py"):
      assert "oracle" not in open(os.path.join(pkg, fn)).read().replace("# oracle", ""), fn


# ---- schedule (host product code) ---------------------------------------------------------
class _FakeModel:
  device = torch.device("cpu")


def _sampler(**ldm):
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), **ldm)


@pytest.mark.parametrize("n", [10, 50, 200])
def test_schedule_matches_oracle_and_golden(n):
  from oracle import ldm_oracle as O
  g = json.load(open(os.path.join(GOLD, "schedule_kats.json")))
  s = _sampler(num_steps=1000, beta_start=0.00085, beta_end=0.012, eta=0.7, num_ddim_steps=n)
  assert s._ddim_steps.dtype == np.int32
  assert s._ddim_steps.tolist() == g["ddim_steps"][str(n)]            # bit-exact integer table
  o = O.make_schedule(1000, 0.00085, 0.012, 0.7, n)
  assert np.array_equal(s._ddim_alphas_cumprod_prev, o["ddim_alphas_cumprod_prev"])
  assert np.array_equal(s._ddim_sigmas, o["ddim_sigmas"])
  assert np.array_equal(s._ddim_sqrt_recip_alphas_cumprod, o["ddim_sqrt_recip_alphas_cumprod"])
  assert np.array_equal(s._ddim_sqrt_recipm1_alphas_cumprod, o["ddim_sqrt_recipm1_alphas_cumprod"])
  assert s._ddim_alphas_cumprod_prev[0] == s._alphas_cumprod[0]       # not 1.0 (model_runners.py:412-415)


def test_schedule_rejects_non_divisor_step_count():
  with pytest.raises(IndexError):
    _sampler(num_steps=1000, beta_start=0.00085, beta_end=0.012, num_ddim_steps=300)


def test_decode_first_stage_rejects_unknown_autoencoder():
  s = _sampler(num_steps=1000, beta_start=0.00085, beta_end=0.012, num_ddim_steps=50)
  with pytest.raises(NotImplementedError):
    s.decode_first_stage(torch.zeros(1, 8, 8, 4))


def test_normal_latents_independent_of_sharding():
  from ldm_tf2_amd.model_runners import normal_latents
  full = normal_latents(0, 0, 8, (4, 4, 4))
  parts = np.concatenate([normal_latents(0, 0, 3, (4, 4, 4)), normal_latents(0, 3, 5, (4, 4, 4))])
  assert np.array_equal(full, parts)
  assert abs(full.mean()) < 0.2 and 0.8 < full.std() < 1.2


# ---- tokenizer ----------------------------------------------------------------------------
def test_token_id_fixture_shape():
  g = json.load(open(os.path.join(GOLD, "token_ids.json")))
  assert len(g["prompt_ids"]) == 77 and len(g["empty_ids"]) == 77
  assert g["prompt_ids"][:12] == [101, 1037, 7865, 6071, 2003, 2652, 2858, 1010, 3514, 2006, 10683, 102]
  assert g["empty_ids"][:3] == [101, 102, 0]


def test_tokenizer_against_reference_pins():
  """convert_ckpt_pytorch_to_tf2.py:384-392 hard-codes these ids."""
  from ldm_tf2_amd.tokenizer import BertWordPieceTokenizer, get_token_ids
  g = json.load(open(os.path.join(GOLD, "token_ids.json")))
  tok = BertWordPieceTokenizer(REF_VOCAB)
  assert len(tok) == 30522
  assert tok.encode(g["prompt"], 77).tolist() == g["prompt_ids"]
  assert tok.encode("", 77).tolist() == g["empty_ids"]
  ids = get_token_ids(g["prompt"], 4, REF_VOCAB, 77)
  assert ids.shape == (8, 77) and ids.dtype == np.int64
  assert (ids[:4] == np.array(g["empty_ids"])).all() and (ids[4:] == np.array(g["prompt_ids"])).all()
  for text in g["extra"]:
    assert tok.encode(text, 77).tolist() == g["extra"][text], text


# ---- weight re-layout -----------------------------------------------------------------------
def test_relayout_is_equivalent_to_reference_layout_math():
  from ldm_tf2_amd import layout as L
  from oracle import ldm_oracle as O
  g = torch.Generator().manual_seed(0)
  f32, cpu = torch.float32, "cpu"
  # conv: OHWI matrix times im2col(kh,kw,ci) == HWIO conv
  k = torch.randn(3, 3, 8, 5, generator=g)
  x = torch.randn(1, 4, 4, 8, generator=g)
  wt = L.conv_kernel(k.numpy(), f32, cpu)
  xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
  cols = torch.stack([xp[0, i:i + 4, j:j + 4, :] for i in range(3) for j in range(3)], dim=2).reshape(16, 72)
  assert torch.allclose((cols @ wt.t()).reshape(1, 4, 4, 5), O.conv2d(x, k, None), atol=1e-5)
  # split / merge projections with head padding
  kd = torch.randn(16, 2, 5, generator=g)
  xs = torch.randn(3, 16, generator=g)
  ws = L.split_kernel(kd.numpy(), 8, f32, cpu)
  got = (xs @ ws.t()).reshape(3, 2, 8)
  assert torch.allclose(got[..., :5], torch.einsum("td,dhs->ths", xs, kd), atol=1e-5)
  assert got[..., 5:].abs().max() == 0
  km = torch.randn(2, 5, 16, generator=g)
  wm = L.merge_kernel(km.numpy(), 8, f32, cpu)
  o = torch.zeros(3, 2, 8)
  o[..., :5] = torch.randn(3, 2, 5, generator=g)
  assert torch.allclose(o.reshape(3, 16) @ wm.t(), torch.einsum("ths,hsd->td", o[..., :5], km), atol=1e-5)
  # GEGLU interleave: blocks of 64 rows = 32 value rows then their 32 gate rows
  kg = torch.randn(16, 128, generator=g)
  bg = torch.randn(128, generator=g)
  wg, bgi = L.geglu_kernel(kg.numpy(), bg.numpy(), f32, cpu)
  xg = torch.randn(4, 16, generator=g)
  y = (xg @ wg.t() + bgi).reshape(4, 2, 2, 32)
  ref = xg @ kg + bg
  a, gate = ref[:, :64], ref[:, 64:]
  assert torch.allclose((y[:, :, 0] * O.gelu(y[:, :, 1])).reshape(4, 64), a * O.gelu(gate), atol=1e-5)


def test_weight_manifests_cover_reference_variable_counts():
  from ldm_tf2_amd import weights as Wt
  # convert_ckpt_pytorch_to_tf2.py: 32 layers x 13 + 4 transformer tensors
  assert len(Wt.transformer_manifest()) == 32 * 13 + 4
  m = Wt.unet_manifest()
  assert sum(1 for k in m if k.endswith("/shortcut/kernel")) == 2 + 12     # i in (4,7) + every output block
  assert sum(1 for k in m if "/upsample/conv/kernel" in k) == 3 and sum(1 for k in m if "/downsample/" in k) == 6
  w = Wt.init_weights(Wt.unet_manifest(model_channels=32, context_dim=64), seed=1)
  w2 = Wt.init_weights(Wt.unet_manifest(model_channels=32, context_dim=64), seed=1)
  assert all(np.array_equal(w[k], w2[k]) for k in w)


# ---- N > 1 over gloo (CPU) ---------------------------------------------------------------------
_WORKER = textwrap.dedent("""
    import os, sys
    import numpy as np, torch
    sys.path.insert(0, %r)
    from ldm_tf2_amd import distributed as D
    from ldm_tf2_amd.model_runners import normal_latents
    rank, world, local = D.init_from_env(backend="gloo")
    B = 3
    first, last = D.shard_range(rank, B)
    x = normal_latents(0, first, B, (2, 2, 4))
    # stand-in for "sample + decode": a per-sample function of x_T only
    imgs = torch.from_numpy(np.tanh(x) * (1 + np.arange(first, last)[:, None, None, None])).float()
    out = D.all_gather_images(imgs)
    t = D.max_over_ranks(float(rank + 1), torch.device("cpu"))
    D.barrier()
    if rank == 0:
      ref = normal_latents(0, 0, world * B, (2, 2, 4))
      ref = np.tanh(ref) * (1 + np.arange(world * B)[:, None, None, None])
      assert out.shape == (world * B, 2, 2, 4), out.shape
      assert np.allclose(out.numpy(), ref.astype(np.float32)), "gathered images != 1-process run"
      assert t == float(world)
      print("GLOO_OK")
""")


def test_sharded_sampling_and_all_gather_over_gloo(tmp_path):
  script = tmp_path / "worker.py"
  script.write_text(_WORKER % ROOT)
  env = dict(os.environ, MASTER_ADDR="127.0.0.1")
  r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                      "--master-addr", "127.0.0.1", "--master-port", "29613", str(script)],
                     capture_output=True, text=True, timeout=240, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
  assert "GLOO_OK" in r.stdout


def test_product_library_reads_no_environment_switch():
  """VERDICT r2 #7 / ADVICE: the timing ablations (LDM_G3_DEBUG) and tile A/B switches exist only in
  the tools build (`make tools`, -DLDM_TOOLS_BUILD).  The shipped library neither names an LDM_*
  variable nor imports getenv: no environment variable can change what it computes."""
  from ldm_tf2_amd import _lib
  data = open(_lib.LIB_PATH, "rb").read()
  import re
  names = set(re.findall(rb"LDM_[A-Z0-9_]{3,}", data))
  assert not names, f"environment-switch-like strings in {_lib.LIB_PATH}: {sorted(names)[:5]}"
  r = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True)
  if r.returncode == 0:
    assert "getenv" not in r.stdout.split(), "libldm_hip.so imports getenv"
