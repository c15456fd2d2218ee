"""Stage-local float64 references for the U-Net and the autoencoders (plain module, torch on the CPU).

The host models can store a clone of every stage's output (`UNet.forward(taps=)`, `decode / encode(taps=)`).  This
module restates the block structure as a list of stages, each run by ONE call of the oracle's stage functions, so
that a single stage can be recomputed in float64 from exactly the values the GPU stage was handed -- its own input
taps, widened -- and an error of one ResBlock or transformer block is not diluted by the rest of the model.

  walk        the stage list chained: equals O.unet_forward / decoder_forward / encoder_forward bit for bit
  local_ref   one stage from the taps that are its inputs, in any dtype
  figure      ||got - ref64|| / max(noise, u ||ref64||): the stage's error in units of what the ORACLE loses on the
              same stage in the same storage type (noise: local_ref in the storage type from the oracle's own taps
              rounded to it, against float64 on the same inputs); u = 2^-24 (float32), 2^-8 (bf16).  Nothing the GPU
              produced is in the denominator.
  calibrated_weights   init_weights(mode="random") has attention logits with a standard deviation of 0.02 .. 0.17: a
              softmax row is a near-uniform average (largest probability 1/256 at T = 256) and a wrong scale or a
              dropped LayerNorm beta moves the output by a fraction of the bf16 noise.  Every attention layer's query
              and key kernels are rescaled by one factor so that its float64 logits have a standard deviation in
              [2, 4]; the context is N(0, 4^2) per row and the rows' timesteps differ.
  MUTANTS     float64 stage references with ONE planted host-level error each; tests/test_block_parity_cpu.py prints
              their size in figure units and asserts that the core ones clear GATES.

GATES (figure units) per stage kind and storage type: twice the largest figure of the first MI355X run of
tests/test_zz_block_parity_gpu.py, rounded up to one significant digit (the convention of small_probes.py).  The
measured table is MEASURED below and in DESIGN.md.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from ldm_tf2_amd import layout as L
from ldm_tf2_amd import weights as Wt
from oracle import ldm_oracle as O

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
TAG = {F32: "f32", BF16: "bf16"}

CTX_DIM = 128
HEADS = 8
UNET_A = dict(model_channels=320, out_channels=4, num_blocks=1, channel_mult=(1, 2), num_heads=HEADS)      # MC320_CFG
UNET_B = dict(model_channels=64, out_channels=4, num_blocks=2, channel_mult=(1, 2, 4, 4), num_heads=HEADS)  # UNET_CFG
KL_SMALL = dict(latent_channels=4, channels=64, num_blocks=2, multipliers=(1, 2, 4, 4))                     # KL_CFG
KL_FULL = dict(latent_channels=4, channels=128, num_blocks=2, multipliers=(1, 2, 4, 4))

# The largest figure of each stage kind in the first MI355X run of tests/test_zz_block_parity_gpu.py, over every
# launch form of the model: {(model, storage type): {kind: figure}}.  In bf16 every stage is below 1: the HIP path
# loses less than the bf16 oracle (float32 accumulation, folded LayerNorms, panels kept in LDS).  In float32 the stages
# sit at the oracle's own float32 loss, but for `temb` of model A (15): the device's sinusoidal embedding (exp, the
# product t f and cos / sin in float32: at t = 981 one ulp of the argument is 6e-5) against torch's, carried through
# the two-layer MLP; relative to the table it is 1e-6 and a wrong slice is 1e7 of these units.  A's bf16 `res` is 0.63
# in every form but the two-launch shortcut (0.74: the shortcut makes a bf16 round trip of its own there).
MEASURED = {
    ("A", "bf16"): dict(conv_in=0.4265, temb=0.7048, res=0.7414, st=0.7046, down=0.5819, up=0.6081, out=0.4034),
    ("A", "f32"): dict(conv_in=1.0967, temb=15.0545, res=0.7286, st=1.1170, down=0.2516, up=0.2275, out=0.3916),
    ("B", "bf16"): dict(conv_in=0.4245, temb=0.6742, res=0.6472, st=0.6862, down=0.6134, up=0.6107, out=0.3582),
    ("B", "f32"): dict(conv_in=0.9947, temb=1.1734, res=0.7986, st=1.0252, down=0.5150, up=0.3458, out=0.3946),
    ("kl-dec", "bf16"): dict(ae_conv_in=0.4235, ae_res=0.7595, ae_attn=0.5404, ae_up=0.6043, ae_out=0.2850),
    ("kl-dec", "f32"): dict(ae_conv_in=0.9483, ae_res=0.6613, ae_attn=1.2749, ae_up=0.3451, ae_out=0.2745),
    ("kl-full-dec", "bf16"): dict(ae_conv_in=0.4201, ae_res=0.7602, ae_attn=0.5578, ae_up=0.6016, ae_out=0.2554),
    ("kl-full-dec", "f32"): dict(ae_conv_in=0.9754, ae_res=0.5905, ae_attn=0.8993, ae_up=0.2450, ae_out=0.2739),
    ("kl-full-enc", "bf16"): dict(ae_conv_in=0.4257, ae_res=0.6147, ae_down=0.6239, ae_attn=0.6310, ae_out=0.4063),
    ("kl-full-enc", "f32"): dict(ae_conv_in=1.1399, ae_res=0.3692, ae_down=0.3826, ae_attn=0.9309, ae_out=0.2215),
}
# kind -> storage type -> gate in figure units: twice the largest MEASURED figure of the kind, rounded up to one
# significant digit (tests/test_block_parity_cpu.py re-derives the table from MEASURED)
GATES = {
    "conv_in": dict(bf16=0.9, f32=3.0), "temb": dict(bf16=2.0, f32=40.0), "res": dict(bf16=2.0, f32=2.0),
    "st": dict(bf16=2.0, f32=3.0), "down": dict(bf16=2.0, f32=2.0), "up": dict(bf16=2.0, f32=0.7),
    "out": dict(bf16=0.9, f32=0.8),
    "ae_conv_in": dict(bf16=0.9, f32=3.0), "ae_res": dict(bf16=2.0, f32=2.0), "ae_attn": dict(bf16=2.0, f32=3.0),
    "ae_up": dict(bf16=2.0, f32=0.7), "ae_down": dict(bf16=2.0, f32=0.8), "ae_out": dict(bf16=0.9, f32=0.6),
}


class Stage:
  """One stage: `name` (= its tap), `kind`, weight `prefix`, `inputs` (tap names; "@x" = the model's input)."""

  def __init__(self, name, kind, prefix, inputs):
    self.name, self.kind, self.prefix, self.inputs = name, kind, prefix, tuple(inputs)

  def __repr__(self):
    return f"Stage({self.name}, {self.kind}, inputs={self.inputs})"


# ----------------------------------------------------------------------------------------------------------------
# stage lists
# ----------------------------------------------------------------------------------------------------------------

def unet_stages(weights):
  has = lambda p: any(k.startswith(p) for k in weights)
  S = [Stage("conv_in", "conv_in", "", ["@x"]), Stage("temb", "temb", "", [])]
  prev, skips, i = "conv_in", ["conv_in"], 0
  while has(f"input_blocks/{i}/"):
    p = f"input_blocks/{i}"
    if (p + "/downsample/conv/kernel") in weights:
      S.append(Stage(p + "/downsample", "down", p + "/downsample/conv/", [prev]))
      prev = S[-1].name
    else:
      S.append(Stage(p + "/residual", "res", p + "/residual/", [prev]))
      prev = S[-1].name
      if has(p + "/spatial_transformer/"):
        S.append(Stage(p + "/spatial_transformer", "st", p + "/spatial_transformer/", [prev]))
        prev = S[-1].name
    skips.append(prev)
    i += 1
  for n, kind in (("residual1", "res"), ("spatial_transformer", "st"), ("residual2", "res")):
    S.append(Stage("middle_block/" + n, kind, f"middle_block/{n}/", [prev]))
    prev = S[-1].name
  j = 0
  while has(f"output_blocks/{j}/"):
    p = f"output_blocks/{j}"
    S.append(Stage(p + "/residual", "res", p + "/residual/", [prev, skips.pop()]))      # concat(previous, skip)
    prev = S[-1].name
    if has(p + "/spatial_transformer/"):
      S.append(Stage(p + "/spatial_transformer", "st", p + "/spatial_transformer/", [prev]))
      prev = S[-1].name
    if (p + "/upsample/conv/kernel") in weights:
      S.append(Stage(p + "/upsample", "up", p + "/upsample/conv/", [prev]))
      prev = S[-1].name
    j += 1
  S.append(Stage("out", "out", "", [prev]))
  return S


def _ae_path(weights, side, S, prev, attention_resolutions, size):
  """The up / down blocks of one autoencoder side; returns (prev, size)."""
  i, step = 0, ("up" if side == "decoder" else "down")
  while any(k.startswith(f"{side}/{step}/{i}/") for k in weights):
    p = f"{side}/{step}/{i}"
    if (p + "/conv/kernel") in weights:
      S.append(Stage(f"{step}/{i}", "ae_" + step, p + "/conv/", [prev]))
      size = size * 2 if step == "up" else size // 2
    else:
      attn = size in tuple(attention_resolutions)
      S.append(Stage(f"{step}/{i}", "ae_res_attn" if attn else "ae_res", p + "/", [prev]))
    prev = S[-1].name
    i += 1
  return prev, size


def _ae_middle(S, side, prev):
  for n, kind in (("residual1", "ae_res_mid"), ("attention", "ae_attn"), ("residual2", "ae_res_mid")):
    S.append(Stage("middle/" + n, kind, f"{side}/middle/{n}/", [prev]))
    prev = S[-1].name
  return prev


def decoder_stages(weights, attention_resolutions=(), latent_size=8):
  S = [Stage("conv_in", "ae_conv_in", "decoder/", ["@x"])]
  prev = _ae_middle(S, "decoder", "conv_in")
  prev, _ = _ae_path(weights, "decoder", S, prev, attention_resolutions, latent_size)
  S.append(Stage("out", "ae_out", "decoder/", [prev]))
  return S


def encoder_stages(weights, attention_resolutions=(), image_size=64):
  S = [Stage("conv_in", "ae_conv_in", "encoder/", ["@x"])]
  prev, _ = _ae_path(weights, "encoder", S, "conv_in", attention_resolutions, image_size)
  prev = _ae_middle(S, "encoder", prev)
  S.append(Stage("out", "ae_out", "encoder/", [prev]))
  return S


# the gate a stage kind reads (the AE middle ResBlocks and a ResBlock + attention pair count as `ae_res` / `ae_attn`)
GATE_KIND = {"ae_res_mid": "ae_res", "ae_res_attn": "ae_attn"}


def gate_kind(kind):
  return GATE_KIND.get(kind, kind)


# ----------------------------------------------------------------------------------------------------------------
# one stage
# ----------------------------------------------------------------------------------------------------------------

class _WZ(O.W):
  """O.W with the tensors named in `zero` (full names) replaced by zeros: a dropped bias or beta."""

  def __init__(self, weights, dtype, prefix="", zero=()):
    super().__init__(weights, dtype, prefix)
    self.zero = frozenset(zero)

  def __call__(self, name):
    t = super().__call__(name)
    return torch.zeros_like(t) if (self.p + name) in self.zero else t

  def sub(self, name):
    return _WZ(self.w, self.dtype, self.p + name + "/", self.zero)


def temb_mlp(t, weights, dtype):
  """unet.py:125-127 exactly as O.unet_forward forms it: [R, 4 mc] in `dtype`."""
  w = O.W(weights, dtype)
  mc = w("conv_in/bias").shape[0]
  temb = O.get_time_embedding(t, mc, dtype)
  return O.dense(O.silu(O.dense(temb, w("time_dense1/kernel"), w("time_dense1/bias"))),
                 w("time_dense2/kernel"), w("time_dense2/bias"))


def res_prefixes(stages):
  return [s.prefix for s in stages if s.kind == "res"]


def temb_slices(stages, weights):
  """[(prefix, offset, cout)] of the ResBlocks' slices of the projected temb table, in the model's order."""
  out, off = [], 0
  for p in res_prefixes(stages):
    c = weights[p + "dense/bias"].shape[0]
    out.append((p, off, c))
    off += c
  return out


def run_stage(stage, ins, weights, dtype, env, zero=()):
  """ONE stage through the oracle's stage functions.  `ins`: its input tensors in `dtype`; `env`: x-independent
  inputs -- `t` (int rows), `ctx` [R, Tk, D], `temb` (the time MLP's output, any dtype), `stages`."""
  w = _WZ(weights, dtype, stage.prefix, zero)
  k = stage.kind
  if k == "conv_in":
    return O.conv2d(ins[0], w("conv_in/kernel"), w("conv_in/bias"))
  if k == "temb":
    te = O.silu(env["temb"].to(dtype))
    return torch.cat([O.dense(te, O._t(weights[p + "dense/kernel"], dtype), O._t(weights[p + "dense/bias"], dtype))
                      for p in res_prefixes(env["stages"])], -1)
  if k == "res":
    x = ins[0] if len(ins) == 1 else torch.cat([ins[0], ins[1]], dim=-1)               # unet.py:135
    return O.unet_residual_block(x, env["temb"].to(dtype), w)
  if k == "st":
    return O.unet_spatial_transformer(ins[0], env["ctx"].to(dtype), w, HEADS)
  if k == "down":
    return O.conv2d(ins[0], w("kernel"), w("bias"), stride=2, pad=((1, 1), (1, 1)))
  if k == "up":
    return O.conv2d(O.upsample_nearest2x(ins[0]), w("kernel"), w("bias"))
  if k == "out":
    h = O.silu(O.group_norm(ins[0], w("groupnorm/gamma"), w("groupnorm/beta"), eps=1e-5))
    return O.conv2d(h, w("conv_out/kernel"), w("conv_out/bias"))
  # ---- autoencoders
  side = stage.prefix.split("/")[0]
  if k == "ae_conv_in":
    x = ins[0]
    if side == "decoder":
      top = _WZ(weights, dtype, "", zero)
      x = O.dense(x, top("post_quant_conv/kernel"), top("post_quant_conv/bias"))
    return O.conv2d(x, w("conv_in/kernel"), w("conv_in/bias"))
  if k == "ae_res_mid":
    return O.ae_residual_block(ins[0], w)
  if k == "ae_res":
    return O.ae_residual_block(ins[0], w.sub("residual"))
  if k == "ae_res_attn":
    return O.ae_attention_block(O.ae_residual_block(ins[0], w.sub("residual")), w.sub("attention"))
  if k == "ae_attn":
    return O.ae_attention_block(ins[0], w)
  if k == "ae_up":
    return O.conv2d(O.upsample_nearest2x(ins[0]), w("kernel"), w("bias"))
  if k == "ae_down":
    return O.conv2d(ins[0], w("kernel"), w("bias"), stride=2, pad=((0, 1), (0, 1)))
  if k == "ae_out":
    h = O.conv2d(O.silu(O.group_norm(ins[0], w("group_norm/gamma"), w("group_norm/beta"), eps=O.AE_GN_EPS)),
                 w("conv_out/kernel"), w("conv_out/bias"))
    if side == "encoder":
      top = _WZ(weights, dtype, "", zero)
      h = O.dense(h, top("quant_conv/kernel"), top("quant_conv/bias"))
    return h
  raise ValueError(k)


def walk(stages, weights, dtype, env, mutate=None, base=None):
  """The stages chained in `dtype` from env["x"]: {tap name: tensor}.  `mutate` {stage name: fn(stage, ins, weights,
  dtype, env)} replaces single stages (a planted error carried to the whole output); `base`: the taps of the same
  walk without `mutate`, reused for the stages in front of the first replaced one."""
  env = dict(env, stages=stages)
  if "t" in env:
    env["temb"] = temb_mlp(env["t"], weights, dtype)
  taps = {}
  with torch.no_grad():
    for s in stages:
      if base is not None and not any(n in taps for n in (mutate or {})) and s.name not in (mutate or {}):
        taps[s.name] = base[s.name]
        continue
      ins = [O._t(env["x"], dtype) if n == "@x" else taps[n] for n in s.inputs]
      fn = (mutate or {}).get(s.name)
      taps[s.name] = run_stage(s, ins, weights, dtype, env) if fn is None else fn(s, ins, weights, dtype, env)
  return taps


def _rows(t, n):
  """`t` with n rows: a stage of a CFG pair's common prefix holds the first half, both halves being equal."""
  return t if t.shape[0] == n else torch.cat([t] * (n // t.shape[0]), 0)


def stage_inputs(stage, taps, dtype, env):
  """The stage's inputs, widened to `dtype`, from `taps` (the taps of the run under test)."""
  n = env["x"].shape[0]
  return [O._t(env["x"], dtype) if name == "@x" else _rows(taps[name].detach().cpu().to(dtype), n)
          for name in stage.inputs]


def local_ref(stage, taps, weights, dtype, env, fn=None):
  """ONE stage in `dtype` from the taps that are its inputs (widened: exactly what the stage was given).  Weights are
  the float32 masters widened to `dtype`; the ResBlocks' temb is the oracle's float64 one from `t` (env["temb"])."""
  with torch.no_grad():
    ins = stage_inputs(stage, taps, dtype, env)
    return (run_stage if fn is None else fn)(stage, ins, weights, dtype, env)


def rel(a, b):
  a, b = a.detach().cpu().double(), b.detach().cpu().double()
  return ((a - b).norm() / b.norm()).item()


def figure(got, ref64, noise, dtype):
  """||got - ref64|| / max(noise ||ref64||, u ||ref64||); `noise` is relative to ||ref64|| already.  A tap with
  fewer rows than the reference (the common prefix of a CFG pair) is compared with those rows."""
  got = got.detach().cpu().double()
  ref64 = ref64[:got.shape[0]]
  return rel(got, ref64) / max(noise, U[dtype])


def temb_figure(got, ref64, noise, dtype, slices):
  """The projected temb table slice by slice (a wrong `temb_off` moves whole slices): the largest slice figure."""
  got = got.detach().cpu().double()
  ref64 = ref64[:got.shape[0]]
  return max(rel(got[:, o:o + c], ref64[:, o:o + c]) for _, o, c in slices) / max(noise, U[dtype])


# ----------------------------------------------------------------------------------------------------------------
# calibrated inputs
# ----------------------------------------------------------------------------------------------------------------

class _Spy:
  """Records (layer prefix, logit std, mean largest probability) of every attention the oracle runs (float64)."""

  def __init__(self):
    self.seen = []

  def __enter__(self):
    self._mha, self._ae = O.multihead_attention, O.ae_attention_block
    seen, mha, ae = self.seen, self._mha, self._ae

    def spy_mha(query, context, w, scale_dim):
      q, k = O.projection_split(query, w("query/kernel")), O.projection_split(context, w("key/kernel"))
      lg = torch.einsum("nqhs,nchs->nhqc", q, k) * (q.shape[-1] ** -0.5)
      seen.append((w.p, ("query/kernel", "key/kernel"), lg.std().item(),
                   torch.softmax(lg, 3).max(3).values.mean().item()))
      return mha(query, context, w, scale_dim)

    def spy_ae(x, w):
      b, hh, ww, c = x.shape
      h = O.group_norm(x, w("group_norm/gamma"), w("group_norm/beta"), eps=O.AE_GN_EPS)
      q = O.dense(h, w("dense_query/kernel"), w("dense_query/bias")).reshape(b, hh * ww, c)
      k = O.dense(h, w("dense_key/kernel"), w("dense_key/bias")).reshape(b, hh * ww, c)
      lg = torch.einsum("bqc,bkc->bqk", q, k) * (c ** -0.5)
      seen.append((w.p, ("dense_query/kernel", "dense_query/bias", "dense_key/kernel", "dense_key/bias"),
                   lg.std().item(), torch.softmax(lg, -1).max(-1).values.mean().item()))
      return ae(x, w)

    O.multihead_attention, O.ae_attention_block = spy_mha, spy_ae
    return self

  def __exit__(self, *exc):
    O.multihead_attention, O.ae_attention_block = self._mha, self._ae


def attention_stats(stages, weights, env):
  """[(layer prefix, tensor names, logit std, mean largest probability)] of a float64 walk."""
  with _Spy() as spy:
    walk(stages, weights, F64, env)
  return spy.seen


def calibrated_weights(weights, stages, env, target=3.0, passes=3):
  """A copy of `weights` in which every attention layer's query and key tensors are rescaled by one factor per layer
  so that its float64 logits have a standard deviation near `target` (measure-and-rescale, `passes` times: rescaling
  a layer moves the inputs of the ones behind it)."""
  w = dict(weights)
  for _ in range(passes):
    for p, names, sd, _ in attention_stats(stages, w, env):
      f = (target / sd) ** 0.5
      for n in names:
        w[p + n] = (w[p + n] * np.float32(f)).astype(np.float32)
  return w


# ----------------------------------------------------------------------------------------------------------------
# the cases both test modules use (built once per process)
# ----------------------------------------------------------------------------------------------------------------

def unet_inputs(R=4, hw=16, seed=7):
  """A 2+2 CFG pair: rows r and r + R/2 share x and t and differ in their context; the timesteps within a half
  differ; context rows are independent N(0, 4^2)."""
  g = np.random.default_rng(seed)
  xh = g.standard_normal((R // 2, hw, hw, 4)).astype(np.float32)
  x = np.concatenate([xh, xh], 0)
  ctx = (4.0 * g.standard_normal((R, 77, CTX_DIM))).astype(np.float32)
  th = np.array([981, 21, 500, 261][:R // 2], dtype=np.int32)
  return x, np.concatenate([th, th]), ctx


@functools.lru_cache(maxsize=None)
def unet_case(model):
  """dict(cfg, weights (calibrated), stages, env, taps64 (the oracle's own taps), slices)."""
  cfg, seed = {"A": (UNET_A, 4), "B": (UNET_B, 2)}[model]
  w0 = Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **cfg), seed=seed, mode="random", scope="unet")
  stages = unet_stages(w0)
  x, t, ctx = unet_inputs()
  env = dict(x=torch.from_numpy(x), t=t, ctx=torch.from_numpy(ctx))
  w = calibrated_weights(w0, stages, env)
  env = dict(env, stages=stages, temb=temb_mlp(t, w, F64))
  return dict(cfg=cfg, weights=w, raw_weights=w0, stages=stages, env=env, taps64=walk(stages, w, F64, env),
              slices=temb_slices(stages, w))


def sub_env(env, rows):
  """The inputs of rows [lo, hi) (forward(context_rows=(lo, hi)) on the conditional half)."""
  lo, hi = rows
  return dict(env, x=env["x"][lo:hi], t=env["t"][lo:hi], ctx=env["ctx"][lo:hi], temb=env["temb"][lo:hi])


@functools.lru_cache(maxsize=None)
def ae_case(model):
  """model: "kl-dec" (KL_SMALL, 8x8 latent), "kl-full-dec" (1x8x8), "kl-full-enc" (1x64x64 image)."""
  cfg = KL_SMALL if model == "kl-dec" else KL_FULL
  man = Wt.decoder_manifest(**cfg)
  man.update(Wt.encoder_manifest(image_size=64, **cfg))
  w0 = Wt.init_weights(man, seed=2, mode="random", scope="autoencoder")
  g = np.random.default_rng(11)
  if model.endswith("enc"):
    stages = encoder_stages(w0)
    x = (g.random((1, 64, 64, 3)) * 2 - 1).astype(np.float32)
  else:
    stages = decoder_stages(w0)
    x = g.standard_normal((2 if model == "kl-dec" else 1, 8, 8, 4)).astype(np.float32) / np.float32(0.18215)
  env = dict(x=torch.from_numpy(x))
  w = calibrated_weights(w0, stages, env)
  env = dict(env, stages=stages)
  return dict(cfg=cfg, weights=w, raw_weights=w0, stages=stages, env=env, taps64=walk(stages, w, F64, env))


def noise_table(case, dtype):
  """{stage name: the oracle's own loss on that stage in storage type `dtype`}: local_ref in `dtype` from the
  oracle's taps rounded to `dtype`, against float64 on the same rounded inputs, relative to the float64 norm.
  Cached on the case (once per configuration and storage type)."""
  cache = case.setdefault("_noise", {})
  if dtype not in cache:
    rounded = {k: v.to(dtype) for k, v in case["taps64"].items()}
    env = dict(case["env"], x=O._t(case["env"]["x"], dtype))
    tab = {}
    for s in case["stages"]:
      lo = local_ref(s, rounded, case["weights"], dtype, env)
      tab[s.name] = rel(lo, local_ref(s, rounded, case["weights"], F64, env))
    cache[dtype] = tab
  return cache[dtype]


# ----------------------------------------------------------------------------------------------------------------
# mutants: float64 stage references with ONE planted host-level error
# ----------------------------------------------------------------------------------------------------------------

def st_restated(x, context, w, heads, scale_dim=None, geglu_swap=None):
  """O.unet_spatial_transformer written out (bit for bit the same without the two hooks).  `scale_dim`: the head size
  the attention scale is taken from; `geglu_swap` = (row, t0, t1): value and gate halves swapped for those tokens."""
  def mha(query, ctx, aw):
    q, k = O.projection_split(query, aw("query/kernel")), O.projection_split(ctx, aw("key/kernel"))
    v = O.projection_split(ctx, aw("value/kernel"))
    lg = torch.einsum("nqhs,nchs->nhqc", q, k) * ((scale_dim or q.shape[-1]) ** -0.5)
    o = torch.einsum("nhqc,nchs->nqhs", torch.softmax(lg, dim=3), v)
    return O.projection_merge(o, aw("output/kernel"), aw("output/bias"))
  b, hh, ww, c = x.shape
  h = O.group_norm(x, w("groupnorm/gamma"), w("groupnorm/beta"), eps=1e-6)
  y = O.dense(h, w("dense1/kernel"), w("dense1/bias")).reshape(b, hh * ww, c)
  bw = w.sub("block")
  h = O.layer_norm(y, bw("layernorm1/gamma"), bw("layernorm1/beta"))
  y = mha(h, h, bw.sub("att_layer1")) + y
  h = O.layer_norm(y, bw("layernorm2/gamma"), bw("layernorm2/beta"))
  y = mha(h, context, bw.sub("att_layer2")) + y
  h = O.layer_norm(y, bw("layernorm3/gamma"), bw("layernorm3/beta"))
  g = O.dense(h, bw("ffn/geglu/kernel"), bw("ffn/geglu/bias"))
  a, gate = torch.chunk(g, 2, dim=-1)
  if geglu_swap is not None:
    r, t0, t1 = geglu_swap
    a, gate = a.clone(), gate.clone()
    a[r, t0:t1], gate[r, t0:t1] = gate[r, t0:t1].clone(), a[r, t0:t1].clone()
  y = O.dense(a * O.gelu(gate), bw("ffn/dense/kernel"), bw("ffn/dense/bias")) + y
  return O.dense(y.reshape(b, hh, ww, c), w("dense2/kernel"), w("dense2/bias")) + x


def res_restated(x, te, w, second_silu=True):
  """O.unet_residual_block with the projected temb `te` [R, Cout] handed in (bit for bit the same with the block's
  own projection and `second_silu`)."""
  h = O.silu(O.group_norm(x, w("group_norm_1/gamma"), w("group_norm_1/beta"), eps=1e-5))
  h = O.conv2d(h, w("conv2d_1/kernel"), w("conv2d_1/bias"))
  h = h + te[:, None, None, :]
  h = O.group_norm(h, w("group_norm_2/gamma"), w("group_norm_2/beta"), eps=1e-5)
  h = O.conv2d(O.silu(h) if second_silu else h, w("conv2d_2/kernel"), w("conv2d_2/bias"))
  if x.shape[-1] != h.shape[-1]:
    x = O.dense(x, w("shortcut/kernel"), w("shortcut/bias"))
  return h + x


def ae_attn_restated(x, w, scale_pow=-0.5):
  b, hh, ww, c = x.shape
  h = O.group_norm(x, w("group_norm/gamma"), w("group_norm/beta"), eps=O.AE_GN_EPS)
  q = O.dense(h, w("dense_query/kernel"), w("dense_query/bias")).reshape(b, hh * ww, c)
  k = O.dense(h, w("dense_key/kernel"), w("dense_key/bias")).reshape(b, hh * ww, c)
  v = O.dense(h, w("dense_value/kernel"), w("dense_value/bias")).reshape(b, hh * ww, c)
  a = torch.softmax(torch.einsum("bqc,bkc->bqk", q, k) * (c ** scale_pow), dim=-1)
  o = torch.einsum("bqk,bkc->bqc", a, v).reshape(b, hh, ww, c)
  return O.dense(o, w("dense_output/kernel"), w("dense_output/bias")) + x


def _drop(*names):
  """The stage with the named tensors (relative to its prefix) zeroed; applies where all of them exist."""
  def fn(s, ins, weights, dtype, env):
    return run_stage(s, ins, weights, dtype, env, zero=[s.prefix + n for n in names])
  fn.applies = lambda s, weights: all((s.prefix + n) in weights for n in names)
  return fn


def _mut(applies=None):
  def deco(fn):
    fn.applies = applies or (lambda s, weights: True)
    return fn
  return deco


@_mut()
def _st_other_context(s, ins, weights, dtype, env):
  return run_stage(s, ins, weights, dtype, dict(env, ctx=env["ctx"].roll(1, 0)))


@_mut()
def _gain(s, ins, weights, dtype, env):
  x = ins[0]
  return x + 1.05 * (run_stage(s, ins, weights, dtype, env) - x)


def _head(s, weights):
  return weights[s.prefix + "dense1/bias"].shape[0] // HEADS


@_mut(lambda s, weights: L.padded_head(_head(s, weights)) != _head(s, weights))
def _st_padded_scale(s, ins, weights, dtype, env):
  return st_restated(ins[0], env["ctx"].to(dtype), _WZ(weights, dtype, s.prefix), HEADS,
                     scale_dim=L.padded_head(_head(s, weights)))


@_mut()
def _st_zero_keys(s, ins, weights, dtype, env):
  c = env["ctx"].to(dtype)
  return run_stage(s, ins, weights, dtype, dict(env, ctx=torch.cat([c, torch.zeros_like(c[:, :3])], 1)))


@_mut()
def _st_geglu_swap(s, ins, weights, dtype, env):
  T = ins[0].shape[1] * ins[0].shape[2]
  return st_restated(ins[0], env["ctx"].to(dtype), _WZ(weights, dtype, s.prefix), HEADS, geglu_swap=(0, 0, min(64, T)))


def _own_te(s, weights, dtype, env, temb=None):
  te = O.silu((env["temb"] if temb is None else temb).to(dtype))
  return O.dense(te, O._t(weights[s.prefix + "dense/kernel"], dtype), O._t(weights[s.prefix + "dense/bias"], dtype))


def _res_x(ins):
  return ins[0] if len(ins) == 1 else torch.cat([ins[0], ins[1]], dim=-1)


@_mut()
def _res_other_temb(s, ins, weights, dtype, env):
  return res_restated(_res_x(ins), _own_te(s, weights, dtype, env, env["temb"].roll(1, 0)), _WZ(weights, dtype, s.prefix))


def _next_slice(s, env, weights):
  sl = temb_slices(env["stages"], weights)
  total = sl[-1][1] + sl[-1][2]
  _, off, c = next(e for e in sl if e[0] == s.prefix)
  return (off + c, c) if off + 2 * c <= total else None


@_mut()
def _res_next_temb(s, ins, weights, dtype, env):
  """temb_off of the following block: the slice [off + Cout, off + 2 Cout) of the projected table (the last block,
  whose following slice would leave the table, reads the preceding one)."""
  sl = temb_slices(env["stages"], weights)
  _, off, c = next(e for e in sl if e[0] == s.prefix)
  nxt = _next_slice(s, env, weights)
  o2 = nxt[0] if nxt is not None else off - c
  tall = run_stage(Stage("temb", "temb", "", []), [], weights, dtype, env)
  return res_restated(_res_x(ins), tall[:, o2:o2 + c], _WZ(weights, dtype, s.prefix))


@_mut()
def _res_no_second_silu(s, ins, weights, dtype, env):
  return res_restated(_res_x(ins), _own_te(s, weights, dtype, env), _WZ(weights, dtype, s.prefix), second_silu=False)


@_mut(lambda s, weights: len(s.inputs) == 2)
def _concat_swapped(s, ins, weights, dtype, env):
  return run_stage(s, [ins[1], ins[0]], weights, dtype, env)


@_mut()
def _down_pad01(s, ins, weights, dtype, env):
  w = O.W(weights, dtype, s.prefix)
  return O.conv2d(ins[0], w("kernel"), w("bias"), stride=2, pad=((0, 1), (0, 1)))


@_mut()
def _up_phases_transposed(s, ins, weights, dtype, env):
  y = run_stage(s, ins, weights, dtype, env)
  r, h2, w2, c = y.shape
  return y.reshape(r, h2 // 2, 2, w2 // 2, 2, c).transpose(2, 4).reshape(r, h2, w2, c)


@_mut()
def _ae_scale_c1(s, ins, weights, dtype, env):
  return ae_attn_restated(ins[0], _WZ(weights, dtype, s.prefix), scale_pow=-1.0)


# name -> (stage kinds, core?, fn).  Core mutants must clear GATES at every stage they apply to; the others are
# listed with their ratio to the gate.
MUTANTS = {
    "st: other row's context": (("st",), True, _st_other_context),
    "st: contribution x 1.05": (("st",), True, _gain),
    "st: scale from the padded head size": (("st",), False, _st_padded_scale),
    "st: LayerNorm 2 beta dropped": (("st",), False, _drop("block/layernorm2/beta")),
    "st: LayerNorm 3 beta dropped": (("st",), False, _drop("block/layernorm3/beta")),
    "st: proj_out bias dropped": (("st",), True, _drop("dense2/bias")),
    "st: cross-attention output bias dropped": (("st",), True, _drop("block/att_layer2/output/bias")),
    "st: FF-out bias dropped": (("st",), True, _drop("block/ffn/dense/bias")),
    "st: three zero keys appended": (("st",), False, _st_zero_keys),
    "st: GEGLU value/gate swapped in 64 rows": (("st",), False, _st_geglu_swap),
    "res: temb of the other row": (("res",), True, _res_other_temb),
    "res: temb slice of the following block": (("res",), False, _res_next_temb),
    "res: temb bias dropped": (("res",), True, _drop("dense/bias")),
    "res: shortcut bias dropped": (("res",), True, _drop("shortcut/bias")),
    "res: conv2 bias dropped": (("res",), True, _drop("conv2d_2/bias")),
    "res: second SiLU missing": (("res",), False, _res_no_second_silu),
    "structure: concat halves swapped": (("res",), True, _concat_swapped),
    "structure: downsample padded (0,1)": (("down",), True, _down_pad01),
    "structure: upsample phases transposed": (("up",), True, _up_phases_transposed),
    "ae: attention scale C^-1": (("ae_attn",), False, _ae_scale_c1),
    "ae: shortcut bias dropped": (("ae_res",), False, _drop("residual/shortcut/bias")),
}


def mutant_sizes(case, name, dtype):
  """{stage name: size of mutant `name` in figure units of storage type `dtype`} at the stages it applies to, each from
  the oracle's own taps rounded to `dtype` (the inputs the noise table uses)."""
  kinds, _, fn = MUTANTS[name]
  noise = noise_table(case, dtype)
  rounded = {k: v.to(dtype) for k, v in case["taps64"].items()}
  env = dict(case["env"], x=O._t(case["env"]["x"], dtype))
  out = {}
  for s in case["stages"]:
    if s.kind in kinds and fn.applies(s, case["weights"]):
      ref = local_ref(s, rounded, case["weights"], F64, env)
      out[s.name] = rel(local_ref(s, rounded, case["weights"], F64, env, fn=fn), ref) / max(noise[s.name], U[dtype])
  return out
