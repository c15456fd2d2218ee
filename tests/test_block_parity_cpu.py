"""The stage-local reference of tests/block_ref.py, checked without a GPU.

  * the stage walk chained in float64 and float32 IS the oracle (bit for bit), and so are the restated stages the
    mutants are built from;
  * the calibrated inputs meet their condition (every attention layer: float64 logit standard deviation in [2, 4],
    mean largest probability above 0.1);
  * the noise table (what the oracle itself loses per stage in float32 / bf16) and the mutant table (the size of every
    planted host-level error in figure units, per stage it applies to) are printed (pytest -s);
  * every CORE mutant clears the gate recorded in block_ref.GATES at every stage it applies to -- the share left
    undetected is 0; every other mutant is listed with its ratio to the gate, above or below;
  * the gap that is the reason for the module: with test_models_gpu.py's own inputs the wrong-context and the gain
    mutant stay under that module's bf16 gate at the whole output, at every transformer block.
"""
import numpy as np
import pytest
import torch

import block_ref as BR
from ldm_tf2_amd import weights as Wt
from oracle import ldm_oracle as O

F64, F32, BF16 = BR.F64, BR.F32, BR.BF16
UNETS = ["A", "B"]
AES = ["kl-dec", "kl-full-dec", "kl-full-enc"]


def _case(model):
  return BR.unet_case(model) if model in UNETS else BR.ae_case(model)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("model", UNETS + AES)
def test_the_walk_is_the_oracle(model, dtype):
  c = _case(model)
  env, w = c["env"], c["weights"]
  with torch.no_grad():
    if model in UNETS:
      otaps = {}
      ref = O.unet_forward(env["x"], env["t"], env["ctx"], w, dtype=dtype, num_heads=BR.HEADS, taps=otaps)
    elif model.endswith("dec"):
      ref = O.decoder_forward(env["x"], w, dtype=dtype)
    else:
      ref = O.encoder_forward(env["x"], w, dtype=dtype)
  taps = BR.walk(c["stages"], w, dtype, env)
  assert [s.name for s in c["stages"]] == list(taps)
  assert torch.equal(taps["out"], ref)
  if model in UNETS:
    # the oracle's own per-block taps are the last stage of each block
    last = {}
    for s in c["stages"]:
      if "/" in s.name:
        blk = s.name.rsplit("/", 1)[0]
        last[blk] = s.name
    last["middle_block"] = "middle_block/residual2"
    assert set(otaps) == set(last)
    for blk, t in otaps.items():
      assert torch.equal(taps[last[blk]], t), blk
    # each output block's ResBlock reads concat(previous, popped skip): the skips are popped in reverse
    cat = [s for s in c["stages"] if len(s.inputs) == 2]
    assert len(cat) == len([b for b in otaps if b.startswith("output_blocks/")]) and cat[-1].inputs[1] == "conv_in"
    assert cat[0].inputs == ("middle_block/residual2", last[f"input_blocks/{len(cat) - 2}"])


@pytest.mark.parametrize("model", UNETS)
def test_the_restated_stages_are_the_oracle(model):
  """st_restated / res_restated without their hooks, and local_ref on the oracle's own taps, reproduce the walk."""
  c = BR.unet_case(model)
  w, env, taps = c["weights"], c["env"], c["taps64"]
  with torch.no_grad():
    for s in c["stages"]:
      ins = BR.stage_inputs(s, taps, F64, env)
      assert torch.equal(BR.local_ref(s, taps, w, F64, env), taps[s.name]), s.name
      if s.kind == "st":
        assert torch.equal(BR.st_restated(ins[0], env["ctx"].double(), O.W(w, F64, s.prefix), BR.HEADS), taps[s.name])
      if s.kind == "res":
        te = BR._own_te(s, w, F64, env)
        assert torch.equal(BR.res_restated(BR._res_x(ins), te, O.W(w, F64, s.prefix)), taps[s.name])
  # the temb stage holds each ResBlock's projection at its offset
  tall = taps["temb"]
  assert tall.shape[1] == sum(cc for _, _, cc in c["slices"])
  for p, o, cc in c["slices"]:
    assert torch.equal(tall[:, o:o + cc], BR._own_te(BR.Stage("", "res", p, []), w, F64, env))


def test_the_restated_ae_attention_is_the_oracle():
  c = BR.ae_case("kl-dec")
  s = next(s for s in c["stages"] if s.kind == "ae_attn")
  ins = BR.stage_inputs(s, c["taps64"], F64, c["env"])
  with torch.no_grad():
    assert torch.equal(BR.ae_attn_restated(ins[0], O.W(c["weights"], F64, s.prefix)), c["taps64"][s.name])


@pytest.mark.parametrize("model", UNETS + AES)
def test_calibrated_attention_is_not_a_uniform_average(model):
  c = _case(model)
  raw = BR.attention_stats(c["stages"], c["raw_weights"], c["env"])
  cal = BR.attention_stats(c["stages"], c["weights"], c["env"])
  assert len(cal) == (2 * sum(s.kind == "st" for s in c["stages"]) if model in UNETS else 1)
  for (p, _, sd0, mx0), (_, _, sd, mx) in zip(raw, cal):
    print(f"{model} {p:58s} random init: logit std {sd0:6.3f} max p {mx0:.4f}   calibrated: std {sd:5.2f} max p {mx:.3f}")
    assert 2.0 <= sd <= 4.0 and mx > 0.1, (p, sd, mx)
  if model in UNETS:
    # the premise: at random init a self-attention row is a near-uniform average (the cross-attention's logits grow
    # with the context's scale, 4 here)
    assert max(sd0 for p, _, sd0, _ in raw if p.endswith("att_layer1/")) < 0.5
    env = c["env"]
    assert len(set(env["t"][:2].tolist())) == 2 and np.array_equal(env["t"][:2], env["t"][2:])
    assert torch.equal(env["x"][:2], env["x"][2:]) and 3.5 < float(env["ctx"].std()) < 4.5


@pytest.mark.parametrize("model", UNETS + AES)
def test_noise_table(model):
  """What the oracle itself loses on each stage, from exact (rounded) inputs: the unit of a figure."""
  c = _case(model)
  n32, n16 = BR.noise_table(c, F32), BR.noise_table(c, BF16)
  for s in c["stages"]:
    print(f"noise {model:12s} {s.name:42s} {s.kind:11s} f32 {n32[s.name]:.2e}  bf16 {n16[s.name]:.2e}")
    assert 0 < n32[s.name] < 1e-5 and 2.0 ** -10 < n16[s.name] < 5e-2, s.name
    assert n16[s.name] > 100 * n32[s.name]


def test_gates_are_twice_the_measured_figures():
  """GATES = 2 x the largest figure of the first MI355X run per stage kind and storage type, rounded up to one
  significant digit."""
  import math
  worst = {}
  for (model, tag), kinds in BR.MEASURED.items():
    for kind, f in kinds.items():
      worst[kind, tag] = max(worst.get((kind, tag), 0.0), f)
  assert {k for k, _ in worst} == set(BR.GATES)
  for (kind, tag), f in sorted(worst.items()):
    e = 10.0 ** math.floor(math.log10(2 * f))
    want = math.ceil(2 * f / e - 1e-9) * e
    print(f"gate {kind:11s} {tag:4s} largest figure {f:8.4f} -> gate {want:g}")
    assert math.isclose(BR.GATES[kind][tag], want, rel_tol=1e-9), (kind, tag, BR.GATES[kind][tag], want)


def _gate(kind, dtype):
  return BR.GATES.get(BR.gate_kind(kind), {}).get(BR.TAG[dtype])


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_mutant_table(dtype):
  """Every mutant at every stage it applies to, in figure units of `dtype` and as a ratio to the stage kind's gate.
  Core mutants must clear the gate everywhere; the rest are listed whichever side they fall on."""
  missed, listed = [], 0
  for name, (kinds, core, fn) in BR.MUTANTS.items():
    for model in (AES if name.startswith("ae:") else UNETS):
      c = _case(model)
      sizes = BR.mutant_sizes(c, name, dtype)
      if not sizes:
        print(f"mutant {name:42s} {model:12s} applies to no stage of this model")
        continue
      kind = next(s.kind for s in c["stages"] if s.name in sizes)
      gate = _gate(kind, dtype)
      lo, hi = min(sizes.values()), max(sizes.values())
      where = min(sizes, key=sizes.get)
      ratio = "gate unmeasured" if gate is None else f"{lo / gate:7.2f} .. {hi / gate:8.2f} x gate {gate:g}"
      note = ""
      if "zero keys" in name:
        note = "  (below the noise by construction: tests/test_attention_accounting_gpu.py accounts for every key exactly)"
      print(f"mutant {'CORE ' if core else '     '}{name:42s} {model:12s} {BR.TAG[dtype]:4s} {len(sizes):2d} stages "
            f"size {lo:8.2f} .. {hi:9.2f}  {ratio}  smallest at {where}{note}")
      listed += 1
      if core and gate is None:
        missed.append((name, model, f"no gate recorded for stage kind {kind}"))
      elif core:
        missed += [(name, model, st, round(v, 2), gate) for st, v in sizes.items() if not v > gate]
  assert listed >= len(BR.MUTANTS)
  assert not missed, f"core mutants under their gate (share undetected must be 0): {missed}"


def test_mutants_at_the_whole_output():
  """Each U-Net mutant planted at ONE stage (the middle one of those it applies to) and carried to the model's
  output (model B, calibrated inputs, float64), relative to the whole-output gates of test_models_gpu.py."""
  from test_models_gpu import REL
  c = BR.unet_case("B")
  ref = c["taps64"]["out"]
  for name, (kinds, core, fn) in BR.MUTANTS.items():
    if name.startswith("ae:"):
      continue
    st = [s for s in c["stages"] if s.kind in kinds and fn.applies(s, c["weights"])]
    s = st[len(st) // 2]
    out = BR.walk(c["stages"], c["weights"], F64, c["env"], mutate={s.name: fn}, base=c["taps64"])["out"]
    r = BR.rel(out, ref)
    print(f"whole output {name:42s} at {s.name:36s} rel {r:.2e} = {r / REL[BF16]:6.3f} x the bf16 gate, "
          f"{r / REL[F32]:9.1f} x the float32 gate")
    assert np.isfinite(r)


def test_the_gap_the_whole_output_gate_leaves():
  """test_models_gpu.py's model, weights and inputs: a transformer block that reads the other row's context, or whose
  contribution is scaled by 1.05, changes the final output by less than that module's bf16 gate -- at every block."""
  from test_models_gpu import CTX_DIM, REL, UNET_CFG, _inputs
  w = Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **UNET_CFG), seed=2, mode="random", scope="unet")
  x, ctx = _inputs()
  t = np.array([981, 981, 21, 500], dtype=np.int32)
  stages = BR.unet_stages(w)
  env = dict(x=torch.from_numpy(x), t=t, ctx=torch.from_numpy(ctx))
  base = BR.walk(stages, w, F64, env)
  with torch.no_grad():
    assert torch.equal(base["out"], O.unet_forward(x, t, ctx, w, dtype=F64))
  worst = {}
  for name in ("st: other row's context", "st: contribution x 1.05"):
    fn = BR.MUTANTS[name][2]
    for s in stages:
      if s.kind == "st":
        r = BR.rel(BR.walk(stages, w, F64, env, mutate={s.name: fn}, base=base)["out"], base["out"])
        print(f"gap {name:28s} at {s.name:36s} whole-output rel {r:.2e} ({r / REL[BF16]:.2f} x the bf16 gate)")
        worst[name] = max(worst.get(name, 0.0), r)
        assert 0 < r < REL[BF16], (name, s.name, r)
  print("gap: largest", {k: f"{v:.2e}" for k, v in worst.items()}, "under the bf16 gate", REL[BF16])
