#!/usr/bin/env python3
"""Same-process, interleaved A/B of two-pass high-resolution sampling at the C5 model (bf16 U-Net, f32 text encoder and
autoencoder, packaged plan tables, B=4).  Arm A is txt2img at 64x64 latents from noise, N steps
(the only way to a 64x64 sample before the two-pass loop existed); arm H is ddim_p_sample_loop_hires: N steps at 32x32,
the resize, k = int(strength * N) steps at 64x64.  Each arm has its own sampler and captured graphs; the models are
shared.  Times are device time of graph replay over interleaved rounds: per step for arm A and for each pass of arm H
(last_loop_ms_per_step, last_hires_ms), and the whole denoising (all steps of all passes) per arm; the decode at 64x64
is the same launch sequence in both arms and is not in the loop times.  Also the resize launch alone at arm H's shape,
every mode (events around `--kernel-iters` back-to-back launches).  Writes profiles/hires_ab_c5.json and prints the
same JSON line.  A report, not a gate.

    python tools/hires_ab.py [--steps 50] [--strength 0.5] [--rounds 3] [--out profiles/hires_ab_c5.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as BN  # noqa: E402
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402
from ldm_tf2_amd.autoencoder import AutoencoderKL  # noqa: E402
from ldm_tf2_amd.model_runners import RESIZE_MODES, LatentDiffusionModelSampler, img2img_start  # noqa: E402
from ldm_tf2_amd.transformer import TransformerModel  # noqa: E402
from ldm_tf2_amd.unet import UNet  # noqa: E402

GS = 5.
LO, HI = 32, 64


def time_kernel(fn, iters):
  """Median over 5 repeats of (device time of `iters` back-to-back launches) / iters, in microseconds."""
  for _ in range(10):
    fn()
  out = []
  for _ in range(5):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
      fn()
    t1.record()
    t1.synchronize()
    out.append(t0.elapsed_time(t1) * 1000. / iters)
  return round(float(np.median(out)), 3)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=4)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--strength", type=float, default=0.5)
  ap.add_argument("--resize", default="bilinear", choices=RESIZE_MODES)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--kernel-iters", type=int, default=200)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hires_ab_c5.json"))
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  cfg = BN.FULL
  unet = UNet(**cfg["unet"], weights=Wt.init_weights(Wt.unet_manifest(**cfg["unet"]), seed=2, scope="unet"),
              dtype=torch.bfloat16, device=dev)
  txt = TransformerModel(**cfg["cond_stage_model"], dtype=torch.float32, device=dev,
                         weights=Wt.init_weights(Wt.transformer_manifest(**cfg["cond_stage_model"]), seed=2,
                                                 scope="cond_stage_model"))
  ae = AutoencoderKL(**cfg["autoencoder_kl"], dtype=torch.float32, device=dev,
                     weights=Wt.init_weights(Wt.decoder_manifest(**cfg["autoencoder_kl"]), seed=2, scope="autoencoder"))
  ldm = dict(cfg["ldm"], num_ddim_steps=args.steps)
  B, n = args.batch, args.steps
  k = img2img_start(args.strength, n)
  s_a = LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **ldm)
  s_h = LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **ldm)
  ids = BN.synthetic_token_ids(B)

  def run_a():
    s_a.ddim_p_sample_loop(ids, [B, HI, HI, 4], GS, seed=0)
    per_step = s_a.last_loop_ms_per_step()
    return dict(loop_ms=per_step * n, ms_per_step=per_step)

  def run_h():
    s_h.ddim_p_sample_loop_hires(ids, [B, LO, LO, 4], [B, HI, HI, 4], strength=args.strength, resize=args.resize,
                                 guidance_scale=GS, seed=0)
    p1, p2 = s_h.last_hires_ms()
    return dict(loop_ms=p1 + p2, pass1_ms_per_step=p1 / n, pass2_ms_per_step=p2 / k)

  arms = {"A_txt2img_64": run_a, "H_hires_32_64": run_h}
  for fn in arms.values():
    fn()                                        # warm-up + capture
  graphs = (s_h._graph, s_h._states[(B, LO, LO, 4)]["_graph"])
  res = {name: [] for name in arms}
  for r in range(args.rounds):
    order = list(arms)
    if r % 2:
      order.reverse()
    for name in order:
      res[name].append(arms[name]())
  assert (s_h._graph, s_h._states[(B, LO, LO, 4)]["_graph"]) == graphs        # captured once, both shapes
  lat = s_h.hires_first_latents
  out_hi = torch.empty(B, HI, HI, 4, device=dev)
  kernels = {f"resize_{mode}_us": time_kernel(lambda: ops.resize_nhwc(lat, (HI, HI), mode, out=out_hi),
                                              args.kernel_iters) for mode in RESIZE_MODES}
  out = dict(unet_dtype="bf16", batch=B, ddim_steps=n, strength=args.strength, pass2_steps=k, resize=args.resize,
             guidance_scale=GS, rounds=args.rounds,
             plan_table_entries={str(L): len(ops.gemm_plans(2 * B, L, "bf16")) for L in (LO, HI)},
             kernels_standalone=kernels, arms={})
  for name, runs in res.items():
    arm = {}
    for key in runs[0]:
      v = [r[key] for r in runs]
      arm[key] = dict(runs=[round(x, 4) for x in v], median=round(float(np.median(v)), 4), min=round(min(v), 4),
                      max=round(max(v), 4))
    out["arms"][name] = arm
  a, h = out["arms"]["A_txt2img_64"]["loop_ms"], out["arms"]["H_hires_32_64"]["loop_ms"]
  out["H_over_A_loop_time"] = round(h["median"] / a["median"], 4)
  out["A_spread_loop_ms"] = round(a["max"] - a["min"], 4)
  line = json.dumps(out)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  print(line)


if __name__ == "__main__":
  main()
