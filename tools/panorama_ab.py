#!/usr/bin/env python3
"""Same-process, interleaved A/B of panorama sampling at the C3 model (bf16 U-Net, f32 text encoder and autoencoder,
packaged plan tables, N=200).  Both arms put R = 32 rows of 32x32 through the U-Net per step:
arm A is txt2img at B=16 (the path and launches the sampler had before the panorama loop existed), arm P the panorama
at B=2 on a 32x144 canvas with 32x32 windows at stride 16 (8 windows per canvas).  Each arm has its own sampler and
captured graph; the models are shared.  Times are device time of graph replay per step (last_loop_ms_per_step) over
interleaved rounds, and the two window kernels alone at arm P's shape (events around `--kernel-iters` back-to-back
launches).  Writes profiles/panorama_ab_c3.json and prints the same JSON line.  A report, not a gate.

    python tools/panorama_ab.py [--steps 200] [--rounds 3] [--out profiles/panorama_ab_c3.json]
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
from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler  # noqa: E402
from ldm_tf2_amd.transformer import TransformerModel  # noqa: E402
from ldm_tf2_amd.unet import UNet  # noqa: E402

GS = 5.
A_BATCH, LATENT = 16, 32
P_BATCH, CANVAS, WINDOW, STRIDE = 2, (32, 144), (32, 32), (16, 16)


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
  ap.add_argument("--steps", type=int, default=200)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--kernel-iters", type=int, default=200)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_ab_c3.json"))
  ap.add_argument("--arm", choices=["A", "P"], default=None,
                  help="run one arm only: a warm-up loop and one timed loop (for a kernel trace), nothing is written")
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
  mk = lambda: LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **ldm)
  arms = {"A_txt2img": mk(), "P_panorama": mk()}
  ids = {"A_txt2img": BN.synthetic_token_ids(A_BATCH), "P_panorama": BN.synthetic_token_ids(P_BATCH)}

  def run(name):
    s = arms[name]
    if name == "A_txt2img":
      s.ddim_p_sample_loop(ids[name], [A_BATCH, LATENT, LATENT, 4], GS, seed=0)
    else:
      s.ddim_p_sample_loop_panorama(ids[name], [P_BATCH, *CANVAS, 4], WINDOW, STRIDE, GS, seed=0)
    return s.last_loop_ms_per_step()

  if args.arm:
    name = {"A": "A_txt2img", "P": "P_panorama"}[args.arm]
    run(name)
    print(json.dumps({name: round(run(name), 4)}))
    return
  for name in arms:
    run(name)                                   # warm-up + capture
  res = {name: [] for name in arms}
  for r in range(args.rounds):
    order = list(arms)
    if r % 2:
      order.reverse()
    for name in order:
      res[name].append(run(name))
  # the two kernels alone at arm P's shape (the window batch is the U-Net's float32 input)
  s = arms["P_panorama"]
  B, (H, W) = P_BATCH, CANVAS
  eps_canvas = s._eps.view(2, B, H, W, 4)
  kernels = dict(
      window_gather_us=time_kernel(lambda: ops.window_gather(s._xt, s._x_win, WINDOW, STRIDE), args.kernel_iters),
      window_fold_us=time_kernel(lambda: ops.window_fold(s._eps_win, eps_canvas, WINDOW, STRIDE), args.kernel_iters))
  out = dict(unet_dtype="bf16", ddim_steps=args.steps, guidance_scale=GS, rounds=args.rounds,
             rows_per_step=dict(A_txt2img=2 * A_BATCH, P_panorama=int(s._x_win.shape[0])),
             A_txt2img=dict(batch=A_BATCH, latent=LATENT),
             P_panorama=dict(batch=P_BATCH, canvas=list(CANVAS), window=list(WINDOW), stride=list(STRIDE),
                             windows_per_canvas=int(s._x_win.shape[0]) // (2 * P_BATCH)),
             kernels_standalone=kernels, arms={})
  for name, ms in res.items():
    out["arms"][name] = dict(ms_per_step=[round(x, 4) for x in ms], median_ms_per_step=round(float(np.median(ms)), 4),
                             min_ms_per_step=round(min(ms), 4), max_ms_per_step=round(max(ms), 4))
  a, p = out["arms"]["A_txt2img"], out["arms"]["P_panorama"]
  out["P_minus_A_ms_per_step"] = round(p["median_ms_per_step"] - a["median_ms_per_step"], 4)
  out["A_spread_ms_per_step"] = round(a["max_ms_per_step"] - a["min_ms_per_step"], 4)
  line = json.dumps(out)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  print(line)


if __name__ == "__main__":
  main()
