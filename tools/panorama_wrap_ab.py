#!/usr/bin/env python3
"""Same-process, interleaved A/B of seamless panorama sampling at the C3 model (bf16 U-Net, f32 text encoder and
autoencoder, packaged plan tables, N=200).  Both arms put R = 32 rows of 32x32 through the U-Net
per step, 8 windows per canvas: arm P is section 12's panorama at B=2 on a 32x144 canvas with 32x32 windows at stride
16 (clamped grid, plain mean: ldm_window_gather / ldm_window_fold), arm W the same window and stride on a 32x128
canvas wrapped along x with tent weights (ldm_window_gather_ex / ldm_window_fold_ex).  Each arm has its own sampler
and captured graph; the models are shared.  Times are device time of graph replay per step (last_loop_ms_per_step)
over interleaved rounds, and the two _ex kernels alone at arm W's shape (events around `--kernel-iters` back-to-back
launches).  Writes profiles/panorama_wrap_ab_c3.json and prints the same JSON line.  A report, not a gate.

    python tools/panorama_wrap_ab.py [--steps 200] [--rounds 3] [--out profiles/panorama_wrap_ab_c3.json]
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
BATCH, WINDOW, STRIDE = 2, (32, 32), (16, 16)
P_CANVAS = (32, 144)
W_CANVAS, WRAP, WEIGHTS = (32, 128), (False, True), "tent"


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
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_wrap_ab_c3.json"))
  ap.add_argument("--arm", choices=["P", "W"], default=None,
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
  arms = {"P_panorama": mk(), "W_wrapped_tent": mk()}
  ids = BN.synthetic_token_ids(BATCH)

  def run(name):
    s = arms[name]
    if name == "P_panorama":
      s.ddim_p_sample_loop_panorama(ids, [BATCH, *P_CANVAS, 4], WINDOW, STRIDE, GS, seed=0)
    else:
      s.ddim_p_sample_loop_panorama(ids, [BATCH, *W_CANVAS, 4], WINDOW, STRIDE, GS, seed=0, wrap=WRAP,
                                    window_weights=WEIGHTS)
    return s.last_loop_ms_per_step()

  if args.arm:
    name = {"P": "P_panorama", "W": "W_wrapped_tent"}[args.arm]
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
  # the two kernels alone at arm W's shape (the window batch is the U-Net's float32 input)
  s = arms["W_wrapped_tent"]
  H, W = W_CANVAS
  eps_canvas = s._eps.view(2, BATCH, H, W, 4)
  weights = (s._win_wy, s._win_wx)
  kernels = dict(
      window_gather_ex_us=time_kernel(lambda: ops.window_gather_ex(s._xt, s._x_win, WINDOW, STRIDE, WRAP),
                                      args.kernel_iters),
      window_fold_ex_us=time_kernel(lambda: ops.window_fold_ex(s._eps_win, eps_canvas, WINDOW, STRIDE, WRAP, weights),
                                    args.kernel_iters))
  rows = {name: int(a._x_win.shape[0]) for name, a in arms.items()}
  out = dict(unet_dtype="bf16", ddim_steps=args.steps, guidance_scale=GS, rounds=args.rounds, rows_per_step=rows,
             P_panorama=dict(batch=BATCH, canvas=list(P_CANVAS), window=list(WINDOW), stride=list(STRIDE),
                             windows_per_canvas=rows["P_panorama"] // (2 * BATCH)),
             W_wrapped_tent=dict(batch=BATCH, canvas=list(W_CANVAS), window=list(WINDOW), stride=list(STRIDE),
                                 wrap=list(WRAP), window_weights=WEIGHTS,
                                 windows_per_canvas=rows["W_wrapped_tent"] // (2 * BATCH)),
             kernels_standalone=kernels, arms={})
  for name, ms in res.items():
    out["arms"][name] = dict(ms_per_step=[round(x, 4) for x in ms], median_ms_per_step=round(float(np.median(ms)), 4),
                             min_ms_per_step=round(min(ms), 4), max_ms_per_step=round(max(ms), 4))
  p, w = out["arms"]["P_panorama"], out["arms"]["W_wrapped_tent"]
  out["W_minus_P_ms_per_step"] = round(w["median_ms_per_step"] - p["median_ms_per_step"], 4)
  out["P_spread_ms_per_step"] = round(p["max_ms_per_step"] - p["min_ms_per_step"], 4)
  line = json.dumps(out)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  print(line)


if __name__ == "__main__":
  main()
