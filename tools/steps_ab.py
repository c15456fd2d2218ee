#!/usr/bin/env python3
"""Same-process, interleaved A/B of the sampling step at the C3 shape (bf16 U-Net, f32 text encoder and autoencoder,
B=16, 32x32 latents) with sampler="plms" against sampler="deis" on one step table, each as ms
per CFG U-Net step from last_loop_ms_per_step (graph replay, device time).  Then, once, whole passes (text encoder,
loop, decode) as images/s for `deis` at each --short-steps N.  A report, not a gate; it says nothing about image
quality at a given N.

    python tools/steps_ab.py [--batch 16] [--latent 32] [--steps 200] [--spacing karras] [--rounds 3]
                             [--short-steps 20 25 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402
from ldm_tf2_amd.autoencoder import AutoencoderKL  # noqa: E402
from ldm_tf2_amd.model_runners import STEP_SPACINGS, LatentDiffusionModelSampler  # noqa: E402
from ldm_tf2_amd.transformer import TransformerModel  # noqa: E402
from ldm_tf2_amd.unet import UNet  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--latent", type=int, default=32)
  ap.add_argument("--steps", type=int, default=200)
  ap.add_argument("--spacing", default="karras", choices=STEP_SPACINGS)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--short-steps", type=int, nargs="*", default=[20, 25, 50])
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
  B, L = args.batch, args.latent
  ids = BN.synthetic_token_ids(B)

  def sampler(name, n):
    # one sampler per form: each keeps its own captured graph (the U-Net's buffers are shared, replays are sequential)
    return LatentDiffusionModelSampler(unet, ae, txt, verbose=False, sampler=name, step_spacing=args.spacing,
                                       **dict(cfg["ldm"], num_ddim_steps=n))

  def run(s):
    images = s.ddim_p_sample_loop(ids, [B, L, L, 4], 5., seed=0)
    assert bool(torch.isfinite(images.float()).all()), "non-finite images"
    return s.last_loop_ms_per_step()

  pair = {name: sampler(name, args.steps) for name in ("plms", "deis")}
  for s in pair.values():
    run(s)                                      # warm-up + capture
  res = {name: [] for name in pair}
  for r in range(args.rounds):
    order = list(pair)
    if r % 2:
      order.reverse()
    for name in order:
      res[name].append(run(pair[name]))
  med = {k: float(np.median(v)) for k, v in res.items()}

  def images_per_s(s):
    run(s)                                      # warm-up + capture
    torch.cuda.synchronize()
    t = []
    for _ in range(args.rounds):
      t0 = time.perf_counter()
      run(s)
      torch.cuda.synchronize()
      t.append(time.perf_counter() - t0)
    return B / float(np.median(t))

  rate = {f"deis_N{n}": images_per_s(sampler("deis", n)) for n in args.short_steps}
  out = dict(batch=B, latent=L, ddim_steps=args.steps, step_spacing=args.spacing, unet_dtype="bf16",
             ms_per_step={k: [round(x, 4) for x in v] for k, v in res.items()},
             median_ms_per_step={k: round(v, 4) for k, v in med.items()},
             deis_over_plms=round(med["deis"] / med["plms"] - 1, 5),
             images_per_s={k: round(v, 3) for k, v in rate.items()},
             note="images/s = whole passes (text encoder + loop + decode); quality at a given N is not measured")
  print(json.dumps(out))


if __name__ == "__main__":
  main()
