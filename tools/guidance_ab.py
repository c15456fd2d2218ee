#!/usr/bin/env python3
"""Same-process, interleaved A/B of guidance schedules at the C3 shape (bf16 U-Net, f32 text encoder and autoencoder,
B=16, 32x32 latents, N=200).  Arm A is the constant-guidance loop (a float scale, no interval:
the path and launches the sampler had before schedules existed).  The other arms run guidance_interval= over the
middle of the step table so that 100 %, 50 % and 25 % of the steps are guided, each with skip_unguided=True (unguided
steps evaluate the U-Net on the B conditional rows) and False (all 2B rows, only the table is used).  Every arm has
its own sampler and captured graphs; the models are shared.  Times are device time of graph replay: ms per step of
the loop (last_loop_ms_per_step) and per form (last_form_ms_per_step).  Prints one JSON line.  A report, not a gate.

    python tools/guidance_ab.py [--batch 16] [--latent 32] [--steps 200] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402
from ldm_tf2_amd.autoencoder import AutoencoderKL  # noqa: E402
from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler  # noqa: E402
from ldm_tf2_amd.transformer import TransformerModel  # noqa: E402
from ldm_tf2_amd.unet import UNet  # noqa: E402

GS = 5.


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--latent", type=int, default=32)
  ap.add_argument("--steps", type=int, default=200)
  ap.add_argument("--rounds", type=int, default=3)
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
  B, L, N = args.batch, args.latent, args.steps
  ids = BN.synthetic_token_ids(B)
  shape = [B, L, L, 4]
  mk = lambda **kw: LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **kw, **ldm)
  arms = {"A_constant": (mk(), {})}
  steps = arms["A_constant"][0]._ddim_steps
  for pct in (100, 50, 25):
    n_g = N * pct // 100
    lo = (N - n_g) // 2
    iv = (int(steps[lo]), int(steps[lo + n_g - 1]))
    for skip in (True, False):
      arms[f"guided{pct}_{'skip' if skip else 'noskip'}"] = (mk(skip_unguided=skip), dict(guidance_interval=iv))

  def run(name):
    s, kw = arms[name]
    s.ddim_p_sample_loop(ids, shape, GS, seed=0, **kw)
    ms = s.last_loop_ms_per_step()
    forms = s.last_form_ms_per_step() if kw else dict(guided=ms, unguided=None)
    return ms, forms

  for name in arms:
    run(name)                                   # warm-up + capture
  res = {name: [] for name in arms}
  for r in range(args.rounds):
    order = list(arms)
    if r % 2:
      order.reverse()
    for name in order:
      res[name].append(run(name))
  med = lambda v: None if any(x is None for x in v) else round(float(np.median(v)), 4)
  out = dict(batch=B, latent=L, ddim_steps=N, unet_dtype="bf16", guidance_scale=GS, rounds=args.rounds, arms={})
  for name, runs in res.items():
    ms = [r[0] for r in runs]
    out["arms"][name] = dict(
        ms_per_step=[round(x, 4) for x in ms], median_ms_per_step=med(ms),
        guided_ms_per_step=med([r[1]["guided"] for r in runs]),
        unguided_ms_per_step=med([r[1]["unguided"] for r in runs]),
        loop_images_per_s=round(B / (float(np.median(ms)) * N / 1000.), 3))
  a = out["arms"]
  out["unguided_over_guided"] = round(a["guided50_skip"]["unguided_ms_per_step"] / a["guided50_skip"]["guided_ms_per_step"], 4)
  print(json.dumps(out))


if __name__ == "__main__":
  main()
