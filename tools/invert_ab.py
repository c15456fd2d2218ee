#!/usr/bin/env python3
"""Same-process, interleaved timing of DDIM inversion at the C3 shape (bf16 U-Net, f32 text encoder and autoencoder,
B=16, 32x32 latents, N=200).  Three arms on one sampler, each with its captured graph: the
conditional-only inversion step (guidance scale 1: the U-Net on B rows), the guided inversion step (scale 3: 2B rows)
and the sampling step (scale 5, started from the inverted latents).  Times are device time of graph replay, ms per step
(last_loop_ms_per_step).  Then the reconstruction error of invert -> sample, both at scale 1 and full depth, at N = 50
and N = 200: relative L2 of the returned latents against z0.  The weights are random, so the error says what the
arithmetic and the U-Net's Lipschitz constant make of the round trip, not what a trained model reaches.  Prints one
JSON line.  A report, not a gate.

    python tools/invert_ab.py [--batch 16] [--latent 32] [--steps 200] [--rounds 3]
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

GS, GS_INVERT = 5., 3.


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
  B, L, N = args.batch, args.latent, args.steps
  ids = BN.synthetic_token_ids(B)
  shape = [B, L, L, 4]
  z0 = (0.8 * np.random.default_rng(0).standard_normal(shape)).astype(np.float32)
  mk = lambda n: LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **dict(cfg["ldm"], num_ddim_steps=n))
  s = mk(N)
  state = {}

  def run(name):
    if name == "invert_cond_only":
      state["x"] = s.ddim_invert_loop(ids, latents=z0, guidance_scale=1.)
    elif name == "invert_guided":
      s.ddim_invert_loop(ids, latents=z0, guidance_scale=GS_INVERT)
    else:
      s.ddim_p_sample_loop(ids, shape, GS, x_T=state["x"], start_index=N)
    return s.last_loop_ms_per_step()

  arms = ("invert_cond_only", "invert_guided", "sampling")
  for name in arms:
    run(name)                                   # warm-up + capture
  res = {name: [] for name in arms}
  for r in range(args.rounds):
    for name in (arms if r % 2 == 0 else arms[::-1]):
      res[name].append(run(name))
  out = dict(batch=B, latent=L, ddim_steps=N, unet_dtype="bf16", guidance_scale=GS, invert_guidance_scale=GS_INVERT,
             rounds=args.rounds, arms={}, reconstruction={})
  for name, ms in res.items():
    out["arms"][name] = dict(ms_per_step=[round(x, 4) for x in ms], median_ms_per_step=round(float(np.median(ms)), 4))
  a = out["arms"]
  out["cond_only_over_sampling"] = round(a["invert_cond_only"]["median_ms_per_step"] /
                                         a["sampling"]["median_ms_per_step"], 4)
  z = torch.from_numpy(z0).to(dev)
  for n in (50, 200):
    r = s if n == N else mk(n)
    x = r.ddim_invert_loop(ids, latents=z0, guidance_scale=1.)
    r.ddim_p_sample_loop(ids, shape, 1., x_T=x, start_index=n)
    out["reconstruction"][str(n)] = dict(
        rel_l2=round(float((r._xt - z).norm() / z.norm()), 6),
        inverted_rms=round(float(x.pow(2).mean().sqrt()), 4))
  print(json.dumps(out))


if __name__ == "__main__":
  main()
