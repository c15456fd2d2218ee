#!/usr/bin/env python3
"""Same-process, interleaved A/B of the two noise sources at the C3 shape (bf16 U-Net, f32 text
encoder and autoencoder, B=16, 32x32 latents, N=200): eta = 1 img2img at strength 1.0 with a half mask, so both the
eta noise and the blend's Q are in every step.  noise_source="host" builds and uploads two [N,B,h,w,c] tables before
the loop; "device" draws the same kind of numbers inside the update launch.  Per source: ms per CFG U-Net step from
last_loop_ms_per_step (graph replay, device time), the wall time of the whole pass (text encoder, image encoder,
set-up, loop, decode) and of the set-up alone (whole pass minus the loop's device time).  A report, not a gate.

    python tools/noise_ab.py [--batch 16] [--latent 32] [--steps 200] [--rounds 3]
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
from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler  # noqa: E402
from ldm_tf2_amd.transformer import TransformerModel  # noqa: E402
from ldm_tf2_amd.unet import UNet  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--latent", type=int, default=32)
  ap.add_argument("--steps", type=int, default=200)
  ap.add_argument("--rounds", type=int, default=3)
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  cfg = BN.FULL
  ae_man = Wt.decoder_manifest(**cfg["autoencoder_kl"])
  ae_man.update(Wt.encoder_manifest(**cfg["autoencoder_kl"], image_size=8 * args.latent, double_z=True))
  unet = UNet(**cfg["unet"], weights=Wt.init_weights(Wt.unet_manifest(**cfg["unet"]), seed=2, scope="unet"),
              dtype=torch.bfloat16, device=dev)
  txt = TransformerModel(**cfg["cond_stage_model"], dtype=torch.float32, device=dev,
                         weights=Wt.init_weights(Wt.transformer_manifest(**cfg["cond_stage_model"]), seed=2,
                                                 scope="cond_stage_model"))
  ae = AutoencoderKL(**cfg["autoencoder_kl"], weights=Wt.init_weights(ae_man, seed=2, scope="autoencoder"),
                     dtype=torch.float32, device=dev)
  ldm = dict(cfg["ldm"], num_ddim_steps=args.steps, eta=1.)
  # one sampler per source: each keeps its own captured graph (the U-Net's buffers are shared, replays are sequential)
  pair = {name: LatentDiffusionModelSampler(unet, ae, txt, verbose=False, noise_source=name, **ldm)
          for name in ("host", "device")}
  B, L = args.batch, args.latent
  ids = BN.synthetic_token_ids(B)
  images = (np.random.default_rng(0).random((B, 8 * L, 8 * L, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
  mask = np.zeros((B, L, L), np.float32)
  mask[:, :, : L // 2] = 1.

  def run(name, seed):
    s = pair[name]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = s.ddim_p_sample_loop_img2img(ids, images, 5., strength=1.0, mask=mask, seed=seed)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    assert bool(torch.isfinite(out.float()).all()), "non-finite images"
    step = s.last_loop_ms_per_step()
    return step, wall, wall - step * args.steps

  for name in pair:
    run(name, 0)                                # warm-up + capture
  res = {name: [] for name in pair}
  for r in range(args.rounds):
    order = list(pair)
    if r % 2:
      order.reverse()
    for name in order:
      res[name].append(run(name, r + 1))        # a new seed every round: the same graph
  col = lambda name, i: [round(x[i], 4) for x in res[name]]
  med = lambda name, i: round(float(np.median([x[i] for x in res[name]])), 4)
  out = dict(batch=B, latent=L, ddim_steps=args.steps, unet_dtype="bf16", eta=1.0, mask="half",
             ms_per_step={k: col(k, 0) for k in res}, median_ms_per_step={k: med(k, 0) for k in res},
             device_over_host=round(med("device", 0) / med("host", 0) - 1, 5),
             whole_pass_ms={k: col(k, 1) for k in res}, median_whole_pass_ms={k: med(k, 1) for k in res},
             setup_ms={k: col(k, 2) for k in res}, median_setup_ms={k: med(k, 2) for k in res},
             table_mbytes_host=round(2 * args.steps * B * L * L * 4 * 4 / 2 ** 20, 1),
             note="setup = whole pass - loop device time: text and image encoders, noise set-up, decode")
  print(json.dumps(out))


if __name__ == "__main__":
  main()
