#!/usr/bin/env python3
"""Same-process, interleaved A/B of the DDIM step at the C3 shape (bf16 U-Net, f32 text encoder and
autoencoder, B=16, 32x32 latents, N=200): txt2img against img2img at strength 1.0 with a half mask (the
masked CFG+DDIM update), each as ms per U-Net step from last_loop_ms_per_step (graph
replay, device time).  Also reports the KL encoder's time for B images at 8*latent squared.  A report,
not a gate.

    python tools/img2img_ab.py [--batch 16] [--latent 32] [--steps 200] [--rounds 3]
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
  ldm = dict(cfg["ldm"], num_ddim_steps=args.steps)
  # one sampler per form: each keeps its own captured graph (the U-Net's buffers are shared, replays are sequential)
  s_txt = LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **ldm)
  s_img = LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **ldm)
  B, L = args.batch, args.latent
  ids = BN.synthetic_token_ids(B)
  g = np.random.default_rng(0)
  images = (g.random((B, 8 * L, 8 * L, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
  mask = np.zeros((B, L, L), np.float32)
  mask[:, :, : L // 2] = 1.
  q_noises = g.standard_normal((args.steps, B, L, L, 4), dtype=np.float32)
  enc_noise = g.standard_normal((B, L, L, 4), dtype=np.float32)

  def run_txt():
    s_txt.ddim_p_sample_loop(ids, [B, L, L, 4], 5., seed=0)
    return s_txt.last_loop_ms_per_step()

  def run_img():
    s_img.ddim_p_sample_loop_img2img(ids, images, 5., strength=1.0, mask=mask, encode_noise=enc_noise,
                                     q_noises=q_noises)
    return s_img.last_loop_ms_per_step()

  run_txt()
  run_img()                                     # warm-up + capture
  res = {"txt2img": [], "img2img_masked": []}
  for r in range(args.rounds):
    order = [("txt2img", run_txt), ("img2img_masked", run_img)]
    if r % 2:
      order.reverse()
    for name, fn in order:
      res[name].append(fn())
  # the encoder alone: images -> moments, B images at 8L x 8L
  x = torch.from_numpy(images).to(dev)
  ae.encode(x)
  torch.cuda.synchronize()
  enc_ms = []
  for _ in range(args.rounds):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    ae.encode(x)
    t1.record()
    t1.synchronize()
    enc_ms.append(t0.elapsed_time(t1))
  med = {k: float(np.median(v)) for k, v in res.items()}
  out = dict(batch=B, latent=L, ddim_steps=args.steps, unet_dtype="bf16",
             ms_per_step={k: [round(x, 4) for x in v] for k, v in res.items()},
             median_ms_per_step={k: round(v, 4) for k, v in med.items()},
             masked_over_txt2img=round(med["img2img_masked"] / med["txt2img"] - 1, 5),
             encoder_ms=round(float(np.median(enc_ms)), 3), encoder_images=f"{B}x{8 * L}x{8 * L}")
  print(json.dumps(out))


if __name__ == "__main__":
  main()
