#!/usr/bin/env python3
"""Same-process, interleaved A/B of the txt2img loop at the benchmark's model (f32 text encoder and autoencoder, 32x32
latents) for the cross-attention heat maps, as ms per U-Net step from last_loop_ms_per_step
(graph replay, device time):

    off           the loop without attn_maps: the parent commit's graph key, launches and replayed graph
    on            attn_maps=True for all 16 transformer blocks: one ldm_xattn_map launch per block on the conditional
                  rows, and no block in the ldm_st_block form
    off_no_block  the loop without attn_maps on a U-Net built with fused_block=False: what leaving ldm_st_block
                  alone costs, so that (on - off_no_block) is the map launches themselves

    python tools/attn_maps_ab.py [--dtype bf16] [--batch 16] [--latent 32] [--steps 50] [--rounds 3]

A report, not a gate.
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
  ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--latent", type=int, default=32)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--rounds", type=int, default=3)
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  cfg = BN.FULL
  dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
  unet_w = Wt.init_weights(Wt.unet_manifest(**cfg["unet"]), seed=2, scope="unet")
  txt = TransformerModel(**cfg["cond_stage_model"], dtype=torch.float32, device=dev,
                         weights=Wt.init_weights(Wt.transformer_manifest(**cfg["cond_stage_model"]), seed=2,
                                                 scope="cond_stage_model"))
  ae = AutoencoderKL(**cfg["autoencoder_kl"], dtype=torch.float32, device=dev,
                     weights=Wt.init_weights(Wt.decoder_manifest(**cfg["autoencoder_kl"]), seed=2, scope="autoencoder"))
  ldm = dict(cfg["ldm"], num_ddim_steps=args.steps)
  B, L = args.batch, args.latent
  ids = BN.synthetic_token_ids(B)
  shape = [B, L, L, 4]
  # one sampler for off / on: the loops with and without the maps keep their graphs in slots of their own
  s = LatentDiffusionModelSampler(UNet(**cfg["unet"], weights=unet_w, dtype=dtype, device=dev), ae, txt, verbose=False,
                                  **ldm)
  nb = LatentDiffusionModelSampler(UNet(**cfg["unet"], weights=unet_w, dtype=dtype, device=dev, fused_block=False), ae,
                                   txt, verbose=False, **ldm)
  st_block = []
  from ldm_tf2_amd import ops
  orig = ops.st_block
  ops.st_block = lambda *a, **k: (st_block.append(1), orig(*a, **k))[1]

  def loop(sampler, maps):
    def run():
      sampler.ddim_p_sample_loop(ids, shape, 5., seed=0, attn_maps=maps)
      return sampler.last_loop_ms_per_step()     # (synchronises)
    return run

  forms = [("off", loop(s, None)), ("on", loop(s, True)), ("off_no_block", loop(nb, None))]
  blocks = {}
  for name, fn in forms:
    st_block.clear()
    fn()                                         # warm-up + capture (the warm-up and the captured step: two steps)
    blocks[name] = len(st_block) // 2
  ops.st_block = orig
  step_ms = {name: [] for name, _ in forms}
  for r in range(args.rounds):
    for name, fn in (forms[::-1] if r % 2 else forms):
      step_ms[name].append(fn())
  med = {k: float(np.median(v)) for k, v in step_ms.items()}
  m = s.last_attention_maps()
  out = dict(batch=B, latent=L, ddim_steps=args.steps, unet_dtype=args.dtype, layers=len(m["layers"]),
             heat=list(m["heat"].shape), st_block_launches_per_step=blocks,
             ms_per_step={k: [round(x, 4) for x in v] for k, v in step_ms.items()},
             median_ms_per_step={k: round(v, 4) for k, v in med.items()},
             on_over_off=round(med["on"] / med["off"] - 1, 5),
             no_block_over_off=round(med["off_no_block"] / med["off"] - 1, 5),
             map_launches_ms=round(med["on"] - med["off_no_block"], 4))
  print(json.dumps(out))


if __name__ == "__main__":
  main()
