#!/usr/bin/env python3
"""Same-process, interleaved A/B of the txt2img loop at the C3 shape (bf16 U-Net, f32 text encoder and autoencoder,
B=16, 32x32 latents, N=200) without previews, with preview_freq 1 and with preview_freq 5 (DESIGN.md section 17:
scale 8, bilinear, one ldm_latent_preview launch inside every captured step), each as ms per U-Net step from
last_loop_ms_per_step (graph replay, device time), and against ddim_p_sample_loop_progressive with record_freq 5 as
wall time of the whole call, its decodes of the recorded latents included.  The loop without previews is the parent
commit's loop: its graph key, launches and replayed graph are unchanged.  A report, not a gate.

    python tools/preview_ab.py [--batch 16] [--latent 32] [--steps 200] [--rounds 3]
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
  unet = UNet(**cfg["unet"], weights=Wt.init_weights(Wt.unet_manifest(**cfg["unet"]), seed=2, scope="unet"),
              dtype=torch.bfloat16, device=dev)
  txt = TransformerModel(**cfg["cond_stage_model"], dtype=torch.float32, device=dev,
                         weights=Wt.init_weights(Wt.transformer_manifest(**cfg["cond_stage_model"]), seed=2,
                                                 scope="cond_stage_model"))
  ae = AutoencoderKL(**cfg["autoencoder_kl"], dtype=torch.float32, device=dev,
                     weights=Wt.init_weights(Wt.decoder_manifest(**cfg["autoencoder_kl"]), seed=2, scope="autoencoder"))
  ldm = dict(cfg["ldm"], num_ddim_steps=args.steps)
  B, L = args.batch, args.latent
  ids = BN.synthetic_token_ids(B)
  shape = [B, L, L, 4]
  # one sampler: the loops with and without previews keep their graphs in slots of their own
  s = LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **ldm)
  proj = (0.3 * np.random.default_rng(0).standard_normal((5, 3))).astype(np.float32)
  s.set_preview(proj)                            # scale = the autoencoder's factor (8), bilinear

  def loop(q):
    def run():
      t0 = time.perf_counter()
      s.ddim_p_sample_loop(ids, shape, 5., seed=0, preview_freq=q)
      ms = s.last_loop_ms_per_step()             # (synchronises)
      if q is not None:
        s.last_previews()                        # the strips' copy to the host belongs to the call
      return ms, (time.perf_counter() - t0) * 1e3
    return run

  def progressive():
    t0 = time.perf_counter()
    out = s.ddim_p_sample_loop_progressive(ids, shape, 5., record_freq=5, seed=0)
    [o.cpu() for o in out[1:]]
    torch.cuda.synchronize()
    return None, (time.perf_counter() - t0) * 1e3

  forms = [("no_preview", loop(None)), ("preview_freq_1", loop(1)), ("preview_freq_5", loop(5)),
           ("progressive_freq_5", progressive)]
  for _, fn in forms:
    fn()                                         # warm-up + capture
  step_ms = {name: [] for name, _ in forms}
  wall_ms = {name: [] for name, _ in forms}
  for r in range(args.rounds):
    for name, fn in (forms[::-1] if r % 2 else forms):
      ms, wall = fn()
      if ms is not None:
        step_ms[name].append(ms)
      wall_ms[name].append(wall)
  med = {k: float(np.median(v)) for k, v in step_ms.items() if v}
  wall = {k: float(np.median(v)) for k, v in wall_ms.items()}
  pv = s.last_previews()
  out = dict(batch=B, latent=L, ddim_steps=args.steps, unet_dtype="bf16", scale=s._pv_scale, mode=s._pv_mode,
             frames=list(pv["sample"].shape),
             ms_per_step={k: [round(x, 4) for x in v] for k, v in step_ms.items() if v},
             median_ms_per_step={k: round(v, 4) for k, v in med.items()},
             preview_1_over_none=round(med["preview_freq_1"] / med["no_preview"] - 1, 5),
             preview_5_over_none=round(med["preview_freq_5"] / med["no_preview"] - 1, 5),
             median_call_wall_ms={k: round(v, 1) for k, v in wall.items()})
  print(json.dumps(out))


if __name__ == "__main__":
  main()
