#!/usr/bin/env python3
"""Fits the latent previews' matrix on the final latents of a run and writes it as a .npy, the
file `ldm_sampling.preview_matrix` names.  The run is the one the YAML describes (the sampler CLI's call, without its
preview keys); its final latents [B,h,w,c] are decoded by the run's own autoencoder, and the f x f block means of the
images are regressed on [latents, 1] (model_runners.fit_latent_preview).  `--runs` repeats the run under the seeds
seed, seed + 1, .. and fits on all their latents: B * runs * h * w cells for c + 1 unknowns per colour.

    python tools/fit_preview.py --config_path all_in_one_config.yaml [--dtype bf16|f32] [--seed 0] [--runs 1] \
        [--out preview_matrix.npy]
"""
import argparse
import os
import sys

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldm_tf2_amd import run_ldm_sampler as R  # noqa: E402
from ldm_tf2_amd.tokenizer import get_token_ids  # noqa: E402


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--config_path", required=True)
  ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
  ap.add_argument("--seed", type=int, default=0)
  ap.add_argument("--runs", type=int, default=1)
  ap.add_argument("--out", default="preview_matrix.npy")
  args = ap.parse_args(argv)
  with open(args.config_path) as f:
    config = yaml.safe_load(f)
  samp = config["ldm_sampling"]
  for key in ("preview_freq",) + R.PREVIEW_KEYS:
    samp.pop(key, None)
  samp["sample_save_progress"] = False
  sampler = R.build_from_config(config, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32, verbose=False)
  max_len = config["cond_stage_model"]["max_seq_len"]
  token_ids = get_token_ids(samp["text_prompt"], samp["latent_shape"][0], samp["vocab_dir"], max_len)
  source_ids = None
  if samp.get("source_prompt") is not None:
    source_ids = get_token_ids(samp["source_prompt"], samp["latent_shape"][0], samp["vocab_dir"], max_len)
  latents = []
  for run in range(args.runs):
    method, args_, kwargs = R.sampling_call(config, token_ids, args.seed + run, source_ids=source_ids)
    getattr(sampler, method)(*args_, **kwargs)
    latents.append(sampler._xt.clone())          # (every loop leaves its final latents there)
  proj = sampler.fit_preview(latents=torch.cat(latents))
  np.save(args.out, proj)
  print(f"[INFO] preview matrix {proj.shape} fitted on {sum(int(x.shape[0]) for x in latents)} latents "
        f"-> '{args.out}'")
  print(np.array2string(proj, precision=4))


if __name__ == "__main__":
  main()
