#!/usr/bin/env python3
"""Same-process, interleaved timing of DiffEdit's phases at the C3 shape (bf16 U-Net, f32 text encoder and autoencoder,
B=16, 32x32 latents, N=50), each with its captured graph on one sampler: the map phase (n
contrast steps), the inversion with and without `trajectory`, the masked sampling whose blend reads the trajectory, and
the plain edit loop's sampling next to it.  Times are device time of graph replay (last_loop_ms_per_step times the
loop's steps), ms per phase.  Then the accumulate kernel alone on a large tensor: bytes moved per second against the
HBM read figure of tools/probes/hbm_probe.hip as DESIGN.md records it.  Prints one JSON line.  A report, not a gate.

    python tools/diffedit_ab.py [--batch 16] [--latent 32] [--steps 50] [--maps 10] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as BN  # noqa: E402
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd import weights as Wt  # noqa: E402
from ldm_tf2_amd.autoencoder import AutoencoderKL  # noqa: E402
from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler  # noqa: E402
from ldm_tf2_amd.transformer import TransformerModel  # noqa: E402
from ldm_tf2_amd.unet import UNet  # noqa: E402

GS, STRENGTH = 5., 0.75
HBM_READ_TBS = 6.6                             # DESIGN.md, "HBM (hbm_probe.hip)": read 6.6 TB/s, write 5.5 TB/s


def accum_bandwidth(dev, B=16, cells=1 << 20, c=4, reps=20):
  eps = torch.randn(2 * B, cells, c, device=dev)
  acc = torch.zeros(B, cells, device=dev)
  for _ in range(3):
    ops.eps_contrast_accum(eps, acc)
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0.record()
  for _ in range(reps):
    ops.eps_contrast_accum(eps, acc)
  t1.record()
  t1.synchronize()
  ms = t0.elapsed_time(t1) / reps
  moved = eps.numel() * 4 + 2 * acc.numel() * 4                # both halves read, acc read and written
  return dict(bytes=moved, ms=round(ms, 4), tb_per_s=round(moved / ms / 1e9, 3),
              fraction_of_hbm_read=round(moved / ms / 1e9 / HBM_READ_TBS, 3))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=16)
  ap.add_argument("--latent", type=int, default=32)
  ap.add_argument("--steps", type=int, default=50)
  ap.add_argument("--maps", type=int, default=10)
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
  other = ids.copy()
  other[B:] = np.random.default_rng(2).integers(0, cfg["cond_stage_model"]["vocab_size"], size=ids[B:].shape)
  shape = [B, L, L, 4]
  z0 = (0.8 * np.random.default_rng(0).standard_normal(shape)).astype(np.float32)
  s = LatentDiffusionModelSampler(unet, ae, txt, verbose=False, **dict(cfg["ldm"], num_ddim_steps=N))
  k = int(STRENGTH * N)
  half = np.zeros((B, L, L), np.float32)
  half[:, :, :L // 2] = 1.
  state = {}

  def run(name):
    if name == "map":
      s.diffedit_mask(ids, other, latents=z0, num_maps=args.maps)
      steps = args.maps
    elif name == "invert":
      state["x"] = s.ddim_invert_loop(ids, latents=z0, strength=STRENGTH)
      steps = k
    elif name == "invert_trajectory":
      s.ddim_invert_loop(ids, latents=z0, strength=STRENGTH, trajectory=True)
      steps = k
    elif name == "masked_sampling":
      # (the loop's own phases from the inversion on, decoder left out: the trajectory is the previous arm's)
      s._set_context(s._cond_stage_model(other))
      s._owned("_mask_buf", half, (B, L, L))
      start = s._traj[k - 1]

      def set_start():
        s._xt.copy_(start), s._x2[:B].copy_(start), s._x2[B:].copy_(start)
      s._blend_traj = True
      try:
        s._denoise(k, set_start, GS, None, None, True, False, None, decode=False)
      finally:
        s._blend_traj = False
      steps = k
    else:
      s._sample_from(s._cond_stage_model(other), shape, k, GS, None, state["x"], None, 0, 0, None, decode=False)
      steps = k
    return s.last_loop_ms_per_step() * steps

  arms = ("map", "invert", "invert_trajectory", "masked_sampling", "edit_sampling")
  s._de_qcoef = torch.tensor([[0., 1.]] * N, dtype=torch.float32, device=dev)
  for _ in range(2):                            # warm-up + capture (the first pass allocates, which drops graphs)
    for name in arms:
      run(name)
  res = {name: [] for name in arms}
  for r in range(args.rounds):
    for name in (arms if r % 2 == 0 else arms[::-1]):
      res[name].append(run(name))
  out = dict(batch=B, latent=L, ddim_steps=N, k=k, maps=args.maps, unet_dtype="bf16", guidance_scale=GS,
             rounds=args.rounds, arms={})
  for name, ms in res.items():
    out["arms"][name] = dict(ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3))
  a = {n: v["median_ms"] for n, v in out["arms"].items()}
  out["trajectory_over_plain_inversion"] = round(a["invert_trajectory"] / a["invert"], 4)
  out["masked_over_edit_sampling"] = round(a["masked_sampling"] / a["edit_sampling"], 4)
  out["map_ms_per_draw"] = round(a["map"] / args.maps, 4)
  out["accumulate_kernel"] = accum_bandwidth(dev)
  print(json.dumps(out))


if __name__ == "__main__":
  main()
