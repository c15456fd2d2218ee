#!/usr/bin/env python3
"""Times the paste-back at the two image sizes the masked loops meet, 256 x 256 and 512 x 512
pixels, B = 4, c = 3, sigma = 4 (r = 12), the outpaint mask inverted (a centred box of half the extents is kept): the
feather as four launches (lds_tile 0) and as one LDS-tiled launch (lds_tile 1), the keep statistics and the paste, and
next to them the call they follow: the KL decoder on the same B images (float32, the flagship autoencoder's shape,
seeded random weights).  Events on the stream around `--iters` back-to-back calls after a warm-up, median of 5
repeats; the variants are timed in turn inside each repeat, so a drift of the clocks meets all of them.  Workspaces
and tap tables are made before the clock starts.  Writes profiles/paste_back_ab.json and prints the same JSON line.
A report, not a gate.

    python tools/paste_back_ab.py [--iters 200] [--decoder-iters 5] [--out profiles/paste_back_ab.json]
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

SIZES = (256, 512)


def timed(fn, iters):
  """Device time of `iters` back-to-back calls of fn, per call, in microseconds."""
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0.record()
  for _ in range(iters):
    fn()
  t1.record()
  t1.synchronize()
  return t0.elapsed_time(t1) * 1000. / iters


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=4)
  ap.add_argument("--channels", type=int, default=3)
  ap.add_argument("--sigma", type=float, default=4.)
  ap.add_argument("--iters", type=int, default=200)
  ap.add_argument("--decoder-iters", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paste_back_ab.json"))
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  B, c, sigma = args.batch, args.channels, args.sigma
  out = dict(batch=B, channels=c, sigma=sigma, iters=args.iters, decoder_iters=args.decoder_iters, sizes={})
  cfg = BN.FULL["autoencoder_kl"]
  for S in SIZES:
    o = torch.rand(B, S, S, c, device=dev) * 2 - 1
    d = torch.rand(B, S, S, c, device=dev) * 2 - 1
    keep = torch.zeros(B, S, S, device=dev)
    keep[:, S // 4:3 * S // 4, S // 4:3 * S // 4] = 1.
    w, dst = torch.empty_like(keep), torch.empty_like(d)
    _, gain, offset = ops.keep_stats(o, d, keep)
    fns = {
        "feather_lds_tile_0": lambda: ops.mask_feather(keep, sigma, out=w, lds_tile=False),
        "feather_lds_tile_1": lambda: ops.mask_feather(keep, sigma, out=w, lds_tile=True),
        "keep_stats": lambda: ops.keep_stats(o, d, keep),
        "paste_back": lambda: ops.paste_back(o, d, w, gain, offset, out=dst),
    }
    same = torch.equal(fns["feather_lds_tile_0"]().clone(), fns["feather_lds_tile_1"]())
    for fn in fns.values():
      for _ in range(20):
        fn()
    us = {name: [] for name in fns}
    for _ in range(5):
      for name, fn in fns.items():
        us[name].append(timed(fn, args.iters))
    res = dict(bytes_image=4 * B * S * S * c, same_bits=bool(same))
    for name in fns:
      res[name] = dict(us=round(float(np.median(us[name])), 3), us_all=[round(v, 3) for v in us[name]])
    if c == 3:
      man = Wt.decoder_manifest(**cfg)
      ae = AutoencoderKL(**cfg, weights=Wt.init_weights(man, seed=2, scope="autoencoder"), dtype=torch.float32,
                         device=dev)
      z = torch.randn(B, S // 8, S // 8, cfg["latent_channels"], device=dev)
      for _ in range(2):
        ae.decode(z)
      dec = [timed(lambda: ae.decode(z), args.decoder_iters) for _ in range(5)]
      res["decoder_us"] = round(float(np.median(dec)), 1)
      best = min(res["feather_lds_tile_0"]["us"], res["feather_lds_tile_1"]["us"])
      res["paste_back_share_of_decoder"] = round((best + res["keep_stats"]["us"] + res["paste_back"]["us"])
                                                 / res["decoder_us"], 5)
      del ae
    out["sizes"][str(S)] = res
  line = json.dumps(out)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  print(line)


if __name__ == "__main__":
  main()
