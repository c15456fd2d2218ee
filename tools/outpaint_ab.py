#!/usr/bin/env python3
"""Times ldm_pushpull_fill at the two canvases the outpaint loop meets, 256 x 256 and 512 x 512
pixels, c = 3, B = 4, with every pyramid level in its own launch (lds_tail 0) and with the LDS tail (lds_tail 1), the
outpaint mask (a centred box of half the extents is kept), and next to it the call the fill precedes: the KL encoder
on the same B images (float32, the flagship autoencoder's shape, seeded random weights).  Events on the stream around
`--iters` back-to-back calls after a warm-up, median of 5 repeats; the two launch structures are timed in turn inside
each repeat, so a drift of the clocks meets both.  The workspace is made before the clock starts.  Writes
profiles/outpaint_ab.json and prints the same JSON line.  A report, not a gate.

    python tools/outpaint_ab.py [--iters 200] [--encoder-iters 5] [--out profiles/outpaint_ab.json]
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


def launches(H, W, c, lds_tail):
  """The launches of one call: a pull and a push per level below the tail's, and the tail."""
  L = T = int(np.ceil(np.log2(max(H, W))))
  if lds_tail and c <= 10:
    T = next(l for l in range(L + 1) if -(-H >> l) <= 32 and -(-W >> l) <= 32)
  return 2 * T + (1 if T < L else 0)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=4)
  ap.add_argument("--channels", type=int, default=3)
  ap.add_argument("--iters", type=int, default=200)
  ap.add_argument("--encoder-iters", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outpaint_ab.json"))
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  B, c = args.batch, args.channels
  out = dict(batch=B, channels=c, iters=args.iters, encoder_iters=args.encoder_iters, sizes={})
  cfg = BN.FULL["autoencoder_kl"]
  for S in SIZES:
    x = torch.rand(B, S, S, c, device=dev) * 2 - 1
    keep = torch.zeros(B, S, S, device=dev)
    keep[:, S // 4:3 * S // 4, S // 4:3 * S // 4] = 1.
    dst = torch.empty_like(x)
    fns = {tail: (lambda tail=tail: ops.pushpull_fill(x, keep, out=dst, lds_tail=bool(tail))) for tail in (0, 1)}
    same = torch.equal(fns[0]().clone(), fns[1]())
    for fn in fns.values():
      for _ in range(20):
        fn()
    us = {0: [], 1: []}
    for _ in range(5):
      for tail, fn in fns.items():
        us[tail].append(timed(fn, args.iters))
    res = dict(bytes_image=4 * B * S * S * c, same_bits=bool(same))
    for tail in (0, 1):
      res[f"lds_tail_{tail}"] = dict(us=round(float(np.median(us[tail])), 3), launches=launches(S, S, c, tail),
                                     us_all=[round(v, 3) for v in us[tail]])
    if c == 3:
      man = Wt.decoder_manifest(**cfg)
      man.update(Wt.encoder_manifest(**cfg, image_size=S, double_z=True))
      ae = AutoencoderKL(**cfg, weights=Wt.init_weights(man, seed=2, scope="autoencoder"), dtype=torch.float32,
                         device=dev, image_size=S)
      for _ in range(2):
        ae.encode(x)
      enc = [timed(lambda: ae.encode(x), args.encoder_iters) for _ in range(5)]
      res["encoder_us"] = round(float(np.median(enc)), 1)
      del ae
    out["sizes"][str(S)] = res
  line = json.dumps(out)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  print(line)


if __name__ == "__main__":
  main()
