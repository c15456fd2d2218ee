#!/usr/bin/env python3
"""Times ldm_resample_nhwc, both launches of a call together, at the two shapes the loops meet:
a photograph brought down to the autoencoder's size (1024 x 1024 -> 256 x 256) and pass 1's decoded image enlarged for
pass 2 (256 x 256 -> 512 x 512), c = 3, B = 4, every filter.  Events around `--iters` back-to-back calls, median of 5
repeats; the tables are built before the clock starts.  Next to each time the bytes a call has to move (x read, tmp
written and read, out written) and the bandwidth that makes, to be read against the device's peak: the expectation is
a call bound by memory traffic and launch latency, a few tens of microseconds, nothing next to one encoder pass.
Writes profiles/resample_ab.json and prints the same JSON line.  A report, not a gate.

    python tools/resample_ab.py [--iters 200] [--out profiles/resample_ab.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd._lib import RESAMPLE_FILTERS  # noqa: E402
from ldm_tf2_amd.resample import resample_taps  # noqa: E402

SHAPES = {"shrink_1024_256": ((1024, 1024), (256, 256)), "enlarge_256_512": ((256, 256), (512, 512))}


def time_call(fn, iters):
  """Median over 5 repeats of (device time of `iters` back-to-back calls) / iters, in microseconds."""
  for _ in range(10):
    fn()
  out = []
  for _ in range(5):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
      fn()
    t1.record()
    t1.synchronize()
    out.append(t0.elapsed_time(t1) * 1000. / iters)
  return round(float(np.median(out)), 3)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=4)
  ap.add_argument("--channels", type=int, default=3)
  ap.add_argument("--iters", type=int, default=200)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_ab.json"))
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  B, c = args.batch, args.channels
  out = dict(batch=B, channels=c, iters=args.iters, shapes={})
  for label, ((H, W), (Ho, Wo)) in SHAPES.items():
    x = torch.rand(B, H, W, c, device=dev) * 2 - 1
    dst = torch.empty(B, Ho, Wo, c, device=dev)
    moved = 4 * B * c * (H * W + 2 * H * Wo + Ho * Wo)
    res = dict(src=[H, W], dst=[Ho, Wo], bytes_moved=moved, filters={})
    for name in RESAMPLE_FILTERS:
      us = time_call(lambda: ops.resample_nhwc(x, (Ho, Wo), name, out=dst), args.iters)
      res["filters"][name] = dict(us=us, gb_per_s=round(moved / us * 1e-3, 1), xtaps=resample_taps(W, Wo, name)[2],
                                  ytaps=resample_taps(H, Ho, name)[2])
    out["shapes"][label] = res
  line = json.dumps(out)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
  print(line)


if __name__ == "__main__":
  main()
