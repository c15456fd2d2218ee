#!/usr/bin/env python3
"""Kernel durations of the eight sampler update entries at the benchmark shape (B = 16, 32x32x4 latents, bf16 x_unet).

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/update_kernels_bench.py
  python tools/update_kernels_bench.py --summarize <dir>/.../*_kernel_trace.csv > run.json
  python tools/update_kernels_bench.py --compare parent1.json new1.json parent2.json new2.json

The run launches every form of GROUPS `--iters` times in that order, without the index decrement, so the update
launches of the trace in time order are len(GROUPS) blocks of `--iters` dispatches: the summary attributes them by
position, not by kernel name, and so compares builds whose kernels are named differently (LDM_HIP_LIB selects the
build).  It prints one JSON line: form -> mean and median duration in ns over the last `iters - skip` dispatches.
"""
import argparse
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENTRIES = ("ddim", "ddim_masked", "ddim_rng", "plms", "plms_rng", "ms", "ms_rng", "sched", "sched_rng")
# (form, entry, blend): every entry plain, and with the blend where it is optional
GROUPS = [(e + ("+blend" if b else ""), e, b) for e in ENTRIES
          for b in ((True,) if e == "ddim_masked" else (False,) if e == "ddim" else (False, True))]
SHAPE = (16, 32, 32, 4)


def run(iters):
  import torch
  from tools import update_bits as U
  dev = torch.device("cuda:0")
  for _, entry, blend in GROUPS:
    c = dict(entry=entry, shape=SHAPE, x="bf16", blend=blend, idx=5, j=3 if "ddim" not in entry else 0, sigma=True,
             clip=False, guided=True, weights=None if entry.startswith("plms") or "ddim" in entry else "deis",
             alias=True, dec=False)
    if entry == "sched_rng":
      c.update(entry="sched", rng=True)
    U.run_case(c, dev, repeat=iters)
  torch.cuda.synchronize()


def summarize(trace_csv, iters, skip):
  rows = list(csv.DictReader(open(trace_csv)))
  key = lambda *names: next(n for n in names if n in rows[0])
  kn, ks, ke = key("Kernel_Name", "Name"), key("Start_Timestamp", "Start"), key("End_Timestamp", "End")
  upd = sorted((int(r[ks]), int(r[ke]) - int(r[ks]), r[kn]) for r in rows if "cfg_" in r[kn])
  assert len(upd) == iters * len(GROUPS), (len(upd), iters, len(GROUPS))
  out = {}
  for g, (form, _, _) in enumerate(GROUPS):
    blk = upd[g * iters:(g + 1) * iters]
    assert len({n for _, _, n in blk}) == 1, form            # one kernel per form
    d = sorted(t for _, t, _ in blk[skip:])
    out[form] = dict(mean_ns=round(sum(d) / len(d), 1), median_ns=d[len(d) // 2],
                     kernel=re.search(r"cfg_\w+", blk[0][2]).group(0))
  return out


def compare(parent1, new1, parent2, new2):
  """Four summaries, taken alternating -> per form the means, the margin (the larger of the two same-build
  differences) and whether mean(new) - mean(parent) stays inside it."""
  p1, n1, p2, n2 = (json.load(open(f)) for f in (parent1, new1, parent2, new2))
  out = {}
  for form in p1:
    p, n = [p1[form]["mean_ns"], p2[form]["mean_ns"]], [n1[form]["mean_ns"], n2[form]["mean_ns"]]
    margin = max(abs(p[0] - p[1]), abs(n[0] - n[1]))
    delta = sum(n) / 2 - sum(p) / 2
    out[form] = dict(parent_mean_ns=p, new_mean_ns=n, margin_ns=round(margin, 1), new_minus_parent_ns=round(delta, 1),
                     within_margin=delta <= margin, parent_kernel=p1[form]["kernel"], new_kernel=n1[form]["kernel"])
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=300)
  ap.add_argument("--skip", type=int, default=50, help="leading dispatches of each form left out of the summary")
  ap.add_argument("--summarize", default=None, metavar="KERNEL_TRACE_CSV")
  ap.add_argument("--compare", nargs=4, default=None, metavar=("PARENT1", "NEW1", "PARENT2", "NEW2"))
  a = ap.parse_args()
  if a.compare:
    print(json.dumps(compare(*a.compare), indent=1))
  elif a.summarize:
    print(json.dumps(summarize(a.summarize, a.iters, a.skip)))
  else:
    run(a.iters)


if __name__ == "__main__":
  main()
