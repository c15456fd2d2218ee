"""Pin the output bits of the eight sampler update entries (ops.cfg_*_update*) from outside the code under test.

  LDM_HIP_LIB=<library of the commit to record> python tools/update_bits.py --commit <hash> --write
writes tests/golden/update_bits.json: per case one SHA-256 over the SHA-256 digests of xt_out, pred_x0_out, both halves
of x_unet_out and the ring slot written, and *index afterwards, plus the commit the library was built from and the ROCm version.  Without
--write it prints how many cases of the library loaded now differ from the file.  tests/test_update_bits_gpu.py runs
the same cases against the library under test.

Inputs come from integer arithmetic in numpy alone (a multiplicative hash of the element index; no library generator,
no kernel of the project), so the same case has the same input bits on every machine.  What a case must not read holds
NaN: ring slots outside (idx+1 .. idx+j) & 3, the unconditional half of eps_all and gtab[idx] in conditional-only steps.
"""
from __future__ import annotations

import argparse
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "update_bits.json")
N = 8                                  # rows of coef / q_coef / gtab / weights
SMALL, ODD, LARGE = (2, 8, 8, 4), (2, 3, 3, 3), (5, 232, 232, 4)    # LARGE: B n / 4 = 269120 > 1024 * 256 threads
SEED = (1 << 32) + 7


def unit(count, salt):
  """float64 [count] in [0, 1), multiples of 2^-24: the top 24 bits of (i + 1 + salt * 2^20) * 2654435761 mod 2^32."""
  i = np.arange(count, dtype=np.uint64) + np.uint64(1 + (salt << 20))
  return (((i * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float64) / float(1 << 24)


def field(shape, salt, lo=-2., hi=2.):
  """float32 `shape` in [lo, hi) (exact for the default range: (k - 2^23) / 2^22)."""
  return (lo + (hi - lo) * unit(int(np.prod(shape)), salt)).astype(np.float32).reshape(shape)


def tables(sigma):
  """coef [N,4] = (c1, c2, a_prev, sigma) with 1 - a_prev - sigma^2 > 0, q_coef [N,2], gtab [N]."""
  coef = np.stack([field(N, 1, 1., 3.), field(N, 2, .1, 2.), field(N, 3, .05, .9),
                   field(N, 4, .05, .3) if sigma else np.zeros(N, np.float32)], 1)
  return coef, np.stack([field(N, 5, .2, 1.), field(N, 6, .1, 1.)], 1), field(N, 7, 1.5, 7.5)


def weight_table(kind):
  """float32 [N,4,4]: "plms" = the Adams-Bashforth constants in every row; "deis" = model_runners.deis_weights on a
  rising lambda grid, rounded to multiples of 2^-12 (so that an ulp of the host's exp cannot move an input bit)."""
  from ldm_tf2_amd.model_runners import PLMS_WEIGHTS, deis_weights
  w = np.zeros((N, 4, 4), dtype=np.float32)
  lam = lambda i: -3. + .55 * (N - i) + .03 * (N - i) ** 2          # rises as the index falls
  for i, j in itertools.product(range(N), range(4)):
    if kind == "plms":
      w[i, j, :j + 1] = np.array(PLMS_WEIGHTS[j], dtype=np.float32)
    else:
      w[i, j, :j + 1] = np.round(deis_weights([lam(i + m) for m in range(j + 1)], lam(i - 1)) * 4096.) / 4096.
  return w


def cases():
  """[(name, dict)]: entry, shape, x (dtype of x_unet), blend, idx, j, sigma, clip, guided, weights, alias."""
  out = []

  def add(entry, **kw):
    c = dict(dict(shape=SMALL, x="f32", blend=False, idx=5, j=0, sigma=False, clip=False, guided=True, weights=None,
                  alias=False), entry=entry, **kw)
    name = "-".join([entry, "x".join(map(str, c["shape"])), c["x"], "blend" if c["blend"] else "plain",
                     f"idx{c['idx']}", f"j{c['j']}"] + [k for k in ("sigma", "clip", "alias") if c[k]] +
                    (["guided" if c["guided"] else "cond", f"w_{c['weights']}"] if entry.startswith("sched") else []))
    out.append((name, c))

  X, I, TF = ("f32", "bf16"), (0, 5), (False, True)
  for x, idx, sigma, clip in itertools.product(X, I, TF, TF):
    add("ddim", x=x, idx=idx, sigma=sigma, clip=clip)
    add("ddim_masked", x=x, blend=True, idx=idx, sigma=sigma, clip=clip)
    for blend in TF:
      add("ddim_rng", x=x, blend=blend, idx=idx, sigma=sigma, clip=clip)
  for x in X:
    add("ddim", shape=ODD, x=x, sigma=True)                          # n_per_sample = 27: the scalar entry only
  for entry, x, blend, idx, j in itertools.product(("plms", "plms_rng", "ms", "ms_rng"), X, TF, I, range(4)):
    add(entry, x=x, blend=blend, idx=idx, j=j, weights=None if entry.startswith("plms") else "deis")
  for x, blend, rng, guided, w, idx in itertools.product(X, TF, ("sched", "sched_rng"), TF, (None, "plms", "deis"), I):
    for j in {None: (0,), "plms": (1, 3), "deis": range(4)}[w]:
      add(rng, x=x, blend=blend, idx=idx, j=j, guided=guided, weights=w)
  for entry in ("ddim", "ddim_masked", "ddim_rng", "plms", "plms_rng", "ms", "ms_rng", "sched", "sched_rng"):
    hist = dict(j=2, weights=None if entry.startswith("plms") else "deis") if "ddim" not in entry else dict(sigma=True)
    add(entry, x="bf16", blend=entry != "ddim", alias=True, **hist)
    add(entry, shape=LARGE, x="bf16", blend=entry != "ddim", idx=3, **hist)
  return [(n, dict(c, entry="sched", rng=True) if c["entry"] == "sched_rng" else c) for n, c in out]


def run_case(c, dev, repeat=1):
  """Build the inputs of case `c`, call its ops wrapper (`repeat` times: tools/update_kernels_bench.py) and return
  [sha256 of the outputs, *index afterwards]."""
  import torch
  from ldm_tf2_amd import ops
  entry, shape, idx, j = c["entry"], c["shape"], c["idx"], c["j"]
  Bn, numel = shape[0], int(np.prod(shape))
  d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  coef, q_coef, gtab = tables(c["sigma"])
  eps = field((2,) + shape, 11)
  ring = np.full((4,) + shape, np.nan, np.float32)
  for k in range(1, j + 1):
    ring[(idx + k) & 3] = field(shape, 20 + k)
  cond_only = entry == "sched" and not c["guided"]
  if cond_only:
    eps[0] = np.nan
    gtab[idx] = np.nan
  eps_all = d(eps.reshape((2 * Bn,) + shape[1:]))
  xt, ring = d(field(shape, 12)), d(ring)
  xt_out = xt if c["alias"] else torch.full(shape, float("nan"), device=dev)
  px = torch.full(shape, float("nan"), device=dev)
  xu = torch.zeros((2 * Bn,) + shape[1:], device=dev, dtype=torch.bfloat16 if c["x"] == "bf16" else torch.float32)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  start = torch.tensor([idx + j], dtype=torch.int32, device=dev)
  rng = d(np.array([SEED & 0xffffffff, SEED >> 32, 3, 0], dtype=np.uint32).view(np.int32))
  common = dict(x_unet_out=xu, dec_index=c.get("dec", bool((idx + j) & 1)), pred_x0_out=px)
  blend = {}
  if c["blend"]:
    mask = np.minimum((unit(numel // shape[-1], 13) * 4.).astype(np.int64), 2).astype(np.float32) * .5   # 0, .5, 1, 1
    blend = dict(z0=d(field(shape, 14)), mask=d(mask.reshape(shape[:-1])), q_coef=d(q_coef))
  table_q = dict(q_noise=d(field((N,) + shape, 15)), q_index_stride=numel) if c["blend"] else {}
  w = d(weight_table(c["weights"])) if c["weights"] else None
  coef, gtab, gs = d(coef), d(gtab), 5.5
  head, ring_head = (eps_all, xt, xt_out, coef, index), (eps_all, xt, xt_out, ring, coef, index, start)
  if entry in ("ddim", "ddim_masked"):
    noise = dict(noise=d(field((N,) + shape, 16)), noise_index_stride=numel) if c["sigma"] else {}
    if entry == "ddim":
      call = lambda: ops.cfg_ddim_update(*head, gs, clip_denoised=c["clip"], **noise, **common)
    else:
      call = lambda: ops.cfg_ddim_update_masked(*head, gs, blend["z0"], blend["mask"], table_q["q_noise"],
                                                blend["q_coef"], clip_denoised=c["clip"], q_index_stride=numel,
                                                **noise, **common)
  elif entry == "ddim_rng":
    call = lambda: ops.cfg_ddim_update_rng(*head, rng, gs, clip_denoised=c["clip"], **blend, **common)
  elif entry == "plms":
    call = lambda: ops.cfg_plms_update(*ring_head, gs, **blend, **table_q, **common)
  elif entry == "plms_rng":
    call = lambda: ops.cfg_plms_update_rng(*ring_head, rng, gs, **blend, **common)
  elif entry == "ms":
    call = lambda: ops.cfg_ms_update(*ring_head, w, gs, **blend, **table_q, **common)
  elif entry == "ms_rng":
    call = lambda: ops.cfg_ms_update_rng(*ring_head, w, rng, gs, **blend, **common)
  else:
    hist = dict(ring=ring, start=start, weights=w) if w is not None else {}
    draws = c.get("rng", False)
    call = lambda: ops.cfg_sched_update(*head[:4], gtab, index, c["guided"], rng=rng if draws else None, **hist,
                                        **blend, **({} if draws else table_q), **common)
  for _ in range(repeat):
    call()
  torch.cuda.synchronize()
  # one digest per case: the SHA-256 of the outputs' own SHA-256 hex digests, in this order
  sha = lambda t: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
  parts = [sha(t) for t in (xt_out, px, xu[:Bn], xu[Bn:], ring[idx & 3])]
  return [hashlib.sha256("".join(parts).encode()).hexdigest(), int(index.item())]


def rocm_version():
  import torch
  return str(torch.version.hip)


def main():
  import torch
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--commit", default=None, help="the commit the loaded library was built from (recorded with --write)")
  ap.add_argument("--write", action="store_true", help=f"write {os.path.relpath(FIXTURE, ROOT)}")
  a = ap.parse_args()
  dev = torch.device("cuda:0")
  got = {name: run_case(c, dev) for name, c in cases()}
  if a.write:
    if not a.commit:
      ap.error("--write needs --commit")
    with open(FIXTURE, "w") as f:
      json.dump(dict(commit=a.commit, rocm=rocm_version(), cases=got), f, indent=0, sort_keys=True)
      f.write("\n")
    print(f"wrote {len(got)} cases to {FIXTURE}")
    return 0
  with open(FIXTURE) as f:
    want = json.load(f)
  bad = [n for n in got if got[n] != want["cases"].get(n)]
  print(f"{len(got)} cases, {len(bad)} differ from the fixture of commit {want['commit']} (ROCm {want['rocm']}; here "
        f"{rocm_version()})" + "".join(f"\n  {n}" for n in bad))
  return 1 if bad else 0


if __name__ == "__main__":
  sys.exit(main())
