"""Pin the output bits of one U-Net evaluation per launch form from outside the host walk under test.

  LDM_HIP_LIB=<library under test> python tools/unet_form_bits.py --tree <checkout to record> --commit <hash> --write
writes tests/golden/unet_form_bits.json: for every case of tests/test_zz_block_parity_gpu.py (CASES) and of
tests/test_unet_calls_gpu.py (CASES) the SHA-256 of the bytes of the evaluation's output, plus the commit of
<checkout> and the ROCm release.  `--tree` goes to the front of sys.path before the package is imported, so the walk
(ldm_tf2_amd/unet.py and what it imports) is that checkout's, while the library is the one LDM_HIP_LIB names: a change
of the host walk that keeps every launch and every operand reproduces the file.  Without --write it prints which cases
of the tree loaded now differ from the file.  tests/test_zz_unet_form_bits_gpu.py runs the same cases on the tree
under test.

Of the package a case uses `UNet(...)`, `set_context` and `forward` alone; models and inputs are the two test modules'
(16x16 latents, R = 4: tests/block_ref.py unet_case, test_unet_calls_gpu.evaluation).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "unet_form_bits.json")


def _paths(tree=None):
  for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
      sys.path.append(p)
  if tree is not None:
    sys.path.insert(0, os.path.abspath(tree))


def cases():
  """[(name, (module, the module's own case))]."""
  _paths()
  import block_ref as BR
  import test_unet_calls_gpu as TC
  import test_zz_block_parity_gpu as TP
  out = [(f"parity/{m}-{BR.TAG[d]}-{n}-{f}", ("parity", (m, d, n, f))) for m, d, n, f in TP.CASES]
  return out + [(f"calls/{n}", ("calls", n)) for n in TC.CASES]


def _parity(case, dev):
  """The evaluation of test_zz_block_parity_gpu._evaluate, without its recorder and taps."""
  import torch

  import block_ref as BR
  import test_zz_block_parity_gpu as TP
  from ldm_tf2_amd.unet import UNet
  model, dtype, name, form = case
  kw = {} if model == "B" else dict(TP.SMALL, **(TP.FORMS_BF16 if dtype == TP.BF16 else TP.FORMS_F32)[name][0])
  c = BR.unet_case(model)
  env = c["env"]
  x, t, ctx = env["x"].to(dev), torch.from_numpy(env["t"]).to(dev), env["ctx"].to(dev)
  u = UNet(**c["cfg"], context_dim=BR.CTX_DIM, weights=c["weights"], dtype=dtype, device=dev, **kw)
  u.set_context(ctx)
  fkw = dict(t_rows=t)
  if form == "paired":
    fkw["paired_rows"] = True
  elif form == "context_rows":
    x, fkw = x[2:].contiguous(), dict(t_rows=t[2:].contiguous(), context_rows=(2, 4))
  return u.forward(x, **fkw)


_W = {}


def _calls(name, dev):
  import test_unet_calls_gpu as TC
  from ldm_tf2_amd import weights as Wt
  model, dtype, kw, form = TC.CASES[name]
  if model not in _W:
    cfg, seed = (TC.UNET_CFG, 2) if model == "tiny" else (TC.MC320_CFG, 4)
    _W[model] = (cfg, Wt.init_weights(Wt.unet_manifest(context_dim=TC.CTX_DIM, **cfg), seed=seed, mode="random",
                                      scope="unet"))
  call, out = TC.evaluation(dev, *_W[model], dtype, kw, form)
  call()
  return out


def run_case(case, dev):
  """SHA-256 of the bytes of the case's output."""
  import torch
  kind, c = case
  out = (_parity if kind == "parity" else _calls)(c, dev)
  torch.cuda.synchronize()
  return hashlib.sha256(out.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def rocm_version():
  import torch
  return str(torch.version.hip)


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--tree", default=None, help="the checkout whose ldm_tf2_amd is imported (default: this one)")
  ap.add_argument("--commit", default=None, help="the commit of --tree (recorded with --write)")
  ap.add_argument("--write", action="store_true", help=f"write {os.path.relpath(FIXTURE, ROOT)}")
  a = ap.parse_args()
  _paths(a.tree or ROOT)
  import torch

  import ldm_tf2_amd
  print(f"package: {os.path.dirname(ldm_tf2_amd.__file__)}")
  dev = torch.device("cuda:0")
  got = {}
  for name, c in cases():
    got[name] = run_case(c, dev)
    print(f"{name} {got[name]}", flush=True)
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
