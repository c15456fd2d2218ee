#!/usr/bin/env python3
"""Records what the three host queries of ldm_gemm answer over a fixed grid (no GPU: nothing is launched):

    python tests/golden/record_gemm_plans.py                  # writes tests/golden/gemm_plans.json
    python tests/golden/record_gemm_plans.py --rows FILE      # also dumps every row as text, for diffing two builds

Run it on the library whose plans are to be the reference (LDM_HIP_LIB names another build of the same ABI);
tests/test_gemm_plan_identity_cpu.py repeats the sweep on the current build and compares exactly.  The golden file is
re-recorded only by a change that means to alter the cost model, the tile rules or the packaged plan tables.

A row is (status of ldm_gemm_plan, tile, split_k, ldm_gemm_splits, ldm_gemm_workspace_bytes).  The grid is the
Cartesian product of: dtype, form, act | M, N, K, forced tile 0..19, split_k, workspace (in sweep order; the part before
the bar names a group).  One more group holds every key of the packaged plan tables, unforced and with its planned
(tile, split).  The conv and conv_a2 forms take Cin = K // 9 whatever K is, so K = 64, 320 and 1280 give rows with
K != 9 Cin (+ Cin2) that ldm_gemm itself would reject: the plan queries do not look at Cin, and those rows pin the plan of
such K all the same.  Per group the file keeps the count of each distinct (tile, split) answer and a SHA-256 of the rows.
"""
import argparse
import ctypes as C
import glob
import hashlib
import json
import os
import subprocess
import sys
from array import array
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "gemm_plans.json")

F32, BF16, ACT_NONE, ACT_GEGLU = 0, 1, 0, 2
MS = (16, 64, 256, 512, 2048, 8192, 32768)
NS = (64, 128, 160, 320, 640, 1280, 2560)
KS = (64, 320, 1280, 2880, 11520)
FORMS = ("plain", "conv", "conv_a2", "out2", "ln_cs", "phase")
TILES = range(20)
SPLITS = (0, 1, 4)
WS_BYTES = 96 << 20
# M -> (B, H, W) of the 3x3 convolution (M = B*H*W) and of the phase form (M = B*4*H*W)
CONV_GEOM = {16: (1, 4, 4), 64: (1, 8, 8), 256: (1, 16, 16), 512: (2, 16, 16), 2048: (2, 32, 32), 8192: (8, 32, 32),
             32768: (32, 32, 32)}
PHASE_GEOM = {16: (1, 2, 2), 64: (1, 4, 4), 256: (1, 8, 8), 512: (2, 8, 8), 2048: (2, 16, 16), 8192: (2, 32, 32),
              32768: (8, 32, 32)}
PTR = 0x10000          # a 16-byte-aligned stand-in: the host queries never dereference an operand


def _base(P, dtype, act, M, N, K):
  p = P()
  p.a, p.w, p.out = PTR, PTR, PTR
  p.M, p.N, p.K, p.batch = M, N, K, 1
  p.lda, p.ldc_m, p.ldc_n = K, (N // 2 if act == ACT_GEGLU else N), 1
  p.act, p.dtype, p.out_dtype, p.alpha = act, dtype, dtype, 1.0
  return p


def _conv(p, B, H, W, Cin, upsample=0):
  p.conv, p.B, p.H, p.W, p.Cin, p.stride, p.upsample = 1, B, H, W, Cin, 1, upsample
  p.OH, p.OW = (2 * H, 2 * W) if upsample else (H, W)
  p.lda = Cin


def form_params(P, form, dtype, act, M, N, K):
  p = _base(P, dtype, act, M, N, K)
  if form == "conv":
    _conv(p, *CONV_GEOM[M], K // 9)
  elif form == "conv_a2":
    _conv(p, *CONV_GEOM[M], K // 9)
    p.a2, p.lda2, p.Cin2 = PTR, 64, 64
  elif form == "out2":
    p.out2, p.n_split, p.rows2, p.ld2, p.stride2 = PTR, N // 2, M, M, 0
  elif form == "ln_cs":
    p.ln_cs, p.ln_eps, p.bias = PTR, 1e-5, PTR
  elif form == "phase":
    _conv(p, *PHASE_GEOM[M], K // 4, upsample=2)
  return p


def key_params(P, key):
  """Parameters of one plan key (ops.plan_key), as far as the key carries them."""
  f, flags = {}, []
  for tok in key.split():
    name = tok.rstrip("0123456789")
    if name in ("x", "t", "sp", "ln"):
      flags.append(tok)
    else:
      f[name] = int(tok[len(name):])
  p = _base(P, f["dt"], f["act"], f["M"], f["N"], f["K"])
  p.batch, p.out_dtype = f["b"], f["odt"]
  if f["conv"]:
    _conv(p, 1, f["H"], f["W"], f["K"] // 9, f["u"])
    p.stride, p.no_lead_pad = f["s"], f["nlp"]
    hs, ws, pads = p.H * (2 if f["u"] else 1), p.W * (2 if f["u"] else 1), 1 if f["nlp"] else 2
    p.OH, p.OW = (hs + pads - 3) // p.stride + 1, (ws + pads - 3) // p.stride + 1
    p.B = max(1, p.M // (p.OH * p.OW))
  for tok in flags:
    if tok == "x2":
      p.a2, p.lda2, p.Cin2 = PTR, 64, 64
    elif tok == "t1":
      p.out2, p.n_split, p.rows2 = PTR, 0, p.M
    elif tok.startswith("sp"):
      p.out2, p.n_split, p.rows2 = PTR, int(tok[2:]), p.M
    elif tok == "ln1":
      p.ln_cs, p.ln_eps, p.bias = PTR, 1e-5, PTR
  return p


class _Group:
  def __init__(self):
    self.rows, self.answers = array("q"), Counter()

  def summary(self):
    return {"rows": len(self.rows) // 5, "sha256": hashlib.sha256(self.rows.tobytes()).hexdigest(),
            "answers": {"%d,%d" % k: v for k, v in sorted(self.answers.items())}}


def sweep(lib, P, dump=None):
  """{group name: summary}.  `lib`, `P`: the loaded library and its parameter struct (ldm_tf2_amd._lib)."""
  tile, split = C.c_int(), C.c_int()
  plan, splits, wsb = lib.ldm_gemm_plan, lib.ldm_gemm_splits, lib.ldm_gemm_workspace_bytes
  tref, sref = C.byref(tile), C.byref(split)

  def ask(g, p, name):
    ref = C.byref(p)
    tile.value = split.value = -1
    st = plan(ref, tref, sref)
    row = (st, tile.value, split.value, splits(ref), wsb(ref))
    g.rows.extend(row)
    g.answers[row[1:3]] += 1
    if dump:
      dump.write("%s M%d N%d K%d t%d s%d ws%d -> %d %d %d %d %d\n" %
                 ((name, p.M, p.N, p.K, p.tile, p.split_k, p.workspace_bytes) + row))

  out = {}
  for dtype in (F32, BF16):
    for form in FORMS:
      for act in (ACT_NONE, ACT_GEGLU):
        name = "%s %s %s" % ("bf16" if dtype == BF16 else "f32", form, "geglu" if act else "none")
        g = _Group()
        for M in MS:
          for N in NS:
            for K in KS:
              p = form_params(P, form, dtype, act, M, N, K)
              for p.tile in TILES:
                for p.split_k in SPLITS:
                  for p.workspace, p.workspace_bytes in ((PTR, WS_BYTES), (None, 0)):
                    ask(g, p, name)
        out[name] = g.summary()
  g = _Group()
  for path in sorted(glob.glob(os.path.join(ROOT, "ldm_tf2_amd", "plans", "*.json"))):
    for key, (t, s) in json.load(open(path))["plans"].items():
      p = key_params(P, key)
      p.workspace, p.workspace_bytes = PTR, WS_BYTES
      for p.tile, p.split_k in ((0, 0), (t, s)):
        ask(g, p, os.path.basename(path) + " " + key)
  out["packaged plan keys"] = g.summary()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=GOLDEN)
  ap.add_argument("--rows", help="dump every row as text to this file")
  ap.add_argument("--commit", help="commit the library was built from (default: git rev-parse HEAD)")
  a = ap.parse_args()
  from ldm_tf2_amd import _lib
  commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                                      check=True).stdout.strip()
  dump = open(a.rows, "w") if a.rows else None
  groups = sweep(_lib.lib, _lib.GemmParams, dump)
  if dump:
    dump.close()
  distinct = set()
  for g in groups.values():
    distinct |= set(g["answers"])
  with open(a.out, "w") as f:
    json.dump({"about": "ldm_gemm_plan / ldm_gemm_splits / ldm_gemm_workspace_bytes over the grid of "
                        "tests/golden/record_gemm_plans.py", "recorded_at_commit": commit,
               "queries": sum(g["rows"] for g in groups.values()), "distinct_tile_split_answers": len(distinct),
               "groups": groups}, f, indent=1)
    f.write("\n")
  print("%d queries, %d distinct (tile, split) answers -> %s" % (sum(g["rows"] for g in groups.values()),
                                                                 len(distinct), a.out))


if __name__ == "__main__":
  main()
