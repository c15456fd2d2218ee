"""Thin tensor-level wrappers over the C ABI (include/ldm_hip.h).

torch is used here only as the device-memory container and stream provider:
every function turns tensors into (pointer, stride, size) arguments and enqueues
hand-written HIP kernels from libldm_hip.so on torch's current stream.  Nothing
in this module computes with torch ops.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

from . import _lib
from ._lib import ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_SILU, BF16, F32, GemmParams, check, lib

__all__ = [
    "ACT_NONE", "ACT_GELU", "ACT_GEGLU", "ACT_SILU", "F32", "BF16", "code", "linear", "conv3x3",
    "bmm_nt", "conv3x3_small", "groupnorm", "layernorm", "softmax_rows", "attention",
    "time_embedding", "gemv", "cfg_ddim_update", "cfg_ddim_update_masked", "cfg_plms_update", "q_sample",
    "philox_u32", "normal_fill", "q_sample_rng", "cfg_ddim_update_rng", "cfg_plms_update_rng", "cfg_ms_update",
    "cfg_ms_update_rng", "cfg_sched_update", "cfg_ddim_invert_update", "window_gather", "window_fold", "window_gather_ex", "window_fold_ex", "wrap_pad", "resize_nhwc", "resample_nhwc", "latent_preview", "xattn_map", "xattn_map_supported",
    "eps_contrast_accum", "contrast_mask", "contrast_mask_supported", "store_row", "pushpull_fill", "pushpull_workspace", "mask_feather", "mask_feather_workspace", "keep_stats", "paste_back", "post_quant", "vq_nearest", "embedding",
    "minmax_u8", "cast",
]

_TORCH_DT = {torch.float32: F32, torch.bfloat16: BF16}
_byref = C.byref      # (functions below use C for a channel count)
_WS = {}
_WS_BYTES = 96 << 20


def code(dtype) -> int:
  try:
    return _TORCH_DT[dtype]
  except KeyError:
    raise TypeError(f"unsupported dtype {dtype}: the HIP path stores float32 or bfloat16")


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _ptr(t):
  if t is None:
    return None
  if not t.is_cuda:
    raise ValueError("the HIP path needs device tensors (there is no CPU fallback)")
  return t.data_ptr()


def _f32(t, what):
  if t is not None and t.dtype != torch.float32:
    raise TypeError(f"{what} must be float32")
  return t


def row_ld(t) -> int:
  """Row stride (elements) of `t` seen as a 2-D [rows, cols] matrix; the leading
  dims must collapse onto a single uniform stride (true for channel slices of
  NHWC buffers)."""
  if t.dim() < 2:
    return t.shape[-1]
  if t.shape[-1] != 1 and t.stride(-1) != 1:
    raise ValueError("last dim must be contiguous")
  ld = t.stride(-2)
  for i in range(t.dim() - 2, 0, -1):
    if t.shape[i - 1] != 1 and t.stride(i - 1) != t.stride(i) * t.shape[i]:
      raise ValueError(f"tensor with shape {tuple(t.shape)} strides {t.stride()} has no uniform row stride")
  return ld


def workspace(device):
  """Split-K partial-sum workspace for a launch made now.  ldm_gemm's slabs live from the GEMM
  launch to its reduce launch, in stream order, so one workspace serves one stream at a time:
  every model owns its own (`workspace_scope`, allocated at model build, before any graph
  capture); launches outside a model use one per (device, current stream)."""
  stack = _ws_stack()
  if stack:
    return stack[-1]
  key = (device, torch.cuda.current_stream(device).cuda_stream)
  ws = _WS.get(key)
  if ws is None:
    ws = new_workspace(device)
    _WS[key] = ws
  return ws


def new_workspace(device):
  return torch.empty(_WS_BYTES, dtype=torch.uint8, device=device)


# The scope stacks (workspace, active plan table) are per host THREAD: two samplers driven from two
# Python threads, one model each, must not see each other's workspace or plan table (the registry of
# loaded tables, _TABLES, is shared and only read inside a forward).
_TLS = threading.local()


def _ws_stack():
  st = getattr(_TLS, "ws", None)
  if st is None:
    st = _TLS.ws = []
  return st


class workspace_scope:
  """`with workspace_scope(ws): ...` -- ldm_gemm launches made by THIS thread inside use `ws` (a
  model's own workspace), so two models replaying on different streams -- from one host thread or
  from two -- never share split-K slabs."""

  def __init__(self, ws):
    self._ws = ws

  def __enter__(self):
    _ws_stack().append(self._ws)
    return self

  def __exit__(self, *exc):
    _ws_stack().pop()
    return False


# ---- per-shape launch plans -----------------------------------------------------------------
# ldm_gemm picks its tile and split-K with a cost model calibrated on isolated launches.  In
# the real step (weights cold in HBM, activations warm in L2/Infinity Cache, neighbours
# competing) the optimum differs on some shapes, so measured overrides can be loaded:
# {problem key: [tile, split_k]} JSON files written by tools/tune_step_plans.py, which times
# WHOLE captured U-Net steps while varying one shape's plan at a time.
#
# A table belongs to ONE step configuration (its file header: "config": {"rows": R, "latent":
# h, "dtype": "bf16"|"f32"}) because a problem key names a shape, not the step it sits in: the
# same shape occurs in different configurations with different in-situ optima.  Exactly one
# table is active at a time; the U-Net activates the table of its (rows, latent, dtype) for the
# duration of a forward (`plan_scope`), everything else runs on the cost model.  LDM_NO_PLANS=1
# disables the packaged tables, LDM_GEMM_PLANS=<file> registers another.  Plans only reorder
# float additions.
_TABLES = {}          # (rows, latent, dtype code) -> {key: (tile, split_k)}
_PLAN_RECORD = None


def _active():
  """This thread's active table (possibly edited in place by tools/tune_step_plans.py)."""
  return getattr(_TLS, "active", None) or {}


def _active_cfg():
  return getattr(_TLS, "active_cfg", None)


_TILES = _lib.tile_table()      # {tile: (BM, BN, resident workgroups per CU, LDM_TILE_* flags)}, csrc/gemm_tiles.h
_tiles_with = lambda flag: tuple(t for t, row in _TILES.items() if row[3] & flag)
_TILE_DIMS = {t: row[:3] for t, row in _TILES.items() if not row[3] & _lib.TILE_EXPERIMENTAL}   # what a plan may name
_BF16_TILES = _tiles_with(_lib.TILE_BF16_ONLY)
_PERSISTENT_TILES = _tiles_with(_lib.TILE_PERSISTENT)   # no split-K, N % BN == 0
_HALO_RING_TILES = _tiles_with(_lib.TILE_HALO)          # stride-1 convs whose M-tile is whole lines of one image
_GEGLU_TILES = _tiles_with(_lib.TILE_GEGLU)
_WHOLE_N_TILES = _tiles_with(_lib.TILE_WHOLE_N)         # offered only where N % BN == 0 (the N = 160*k layers)


def _halo_ring_key(key, M, N, bn):
  """True if the problem `key` names can run on a halo-staged conv tile (gemm.hip halo_ring_ok)."""
  import re
  m = re.search(r"conv1 H(\d+) W(\d+) s1 u0 nlp0", key or "")
  if not m or " x2" in (key or ""):          # (a second A operand runs on the implicit-GEMM tiles only)
    return False
  H, W = int(m.group(1)), int(m.group(2))
  return W in (16, 32) and H % (256 // W) == 0 and M % 256 == 0 and N % bn == 0


def plan_key(p) -> str:
  key = "M%d N%d K%d b%d conv%d H%d W%d s%d u%d nlp%d act%d dt%d odt%d" % (
      p.M, p.N, p.K, p.batch, p.conv, p.H, p.W, p.stride, p.upsample, p.no_lead_pad, p.act, p.dtype, p.out_dtype)
  if p.a2:
    key += " x2"            # second A operand (the ResBlock shortcut inside the convolution): K = 9 Cin + Cin2
  if p.out2 and p.n_split == 0:
    key += " t1"            # whole product stored transposed (linear_t)
  elif p.out2 and p.ln_cs:
    key += " sp%d" % p.n_split   # q | k row-major + V^T transposed in one LayerNorm-folded launch
  if p.ln_cs:
    key += " ln1"           # LayerNorm of the rows folded in (persistent tiles only)
  return key


def _cfg_key(rows, latent, dtype):
  dt = dtype if isinstance(dtype, int) else (BF16 if str(dtype) in ("bf16", "torch.bfloat16") else F32)
  return (int(rows), int(latent), dt)


def load_plans(path):
  """Registers the {key: [tile, split_k]} table of one JSON file under its header's
  configuration; returns that configuration key.  Two files for one configuration that
  disagree on a key are an error (a silently merged table is not the one that was measured)."""
  import json
  with open(path) as f:
    d = json.load(f)
  c = d.get("config")
  if not c:
    raise ValueError(f"{path}: plan table without a \"config\" header (rows / latent / dtype)")
  ck = _cfg_key(c["rows"], c["latent"], c["dtype"])
  table = _TABLES.setdefault(ck, {})
  for k, v in d["plans"].items():
    plan = (int(v[0]), int(v[1]))
    if table.get(k, plan) != plan:
      raise ValueError(f"{path}: plan for '{k}' conflicts with an already loaded table of config {ck}")
    table[k] = plan
  return ck


def select_plans(rows=None, latent=None, dtype=None):
  """Makes the table of one step configuration the active one (none when no table is
  registered for it, or when called without arguments).  Returns the previous selection."""
  prev = _active_cfg()
  ck = None if rows is None else _cfg_key(rows, latent, dtype)
  _TLS.active_cfg = ck
  _TLS.active = _TABLES.get(ck, {}) if ck is not None else {}
  return prev


class plan_scope:
  """`with plan_scope(rows, latent, dtype): ...` -- the launches inside use that table."""

  def __init__(self, rows, latent, dtype):
    self._cfg = (rows, latent, dtype)

  def __enter__(self):
    self._prev = select_plans(*self._cfg)
    return self

  def __exit__(self, *exc):
    if self._prev is None:
      select_plans()
    else:
      select_plans(*self._prev)
    return False


def set_plan(key, plan):
  """Edits the ACTIVE table: plan = (tile, split_k) or None to drop the override
  (tools/tune_step_plans.py)."""
  cfg = _active_cfg()
  if cfg is None:
    raise RuntimeError("set_plan: no configuration selected (select_plans first)")
  table = _TABLES.setdefault(cfg, {})
  if plan is None:
    table.pop(key, None)
  else:
    table[key] = (int(plan[0]), int(plan[1]))
  select_plans(*cfg)


def gemm_plans(rows=None, latent=None, dtype=None):
  """Copy of one configuration's table (the active one by default)."""
  if rows is None:
    return dict(_active())
  return dict(_TABLES.get(_cfg_key(rows, latent, dtype), {}))


def plan_tables():
  return {k: dict(v) for k, v in _TABLES.items()}


def clear_plans():
  _TABLES.clear()
  select_plans()


def record_plan_keys(sink):
  """While `sink` is a dict, every auto-planned ldm_gemm launch stores key -> (M, N, K, batch,
  act, dtype) in it (tools/tune_step_plans.py enumerates a step's problems this way)."""
  global _PLAN_RECORD
  _PLAN_RECORD = sink


def plan_candidates(M, N, K, batch, act, dtype, key=None):
  """(tile, split_k) pairs worth timing for one problem (`key`: its plan key, which carries the conv
  geometry the halo-staged tiles depend on)."""
  ktiles = K // (64 if dtype == BF16 else 32)
  out = []
  for tile, (bm, bn, res) in _TILE_DIMS.items():
    if ((tile in _HALO_RING_TILES and not (dtype == BF16 and batch == 1 and _halo_ring_key(key, M, N, bn))) or
        (act == ACT_GEGLU and tile not in _GEGLU_TILES) or (tile in _BF16_TILES and dtype != BF16) or
        (tile in _WHOLE_N_TILES and N % bn != 0)):
      continue
    tiles = -(-M // bm) * -(-N // bn) * batch
    if tile in _PERSISTENT_TILES:
      if N % bn == 0 and batch == 1 and tiles >= 128 and " x2" not in (key or ""):
        out.append((tile, 1))
      continue
    out.append((tile, 1))
    if batch == 1 and tiles < 256 * res:         # sub-round launches: split-K candidates
      out += [(tile, s) for s in (2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24)
              if ktiles // s >= 4 and tiles * s <= 512 * res]
  return out


def _load_default_plans():
  d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plans")
  if os.path.isdir(d) and os.environ.get("LDM_NO_PLANS") is None:
    for name in sorted(os.listdir(d)):
      if name.endswith(".json"):
        load_plans(os.path.join(d, name))
  extra = os.environ.get("LDM_GEMM_PLANS")
  if extra:
    load_plans(extra)


_load_default_plans()


def resolve_plan(p: GemmParams):
  """Applies the active plan table to an auto-planned problem (tile == 0 and split_k == 0); True if
  the table supplied the plan."""
  active = _active()
  if p.tile == 0 and p.split_k == 0 and not p.ln_out and (active or _PLAN_RECORD is not None):
    key = plan_key(p)
    if _PLAN_RECORD is not None:
      _PLAN_RECORD[key] = (p.M, p.N, p.K, p.batch, p.act, p.dtype)
    plan = active.get(key)
    if plan is None and p.ln_cs:
      # a LayerNorm-fold launch without an entry of its own inherits the plain product's plan when
      # that names a persistent tile
      plan = active.get(key[:-len(" ln1")])
      if plan is not None and plan[0] not in _PERSISTENT_TILES:
        plan = None
    if plan is not None:
      p.tile, p.split_k = plan
      return True
  return False


class PendingReduce:
  """A split-K product whose float32 slabs wait in the workspace (ldm_gemm with defer_reduce): complete it
  with `finish` (plain reduce) or `groupnorm(..., pending=...)` (reduce + GroupNorm in one launch) before
  anything else uses that workspace or reads `out`."""

  def __init__(self, p, out, ws, keep):
    self.p, self.out, self.ws, self.keep, self.done = p, out, ws, keep, False


def _outstanding():
  st = getattr(_TLS, "pending", None)
  if st is None:
    st = _TLS.pending = {}
  return st


def finish(pending):
  """Completes a deferred split-K product with the plain reduce + epilogue launch."""
  if pending is None or pending.done:
    return
  check(lib.ldm_gemm_reduce(C.byref(pending.p), _stream()), "ldm_gemm_reduce")
  pending.done = True
  _outstanding().pop(pending.ws.data_ptr(), None)


def _launch(p: GemmParams, device, defer=None):
  """The one ldm_gemm launch sequence: this thread's workspace, the plan table's (tile, split) if it has one, the
  launch.  With `defer` = (out, keep) a split-K plan leaves its slabs in the workspace: returns its PendingReduce."""
  ws = workspace(device)
  if ws.data_ptr() in _outstanding():
    raise RuntimeError("ldm_gemm: this workspace still holds the slabs of a deferred split-K product "
                       "(ops.finish it, or let the GroupNorm that follows consume it, first)")
  p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
  planned = resolve_plan(p)
  while True:
    split = defer is not None and lib.ldm_gemm_splits(C.byref(p)) > 1
    p.defer_reduce = int(split)
    st = lib.ldm_gemm(C.byref(p), _stream())
    if st in (_lib.ERR_ARG, _lib.ERR_WORKSPACE) and planned:
      # A plan key names the shape, not the epilogue: the table's persistent / halo tile exists only for the epilogue
      # variants that are instantiated.  A launch that shares a key with a tuned one but not its epilogue runs once
      # more, on the cost model.  Nothing was enqueued by the rejected call (argument checks precede every launch).
      planned, p.tile, p.split_k = False, 0, 0
      continue
    check(st, "ldm_gemm")
    if split:
      _outstanding()[ws.data_ptr()] = pend = PendingReduce(p, defer[0], ws, defer[1])
      return pend
    return None


def _gemm_deferred(p: GemmParams, device, out, keep):
  """ldm_gemm with the reduce left to the caller: a PendingReduce, or None when the plan does not split K."""
  return _launch(p, device, (out, keep))


def _gemm(p: GemmParams, device):
  """Every ldm_gemm launch of the package goes through here (tools/gemm_hooks.py wraps this
  one function for measurements; the product path itself carries no hooks)."""
  _launch(p, device)


def linear_ln_supported(n_out, dtype):
  """True if `linear(..., ln=...)` can emit the LayerNorm of its output rows in the same launch."""
  return bool(lib.ldm_gemm_ln_supported(int(n_out), code(dtype)))


def _row_params(x, wt, out, M, N, K, bias=None, addend=None, add_rows=0, residual=None, x2=None, act=ACT_NONE,
                alpha=1.0, tile=0, split_k=0):
  """GemmParams of a batch-1 product with a row-major output; `x2` [M rows] holds the last columns of K (ldm_gemm a2)."""
  p = GemmParams()
  p.a, p.w, p.out = _ptr(x), _ptr(wt), _ptr(out)
  p.bias = _ptr(_f32(bias, "bias"))
  p.addend = _ptr(_f32(addend, "addend"))
  p.residual = _ptr(residual)
  if residual is not None:
    assert residual.dtype == out.dtype
    p.ldr = row_ld(residual)
  p.lda, p.ldc_m, p.ldc_n = row_ld(x), row_ld(out), 1
  p.M, p.N, p.K, p.batch = M, N, K, 1
  if x2 is not None:
    assert x2.dtype == x.dtype and x2.numel() // x2.shape[-1] == M
    p.a2, p.lda2, p.Cin2 = _ptr(x2), row_ld(x2), x2.shape[-1]
  if addend is not None:
    p.add_rows = add_rows
    p.add_ld = addend.stride(0) if (addend.dim() == 2 and addend.shape[0] > 1) else 0
  p.act, p.dtype, p.out_dtype, p.alpha = act, code(x.dtype), code(out.dtype), alpha
  p.tile, p.split_k = tile, split_k
  return p


def linear(x, wt, out, bias=None, act=ACT_NONE, residual=None, addend=None, add_rows=0,
           alpha=1.0, tile=0, split_k=0, ln=None, out2=None, ln_fold=None, x2=None, defer_reduce=False):
  """out[..., n] = act(alpha * x[..., :] . wt[n, :] + bias[n] + addend[group]) + residual.
  x [..., K]; wt [N, K] contiguous; out [..., N] (N/2 wide for GEGLU).
  `ln=(gamma, beta, ln_out, eps)`: also writes ln_out = LayerNorm(out) (same shape/dtype).
  `out2` [G, N2, T']: the weight rows beyond out's width are a second projection whose result is
  stored TRANSPOSED per group of T = M/G rows (q|k into `out`, v into the attention kernel's
  V^T [rows, heads*Sp, T] in one launch).
  `x2` [..., K2]: out = x . wt[:, :K]^T + x2 . wt[:, K:]^T + ...: two products over the same rows as ONE launch.
  `defer_reduce`: as conv3x3's -- a split-K plan leaves its slabs to the caller (returns a PendingReduce or None).
  `ln_fold=(cs, eps)`: out = LayerNorm(x) . W^T + b with the normalisation folded into the product:
  `wt` holds gamma (.) W, `bias` holds b + W beta, cs[n] = sum_k wt[n, k] (layout.ln_fold); the kernel
  derives the row statistics itself (bf16, persistent tiles)."""
  K1, K2 = x.shape[-1], (0 if x2 is None else x2.shape[-1])
  K, N, M = K1 + K2, wt.shape[0], x.numel() // K1
  assert wt.shape[1] == K and wt.is_contiguous() and wt.dtype == x.dtype
  p = _row_params(x, wt, out, M, N, K, bias, addend, add_rows if add_rows > 0 else M, residual, x2, act, alpha, tile, split_k)
  if out2 is not None:
    assert out2.dtype == out.dtype and out2.dim() == 3 and out2.stride(2) == 1 and M % out2.shape[0] == 0
    assert out.shape[-1] + out2.shape[1] == N and out2.shape[2] >= M // out2.shape[0]
    p.out2, p.n_split, p.rows2 = _ptr(out2), out.shape[-1], M // out2.shape[0]
    p.ld2, p.stride2 = out2.stride(1), out2.stride(0)
  if ln is not None:
    gamma, beta, ln_out, eps = ln
    assert ln_out.dtype == out.dtype and tuple(ln_out.shape) == tuple(out.shape)
    p.ln_out, p.ld_ln, p.ln_eps = _ptr(ln_out), row_ld(ln_out), float(eps)
    p.ln_gamma, p.ln_beta = _ptr(_f32(gamma, "ln gamma")), _ptr(_f32(beta, "ln beta"))
  if ln_fold is not None:
    cs, eps = ln_fold
    assert bias is not None and tuple(cs.shape) == (N,) and cs.is_contiguous()
    p.ln_cs, p.ln_eps = _ptr(_f32(cs, "ln_fold column sums")), float(eps)
  if defer_reduce:
    # -> PendingReduce when the plan splits K (the caller owes `finish` or a consuming groupnorm), else None
    return _gemm_deferred(p, x.device, out, (x, wt, bias, addend, residual, x2))
  _gemm(p, x.device)
  return out


def linear_t_shape_supported(dtype, K, N, rows, ld, stride):
  """`linear_t_supported` of shapes alone: `rows` per group, the transposed output's row length `ld` and group
  stride `stride` (persistent kernel: bf16, N a multiple of 128 or 160, groups of rows that are multiples of 32)."""
  return (dtype == torch.bfloat16 and K % 64 == 0 and (N % 128 == 0 or N % 160 == 0) and rows % 32 == 0 and
          ld % 8 == 0 and stride % 8 == 0)


def linear_t_supported(x, wt, out_t):
  """True if `linear_t` can run this product."""
  K, N = x.shape[-1], wt.shape[0]
  M = x.numel() // K
  G = out_t.shape[0]
  return (out_t.dtype == x.dtype and M % G == 0 and out_t.stride(2) == 1 and
          linear_t_shape_supported(x.dtype, K, N, M // G, out_t.stride(1), out_t.stride(0)))


def linear_t(x, wt, out_t, tile=0, bias=None, ln_fold=None):
  """out_t[g, n, t] = sum_k x[g * T + t, k] * wt[n, k] with T = M / G: the product stored
  TRANSPOSED per group of T rows (the self-attention V projection lands directly in the attention
  kernel's V^T [rows, heads*Sp, T]).  Runs on the persistent kernel (_PERSISTENT_TILES; the plan table
  may name which)."""
  K, N, G = x.shape[-1], wt.shape[0], out_t.shape[0]
  M = x.numel() // K
  assert wt.shape[1] == K and wt.is_contiguous() and wt.dtype == x.dtype
  assert out_t.dim() == 3 and out_t.shape[1] == N and out_t.shape[2] >= M // G
  p = GemmParams()
  p.a, p.w = _ptr(x), _ptr(wt)
  p.out = p.out2 = _ptr(out_t)
  p.lda, p.ldc_m, p.ldc_n = row_ld(x), N, 1
  p.M, p.N, p.K, p.batch = M, N, K, 1
  p.act, p.dtype, p.out_dtype, p.alpha = ACT_NONE, code(x.dtype), code(out_t.dtype), 1.0
  p.n_split, p.rows2, p.ld2, p.stride2 = 0, M // G, out_t.stride(1), out_t.stride(0)
  p.tile = tile
  if ln_fold is not None:                # LayerNorm of the rows folded in (see linear)
    cs, eps = ln_fold
    assert bias is not None and tuple(cs.shape) == (N,) and cs.is_contiguous()
    p.bias = _ptr(_f32(bias, "bias"))
    p.ln_cs, p.ln_eps = _ptr(_f32(cs, "ln_fold column sums")), float(eps)
  resolve_plan(p)
  if p.tile not in _PERSISTENT_TILES:
    by_bn = sorted(_PERSISTENT_TILES, key=lambda t: _TILE_DIMS[t][1])   # the narrowest n-tiles that divide N, else the widest
    p.tile, p.split_k = next((t for t in by_bn if N % _TILE_DIMS[t][1] == 0), by_bn[-1]), 0
  _gemm(p, x.device)
  return out_t


def _conv_params(x, wt, out, bias, stride, upsample, addend, residual, tile, split_k, no_lead_pad=False, x2=None):
  B, H, W, Cin = x.shape
  Cout = wt.shape[0]
  hs, ws_ = (2 * H, 2 * W) if upsample else (H, W)
  pads = 1 if no_lead_pad else 2
  OH, OW = (hs + pads - 3) // stride + 1, (ws_ + pads - 3) // stride + 1
  Cin2 = 0 if x2 is None else x2.shape[-1]
  assert wt.shape[1] == 9 * Cin + Cin2 and wt.is_contiguous() and wt.dtype == x.dtype
  assert tuple(out.shape) == (B, OH, OW, Cout), (tuple(out.shape), (B, OH, OW, Cout))
  assert x2 is None or (tuple(x2.shape[:3]) == (B, OH, OW) and stride == 1 and not upsample)
  p = _row_params(x, wt, out, B * OH * OW, Cout, 9 * Cin + Cin2, bias, addend, OH * OW, residual, x2, tile=tile, split_k=split_k)
  p.conv, p.B, p.H, p.W, p.Cin, p.OH, p.OW = 1, B, H, W, Cin, OH, OW
  p.stride, p.upsample, p.no_lead_pad = stride, int(bool(upsample)), int(bool(no_lead_pad))
  return p


def conv3x3(x, wt, out, bias=None, stride=1, upsample=False, addend=None, residual=None,
            tile=0, split_k=0, no_lead_pad=False, defer_reduce=False, x2=None):
  """3x3 convolution, NHWC, pad 1 (Keras SAME for stride 1; the U-Net's explicit
  pad(1,1)+VALID for stride 2; `no_lead_pad`: the autoencoder's pad (0,1),(0,1)+VALID stride-2
  downsample, autoencoder.py:133), optional fused nearest-2x upsample of the input.
  x [B,H,W,Cin] (channel slice allowed); wt [Cout, 9*Cin] = OHWI; out [B,OH,OW,Cout].
  `x2` [B,H,W,Cin2] (stride 1): out += x2 . wt[:, 9*Cin:]^T at the output pixel -- the ResBlock's 1x1 shortcut
  (unet.py:393-397) inside this convolution's K loop; wt is then [Cout, 9*Cin + Cin2] (layout.conv_shortcut_kernel)."""
  p = _conv_params(x, wt, out, bias, stride, upsample, addend, residual, tile, split_k, no_lead_pad, x2)
  if defer_reduce:
    # -> PendingReduce when the plan splits K (the caller owes `finish` or a consuming groupnorm), else None
    return _gemm_deferred(p, x.device, out, (x, wt, bias, addend, residual))
  _gemm(p, x.device)
  return out


def _up2_params(x, wt4, out, bias, tile, split_k):
  B, H, W, Cin = x.shape
  assert wt4.dim() == 3 and wt4.shape[0] == 4 and wt4.is_contiguous() and wt4.dtype == x.dtype
  Cout = wt4.shape[1]
  assert tuple(out.shape) == (B, 2 * H, 2 * W, Cout), (tuple(out.shape), (B, 2 * H, 2 * W, Cout))
  p = _row_params(x, wt4, out, B * 4 * H * W, Cout, wt4.shape[2], bias, tile=tile, split_k=split_k)
  p.conv, p.B, p.H, p.W, p.Cin, p.OH, p.OW = 1, B, H, W, Cin, 2 * H, 2 * W
  p.stride, p.upsample, p.no_lead_pad = 1, 2, 0
  return p


def conv3x3_up2(x, wt4, out, bias=None, tile=0, split_k=0):
  """conv3x3(x, wt, out, upsample=True) as four 2x2 "phase" convolutions over x itself (ldm_gemm's upsample = 2): the
  same result up to the summation order, at 4/9 of the multiply-adds.  x [B,H,W,Cin] (channel slice allowed);
  wt4 [4, Cout, 4*Cin] = layout.upsample_phase_kernel; out [B,2H,2W,Cout] (channel slice allowed).  Plan key: the
  conv key with `u2` (the tables under plans/ hold nine-tap problems only: these launches run on the cost model)."""
  _gemm(_up2_params(x, wt4, out, bias, tile, split_k), x.device)
  return out


def bmm_nt(a, w, out, alpha=1.0, bias=None, transposed_out=False, tile=0):
  """Batched out[b] = alpha * a[b] @ w[b]^T (+bias).  a [Bt, M, K]; w [Bt, N, K] or
  [N, K] (shared); out [Bt, M, N], or [Bt, N, ldn>=M] when transposed_out."""
  Bt, M, K = a.shape
  shared = w.dim() == 2
  N = w.shape[-2]
  assert a.stride(-1) == 1 and w.stride(-1) == 1 and out.stride(-1) == 1
  assert w.stride(-2) == K, "weights / second operand rows must be dense"
  p = GemmParams()
  p.a, p.w, p.out = _ptr(a), _ptr(w), _ptr(out)
  p.bias = _ptr(_f32(bias, "bias"))
  p.lda = a.stride(1)
  p.stride_a = a.stride(0)
  p.stride_w = 0 if shared else w.stride(0)
  p.stride_c = out.stride(0)
  if transposed_out:
    p.ldc_m, p.ldc_n = 1, out.stride(1)
  else:
    p.ldc_m, p.ldc_n = out.stride(1), 1
  p.M, p.N, p.K, p.batch = M, N, K, Bt
  p.act, p.dtype, p.out_dtype, p.alpha = ACT_NONE, code(a.dtype), code(out.dtype), alpha
  p.tile = tile
  _gemm(p, a.device)
  return out


def conv3x3_small(x, kernel_hwio, bias, out):
  B, H, W, Cin = x.shape
  Cout = kernel_hwio.shape[-1]
  assert kernel_hwio.is_contiguous() and kernel_hwio.dtype == torch.float32
  check(lib.ldm_conv3x3_small(_ptr(x), row_ld(x), code(x.dtype), _ptr(kernel_hwio),
                              _ptr(_f32(bias, "bias")), _ptr(out), row_ld(out), code(out.dtype),
                              B, H, W, Cin, Cout, _stream()), "ldm_conv3x3_small")
  return out


def groupnorm(x, gamma, beta, out, eps, silu=False, groups=32, partial=None, fused=None, pending=None,
              store_x=True):
  """x, out [B, H, W, C] (channel slices allowed).  Small images take the single-launch
  kernel (`fused`; default: whenever the library supports the shape), large ones the
  partial-sums + apply pair.
  `pending`: x is the output of a deferred split-K product (conv3x3(..., defer_reduce=True)): its reduce +
  epilogue and this GroupNorm run as ONE launch (ldm_groupnorm_splitk); x itself is written only when
  `store_x` (a ResBlock's conv1 output has no other reader)."""
  B, C = x.shape[0], x.shape[-1]
  HW = x.numel() // (B * C)
  if pending is not None and not pending.done:
    same = (pending.out.data_ptr() == x.data_ptr() and tuple(pending.out.shape) == tuple(x.shape) and
            pending.out.stride() == x.stride())
    if same and lib.ldm_groupnorm_splitk_supported(B, HW, C, groups, code(x.dtype)) and row_ld(x) == pending.p.ldc_m:
      assert out.dtype == x.dtype
      check(lib.ldm_groupnorm_splitk(_byref(pending.p), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")),
                                     _ptr(out), row_ld(out), B, HW, groups, float(eps), int(bool(silu)),
                                     int(bool(store_x)), _stream()), "ldm_groupnorm_splitk")
      pending.done = True
      _outstanding().pop(pending.ws.data_ptr(), None)
      return out
    finish(pending)
  if fused is None:
    fused = True
  if fused and lib.ldm_groupnorm_fused_supported(B, HW, C, groups, code(x.dtype)):
    assert out.dtype == x.dtype
    check(lib.ldm_groupnorm_fused(_ptr(x), row_ld(x), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")),
                                  _ptr(out), row_ld(out), B, HW, C, groups, float(eps), int(bool(silu)),
                                  code(x.dtype), _stream()), "ldm_groupnorm_fused")
    return out
  nch = lib.ldm_groupnorm_nchunks(B, HW, C)
  if partial is None:
    partial = torch.empty(B * nch * groups * 2, dtype=torch.float32, device=x.device)
  assert partial.numel() >= B * nch * groups * 2
  dt = code(x.dtype)
  assert out.dtype == x.dtype
  check(lib.ldm_groupnorm_partial(_ptr(x), row_ld(x), _ptr(partial), B, HW, C, groups, nch, dt,
                                  _stream()), "ldm_groupnorm_partial")
  check(lib.ldm_groupnorm_apply(_ptr(x), row_ld(x), _ptr(partial), _ptr(_f32(gamma, "gamma")),
                                _ptr(_f32(beta, "beta")), _ptr(out), row_ld(out), B, HW, C, groups,
                                nch, float(eps), int(bool(silu)), dt, _stream()),
        "ldm_groupnorm_apply")
  return out


def layernorm(x, gamma, beta, out, eps=1e-5):
  Cc = x.shape[-1]
  rows = x.numel() // Cc
  assert out.dtype == x.dtype
  check(lib.ldm_layernorm(_ptr(x), row_ld(x), _ptr(_f32(gamma, "gamma")), _ptr(_f32(beta, "beta")),
                          _ptr(out), row_ld(out), rows, Cc, float(eps), code(x.dtype), _stream()),
        "ldm_layernorm")
  return out


def softmax_rows(x, out, scale=1.0):
  cols = x.shape[-1]
  rows = x.numel() // cols
  check(lib.ldm_softmax_rows(_ptr(x), row_ld(x), code(x.dtype), _ptr(out), row_ld(out),
                             code(out.dtype), rows, cols, float(scale), _stream()),
        "ldm_softmax_rows")
  return out


def attention(q, k, vt, out, heads, sp, scale, matrix_softmax=False):
  """q [R, Tq, heads*sp], k [R, Tk, heads*sp], vt [R, heads*sp, ldvt>=Tk], out like q.
  `matrix_softmax`: ldm_attention_ms (bf16, 40-wide heads padded to 48): q pre-scaled into the exp2
  domain, k[..., 40] = 1 and V^T row 40 = 1 per head (layout.MS_DIM; the projections' biases put them
  there), `scale` is not used."""
  R, Tq = q.shape[0], q.shape[1]
  Tk = k.shape[1]
  assert q.dtype == k.dtype == vt.dtype == out.dtype
  assert vt.shape[1] == heads * sp and vt.stride(2) == 1
  if matrix_softmax:
    check(lib.ldm_attention_ms(_ptr(q), q.stride(1), q.stride(0), _ptr(k), k.stride(1), k.stride(0),
                               _ptr(vt), vt.stride(1), vt.stride(0), _ptr(out), out.stride(1),
                               out.stride(0), R, heads, Tq, Tk, sp, code(q.dtype), _stream()), "ldm_attention_ms")
    return out
  check(lib.ldm_attention(_ptr(q), q.stride(1), q.stride(0), _ptr(k), k.stride(1), k.stride(0),
                          _ptr(vt), vt.stride(1), vt.stride(0), _ptr(out), out.stride(1),
                          out.stride(0), R, heads, Tq, Tk, sp, float(scale), code(q.dtype),
                          _stream()), "ldm_attention")
  return out


def ffn_geglu_supported(x):
  Cc = x.shape[-1]
  return bool(lib.ldm_ffn_geglu_supported(x.numel() // Cc, Cc, code(x.dtype)))


def ffn_geglu(x, w1, aux, w2, b2, out, eps):
  """out = x + b2 + W2 (a * gelu(g)), (a | g) = W1 LayerNorm(x) + b1: the transformer block's feed-forward as
  one launch per 128-row panel (ldm_ffn_geglu: bf16, C = 320).  w1 / aux from layout.ln_fold + layout.ffn_aux."""
  Cc = x.shape[-1]
  M = x.numel() // Cc
  assert out.dtype == x.dtype and tuple(out.shape) == tuple(x.shape)
  assert tuple(w1.shape) == (8 * Cc, Cc) and tuple(w2.shape) == (Cc, 4 * Cc) and w1.is_contiguous() and w2.is_contiguous()
  assert aux.dtype == torch.float32 and aux.numel() == 8 * Cc * 2 and aux.is_contiguous()
  check(lib.ldm_ffn_geglu(_ptr(x), row_ld(x), _ptr(w1), _ptr(aux), _ptr(w2), _ptr(_f32(b2, "b2")), _ptr(out),
                          row_ld(out), M, Cc, float(eps), code(x.dtype), _stream()), "ldm_ffn_geglu")
  return out


def st_tail(att, wo, bo, r0, w1, aux, w2, b2, wp, bp, r1, out, eps):
  """out = r1 + bp + Wp y,  y = feed-forward(h),  h = r0 + bo + Wo att: the o-projection of the cross-attention, the
  transformer block's feed-forward and the SpatialTransformer's proj_out as ONE row-panel launch (ldm_st_tail:
  bf16, C = 320, attention width 384).  h and y never reach HBM."""
  Cc = out.shape[-1]
  K0 = att.shape[-1]
  M = out.numel() // Cc
  assert att.numel() // K0 == M and att.dtype == out.dtype == r0.dtype == r1.dtype
  assert tuple(wo.shape) == (Cc, K0) and tuple(wp.shape) == (Cc, Cc) and wo.is_contiguous() and wp.is_contiguous()
  assert tuple(w1.shape) == (8 * Cc, Cc) and tuple(w2.shape) == (Cc, 4 * Cc) and w1.is_contiguous() and w2.is_contiguous()
  assert aux.dtype == torch.float32 and aux.numel() == 8 * Cc * 2 and aux.is_contiguous()
  check(lib.ldm_st_tail(_ptr(att), row_ld(att), K0, _ptr(wo), _ptr(_f32(bo, "bo")), _ptr(r0), row_ld(r0), _ptr(w1),
                        _ptr(aux), _ptr(w2), _ptr(_f32(b2, "b2")), _ptr(wp), _ptr(_f32(bp, "bp")), _ptr(r1), row_ld(r1),
                        _ptr(out), row_ld(out), M, Cc, float(eps), code(out.dtype), _stream()), "ldm_st_tail")
  return out


def st_xtail(q, ctx_k, ctx_vt, wo, bo, r0, w1, aux, w2, b2, wp, bp, r1, out, eps):
  """st_tail with the cross-attention in front: q [R, T, 384] are the queries, ctx_k [R, Tk, 384] / ctx_vt
  [R, 384, ld] the context keys / values^T, all in the matrix-side-softmax layout of ops.attention(...,
  matrix_softmax=True); the attention output lives only in LDS (ldm_st_xtail)."""
  Cc, K0 = out.shape[-1], q.shape[-1]
  R, T = q.shape[0], q.shape[1]
  M = R * T
  assert q.dim() == 3 and q.is_contiguous() and ctx_k.is_contiguous() and ctx_vt.is_contiguous()
  assert ctx_k.shape[0] == R and ctx_k.shape[2] == K0 and tuple(ctx_vt.shape[:2]) == (R, K0)
  assert out.numel() // Cc == M and q.dtype == out.dtype == r0.dtype == r1.dtype == ctx_k.dtype == ctx_vt.dtype
  assert tuple(wo.shape) == (Cc, K0) and tuple(wp.shape) == (Cc, Cc) and wo.is_contiguous() and wp.is_contiguous()
  assert tuple(w1.shape) == (8 * Cc, Cc) and tuple(w2.shape) == (Cc, 4 * Cc) and w1.is_contiguous() and w2.is_contiguous()
  assert aux.dtype == torch.float32 and aux.numel() == 8 * Cc * 2 and aux.is_contiguous()
  check(lib.ldm_st_xtail(_ptr(q), K0, K0, _ptr(ctx_k), _ptr(ctx_vt), ctx_k.shape[1], ctx_vt.shape[2], T, _ptr(wo),
                         _ptr(_f32(bo, "bo")), _ptr(r0), row_ld(r0), _ptr(w1), _ptr(aux), _ptr(w2), _ptr(_f32(b2, "b2")),
                         _ptr(wp), _ptr(_f32(bp, "bp")), _ptr(r1), row_ld(r1), _ptr(out), row_ld(out), M, Cc, float(eps),
                         code(out.dtype), _stream()), "ldm_st_xtail")
  return out


def st_block(att, wo1, bo1, r0, wq, qcs, qb, ctx_k, ctx_vt, wo2, bo2, w1, aux, w2, b2, wp, bp, r1, out, eps):
  """From the self-attention's output to the SpatialTransformer's output in ONE launch (ldm_st_block): o-projection
  + residual r0, LayerNorm-folded query projection, cross-attention against ctx_k / ctx_vt, o-projection + residual,
  feed-forward, proj_out + residual r1.  att [R, T, 384]; layouts as st_xtail / linear(ln_fold=...).
  `out` / the context may cover TWICE the rows of att / r0 / r1 (a classifier-free-guidance pair whose two halves
  are still identical in front of this launch): output row m >= R T reads input row m - R T."""
  Cc, K0 = out.shape[-1], att.shape[-1]
  Rin, T = att.shape[0], att.shape[1]
  R = ctx_k.shape[0]
  M = R * T
  assert R in (Rin, 2 * Rin) and r0.numel() // Cc == Rin * T and r1.numel() // Cc == Rin * T
  assert att.dim() == 3 and att.is_contiguous() and ctx_k.is_contiguous() and ctx_vt.is_contiguous()
  assert ctx_k.shape[0] == R and ctx_k.shape[2] == K0 and tuple(ctx_vt.shape[:2]) == (R, K0)
  assert out.numel() // Cc == M and att.dtype == out.dtype == r0.dtype == r1.dtype == ctx_k.dtype == ctx_vt.dtype
  for w_, shp in ((wo1, (Cc, K0)), (wq, (K0, Cc)), (wo2, (Cc, K0)), (wp, (Cc, Cc)), (w1, (8 * Cc, Cc)), (w2, (Cc, 4 * Cc))):
    assert tuple(w_.shape) == shp and w_.is_contiguous() and w_.dtype == out.dtype
  assert aux.dtype == torch.float32 and aux.numel() == 8 * Cc * 2 and aux.is_contiguous()
  assert qcs.dtype == torch.float32 and qcs.numel() == K0
  check(lib.ldm_st_block(_ptr(att), K0, K0, _ptr(wo1), _ptr(_f32(bo1, "bo1")), _ptr(r0), row_ld(r0), _ptr(wq), _ptr(qcs),
                         _ptr(_f32(qb, "qb")), _ptr(ctx_k), _ptr(ctx_vt), ctx_k.shape[1], ctx_vt.shape[2], T, _ptr(wo2),
                         _ptr(_f32(bo2, "bo2")), _ptr(w1), _ptr(aux), _ptr(w2), _ptr(_f32(b2, "b2")), _ptr(wp),
                         _ptr(_f32(bp, "bp")), _ptr(r1), row_ld(r1), _ptr(out), row_ld(out), M, Rin * T, Cc, float(eps),
                         code(out.dtype), _stream()), "ldm_st_block")
  return out


def time_embedding(out, channels, t_rows=None, steps=None, index=None):
  rows = out.shape[0]
  check(lib.ldm_time_embedding(_ptr(t_rows), _ptr(steps), _ptr(index), _ptr(_f32(out, "out")), rows,
                               channels, _stream()), "ldm_time_embedding")
  return out


def select_row(table, index, out, pre_decrement=False):
  """out[0, :] = table[*index, :] (float32); `pre_decrement`: *index is decremented first (the DDIM loop's
  device-side counter moves in the step's first launch)."""
  assert table.dim() == 2 and table.stride(1) == 1 and out.is_contiguous() and out.numel() == table.shape[1]
  assert index.dtype == torch.int32
  check(lib.ldm_select_row(_ptr(_f32(table, "table")), table.stride(0), table.shape[0], table.shape[1], _ptr(index),
                           int(bool(pre_decrement)), _ptr(_f32(out, "out")), _stream()), "ldm_select_row")
  return out


def gemv(x, wt, bias, y, act_in=ACT_NONE, act_out=ACT_NONE):
  """y[r, n] = act_out(sum_k act_in(x[r, k]) wt[n, k] + bias[n]); x, y float32."""
  rows, K = x.shape
  N = wt.shape[0]
  assert wt.shape[1] == K and wt.is_contiguous()
  check(lib.ldm_gemv(_ptr(_f32(x, "x")), x.stride(0), _ptr(wt), _ptr(_f32(bias, "bias")),
                     _ptr(_f32(y, "y")), y.stride(0), rows, N, K, act_in, act_out, code(wt.dtype),
                     _stream()), "ldm_gemv")
  return y


def _update_dims(xt, index, x_unet_out, ring=None, start=None):
  """The asserts every cfg_*_update wrapper shares -> (B, n_per_sample, the dtype code of x_unet_out)."""
  B = xt.shape[0]
  assert index.dtype == torch.int32
  if ring is not None:
    assert ring.is_contiguous() and ring.numel() == 4 * xt.numel() and start.dtype == torch.int32
  return B, xt.numel() // B, code(x_unet_out.dtype) if x_unet_out is not None else F32


def _update_ptrs(eps_all, xt, mid, xt_out, pred_x0_out, x_unet_out, xd, coef, index):
  """The leading arguments of every ldm_cfg_*_update; `mid`: what the entry has between xt and xt_out."""
  return (_ptr(_f32(eps_all, "eps_all")), _ptr(_f32(xt, "xt")), *mid, _ptr(_f32(xt_out, "xt_out")),
          _ptr(_f32(pred_x0_out, "pred_x0_out")), _ptr(x_unet_out), xd, _ptr(_f32(coef, "coef")), _ptr(index))


def _blend_args(xt, coef, z0, mask, q_coef, q_noise=None, q_index_stride=0, table=True, q_slots=True):
  """The inpainting blend's asserts and trailing arguments (z0, mask, [q_noise, q_index_stride,] q_coef, channels).
  `table`: Q is read from q_noise (else drawn in the launch); `q_slots`: the entry has the two q_noise arguments."""
  if z0 is not None:
    assert z0.is_contiguous() and z0.numel() == xt.numel()
    assert mask.is_contiguous() and mask.numel() * xt.shape[-1] == xt.numel()
    assert q_coef.is_contiguous() and q_coef.shape == (coef.shape[0], 2)
    if table:
      assert q_noise.is_contiguous() and q_noise.numel() >= (q_coef.shape[0] - 1) * q_index_stride + xt.numel()
  q = () if not q_slots else (_ptr(_f32(q_noise, "q_noise")), int(q_index_stride)) if table else (None, 0)
  return (_ptr(_f32(z0, "z0")), _ptr(_f32(mask, "mask")), *q, _ptr(_f32(q_coef, "q_coef")), xt.shape[-1])


def cfg_ddim_update(eps_all, xt, xt_out, coef, index, guidance_scale, noise=None, x_unet_out=None,
                    dec_index=False, clip_denoised=False, noise_index_stride=0, pred_x0_out=None):
  B, n, xd = _update_dims(xt, index, x_unet_out)
  check(lib.ldm_cfg_ddim_update(
      *_update_ptrs(eps_all, xt, (_ptr(_f32(noise, "noise")), int(noise_index_stride)), xt_out, pred_x0_out,
                    x_unet_out, xd, coef, index),
      int(bool(dec_index)), float(guidance_scale), int(bool(clip_denoised)), B, n, _stream()), "ldm_cfg_ddim_update")
  return xt_out


def cfg_ddim_update_masked(eps_all, xt, xt_out, coef, index, guidance_scale, z0, mask, q_noise, q_coef,
                           noise=None, x_unet_out=None, dec_index=False, clip_denoised=False, noise_index_stride=0,
                           q_index_stride=0, pred_x0_out=None):
  """cfg_ddim_update, then (at *index = idx >= 1) o <- m * q_sample(z0, steps[idx-1], Q[idx-1]) + (1 - m) * o:
  z0 [B,h,w,c], mask [B,h,w] (1 = keep the init image), Q row j at q_noise + j * q_index_stride, q_coef [N,2]."""
  B, n, xd = _update_dims(xt, index, x_unet_out)
  check(lib.ldm_cfg_ddim_update_masked(
      *_update_ptrs(eps_all, xt, (_ptr(_f32(noise, "noise")), int(noise_index_stride)), xt_out, pred_x0_out,
                    x_unet_out, xd, coef, index),
      int(bool(dec_index)), float(guidance_scale), int(bool(clip_denoised)), B, n,
      *_blend_args(xt, coef, z0, mask, q_coef, q_noise, q_index_stride), _stream()), "ldm_cfg_ddim_update_masked")
  return xt_out


def cfg_plms_update(eps_all, xt, xt_out, ring, coef, index, start, guidance_scale, x_unet_out=None, dec_index=False,
                    pred_x0_out=None, z0=None, mask=None, q_noise=None, q_coef=None, q_index_stride=0):
  """CFG + PLMS update (include/ldm_hip.h): the sigma = 0 update of cfg_ddim_update with eps replaced by the
  Adams-Bashforth combination of this step's guided eps and the min(*start - *index, 3) before it.  ring
  [4,B,...] float32 (slot *index & 3 is written, the next j slots are read), start int32 [1] on the device.
  `z0` (with mask [B,h,w], q_noise, q_coef [N,2]): the inpainting blend of cfg_ddim_update_masked, same launch."""
  B, n, xd = _update_dims(xt, index, x_unet_out, ring, start)
  check(lib.ldm_cfg_plms_update(
      *_update_ptrs(eps_all, xt, (_ptr(_f32(ring, "ring")),), xt_out, pred_x0_out, x_unet_out, xd, coef, index),
      _ptr(start), int(bool(dec_index)), float(guidance_scale), B, n,
      *_blend_args(xt, coef, z0, mask, q_coef, q_noise, q_index_stride), _stream()), "ldm_cfg_plms_update")
  return xt_out


def q_sample(x0, noise, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, xt_out, x_unet_out=None,
             index=None, noise_index_stride=0):
  """xt_out[b] = sqrt_ac[t[b]] * x0[b] + sqrt_1m_ac[t[b]] * noise[b] (float32); t int32 [B] on the device;
  `index`: noise row *index of a table with `noise_index_stride`; x_unet_out: [xt; xt] in its own dtype."""
  B = x0.shape[0]
  n = x0.numel() // B
  assert x0.is_contiguous() and xt_out.is_contiguous() and xt_out.numel() == x0.numel()
  assert noise.is_contiguous() and (index is not None or noise.numel() == x0.numel())
  assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B
  assert index is None or index.dtype == torch.int32
  assert sqrt_alphas_cumprod.numel() == sqrt_one_minus_alphas_cumprod.numel()
  assert x_unet_out is None or (x_unet_out.is_contiguous() and x_unet_out.numel() == 2 * x0.numel())
  xd = code(x_unet_out.dtype) if x_unet_out is not None else F32
  check(lib.ldm_q_sample(_ptr(_f32(x0, "x0")), _ptr(_f32(noise, "noise")), int(noise_index_stride), _ptr(index),
                         _ptr(t), _ptr(_f32(sqrt_alphas_cumprod, "sqrt_alphas_cumprod")),
                         _ptr(_f32(sqrt_one_minus_alphas_cumprod, "sqrt_one_minus_alphas_cumprod")),
                         sqrt_alphas_cumprod.numel(), _ptr(_f32(xt_out, "xt_out")), _ptr(x_unet_out), xd, B, n,
                         _stream()), "ldm_q_sample")
  return xt_out


def _rng(rng):
  """The generator state of include/ldm_hip.h: four 32-bit words on the device (int32 storage holds uint32 bits)."""
  assert rng.dtype == torch.int32 and rng.is_contiguous() and rng.numel() == 4
  return _ptr(rng)


def philox_u32(out, rng, stream_word):
  """out [B,...] int32 storage = the raw Philox4x32-10 words of one stream (include/ldm_hip.h)."""
  B = out.shape[0]
  assert out.dtype == torch.int32 and out.is_contiguous()
  check(lib.ldm_philox_u32(_ptr(out), _rng(rng), int(stream_word) & 0xffffffff, B, out.numel() // B, _stream()),
        "ldm_philox_u32")
  return out


def normal_fill(out, rng, stream_word, x_unet_out=None):
  """out [B,...] float32 = the N(0,1) draws of one stream, keyed per global sample index; x_unet_out: [out; out]
  in its own dtype."""
  B = out.shape[0]
  assert out.is_contiguous()
  assert x_unet_out is None or (x_unet_out.is_contiguous() and x_unet_out.numel() == 2 * out.numel())
  xd = code(x_unet_out.dtype) if x_unet_out is not None else F32
  check(lib.ldm_normal_fill(_ptr(_f32(out, "out")), _rng(rng), int(stream_word) & 0xffffffff, B, out.numel() // B,
                            _ptr(x_unet_out), xd, _stream()), "ldm_normal_fill")
  return out


def q_sample_rng(x0, rng, stream_word, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, xt_out, x_unet_out=None):
  """q_sample with its noise drawn in the kernel from stream `stream_word` (a host int)."""
  B = x0.shape[0]
  n = x0.numel() // B
  assert x0.is_contiguous() and xt_out.is_contiguous() and xt_out.numel() == x0.numel()
  assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B
  assert sqrt_alphas_cumprod.numel() == sqrt_one_minus_alphas_cumprod.numel()
  assert x_unet_out is None or (x_unet_out.is_contiguous() and x_unet_out.numel() == 2 * x0.numel())
  xd = code(x_unet_out.dtype) if x_unet_out is not None else F32
  check(lib.ldm_q_sample_rng(_ptr(_f32(x0, "x0")), _rng(rng), int(stream_word) & 0xffffffff, _ptr(t),
                             _ptr(_f32(sqrt_alphas_cumprod, "sqrt_alphas_cumprod")),
                             _ptr(_f32(sqrt_one_minus_alphas_cumprod, "sqrt_one_minus_alphas_cumprod")),
                             sqrt_alphas_cumprod.numel(), _ptr(_f32(xt_out, "xt_out")), _ptr(x_unet_out), xd, B, n,
                             _stream()), "ldm_q_sample_rng")
  return xt_out


def cfg_ddim_update_rng(eps_all, xt, xt_out, coef, index, rng, guidance_scale, x_unet_out=None, dec_index=False,
                        clip_denoised=False, pred_x0_out=None, z0=None, mask=None, q_coef=None):
  """cfg_ddim_update / cfg_ddim_update_masked (`z0`, mask [B,h,w], q_coef [N,2]) with the eta noise and the blend's
  Q drawn in the launch from `rng` (streams ETA_STREAM + *index, Q_STREAM + *index - 1): no tables."""
  B, n, xd = _update_dims(xt, index, x_unet_out)
  check(lib.ldm_cfg_ddim_update_rng(
      *_update_ptrs(eps_all, xt, (_rng(rng),), xt_out, pred_x0_out, x_unet_out, xd, coef, index),
      int(bool(dec_index)), float(guidance_scale), int(bool(clip_denoised)), B, n,
      *_blend_args(xt, coef, z0, mask, q_coef, table=False, q_slots=False), _stream()), "ldm_cfg_ddim_update_rng")
  return xt_out


def cfg_plms_update_rng(eps_all, xt, xt_out, ring, coef, index, start, rng, guidance_scale, x_unet_out=None,
                        dec_index=False, pred_x0_out=None, z0=None, mask=None, q_coef=None):
  """cfg_plms_update with the blend's Q drawn in the launch from `rng` (stream Q_STREAM + *index - 1)."""
  B, n, xd = _update_dims(xt, index, x_unet_out, ring, start)
  check(lib.ldm_cfg_plms_update_rng(
      *_update_ptrs(eps_all, xt, (_ptr(_f32(ring, "ring")),), xt_out, pred_x0_out, x_unet_out, xd, coef, index),
      _ptr(start), _rng(rng), int(bool(dec_index)), float(guidance_scale), B, n,
      *_blend_args(xt, coef, z0, mask, q_coef, table=False, q_slots=False), _stream()), "ldm_cfg_plms_update_rng")
  return xt_out


def _ms_weights(weights, coef):
  """The weight table of ldm_cfg_ms_update: float32 [N,4,4] (N = rows of coef), rows of 16 floats `pitch` apart."""
  assert weights.dim() == 3 and tuple(weights.shape[1:]) == (4, 4) and weights.shape[0] == coef.shape[0]
  assert weights.stride(2) == 1 and weights.stride(1) == 4 and weights.stride(0) >= 16
  return _ptr(_f32(weights, "weights")), weights.stride(0)


def cfg_ms_update(eps_all, xt, xt_out, ring, coef, index, start, weights, guidance_scale, x_unet_out=None,
                  dec_index=False, pred_x0_out=None, z0=None, mask=None, q_noise=None, q_coef=None, q_index_stride=0):
  """CFG + table-weighted multistep update (include/ldm_hip.h): cfg_plms_update with the weights of the step at
  *index with j = min(*start - *index, 3) earlier steps read from weights[*index, j, :j + 1] (float32 [N,4,4] on the
  device) instead of the Adams-Bashforth constants.  Ring, start and the blend as cfg_plms_update."""
  B, n, xd = _update_dims(xt, index, x_unet_out, ring, start)
  check(lib.ldm_cfg_ms_update(
      *_update_ptrs(eps_all, xt, (_ptr(_f32(ring, "ring")),), xt_out, pred_x0_out, x_unet_out, xd, coef, index),
      _ptr(start), *_ms_weights(weights, coef), int(bool(dec_index)), float(guidance_scale), B, n,
      *_blend_args(xt, coef, z0, mask, q_coef, q_noise, q_index_stride), _stream()), "ldm_cfg_ms_update")
  return xt_out


def cfg_ms_update_rng(eps_all, xt, xt_out, ring, coef, index, start, weights, rng, guidance_scale, x_unet_out=None,
                      dec_index=False, pred_x0_out=None, z0=None, mask=None, q_coef=None):
  """cfg_ms_update with the blend's Q drawn in the launch from `rng` (stream Q_STREAM + *index - 1)."""
  B, n, xd = _update_dims(xt, index, x_unet_out, ring, start)
  check(lib.ldm_cfg_ms_update_rng(
      *_update_ptrs(eps_all, xt, (_ptr(_f32(ring, "ring")),), xt_out, pred_x0_out, x_unet_out, xd, coef, index),
      _ptr(start), *_ms_weights(weights, coef), _rng(rng), int(bool(dec_index)), float(guidance_scale), B, n,
      *_blend_args(xt, coef, z0, mask, q_coef, table=False, q_slots=False), _stream()), "ldm_cfg_ms_update_rng")
  return xt_out


def cfg_sched_update(eps_all, xt, xt_out, coef, gtab, index, guided, ring=None, start=None, weights=None, rng=None,
                     x_unet_out=None, dec_index=False, pred_x0_out=None, z0=None, mask=None, q_noise=None,
                     q_coef=None, q_index_stride=0):
  """CFG by a guidance table + multistep update (include/ldm_hip.h): cfg_ms_update with the
  scale read from gtab[*index] (float32 [N] on the device).  `guided` False: the step's eps is the conditional half
  eps_all[B:], the other half is not read.  `weights` None: no history (the DDIM step at sigma = 0; ring and start
  unused).  `rng`: the blend's Q is drawn in the launch (no q_noise).  Ring, start and the blend as cfg_ms_update."""
  if weights is None:
    ring = start = None
  B, n, xd = _update_dims(xt, index, x_unet_out, ring, start)
  assert eps_all.is_contiguous() and eps_all.numel() == 2 * xt.numel()
  assert gtab.is_contiguous() and gtab.numel() == coef.shape[0]
  assert x_unet_out is None or (x_unet_out.is_contiguous() and x_unet_out.numel() == 2 * xt.numel())
  *head, idx = _update_ptrs(eps_all, xt, (_ptr(_f32(ring, "ring")),), xt_out, pred_x0_out, x_unet_out, xd, coef, index)
  wp = _ms_weights(weights, coef) if weights is not None else (None, 0)
  check(lib.ldm_cfg_sched_update(
      *head, _ptr(_f32(gtab, "gtab")), idx, _ptr(start), *wp, None if rng is None else _rng(rng), int(bool(guided)),
      int(bool(dec_index)), B, n,
      *_blend_args(xt, coef, z0, mask, q_coef, q_noise, q_index_stride, table=rng is None), _stream()),
        "ldm_cfg_sched_update")
  return xt_out


def cfg_ddim_invert_update(eps_all, xt, xt_out, coef, index, guided, guidance_scale=1., x_unet_out=None,
                           dec_index=False, pred_x0_out=None):
  """The DDIM step run upwards (include/ldm_hip.h): xt on the level of a_prev = coef[*index, 2]
  -> xt_out on the level of steps[*index].  `guided` False: eps is the conditional half eps_all[B:], the other half
  is not read and `guidance_scale` is ignored.  No noise, clip, history or blend."""
  B, n, xd = _update_dims(xt, index, x_unet_out)
  assert eps_all.is_contiguous() and eps_all.numel() == 2 * xt.numel()
  assert xt_out.numel() == xt.numel() and (pred_x0_out is None or pred_x0_out.numel() == xt.numel())
  assert x_unet_out is None or (x_unet_out.is_contiguous() and x_unet_out.numel() == 2 * xt.numel())
  check(lib.ldm_cfg_ddim_invert_update(
      *_update_ptrs(eps_all, xt, (), xt_out, pred_x0_out, x_unet_out, xd, coef, index), int(bool(guided)),
      int(bool(dec_index)), float(guidance_scale), B, n, _stream()), "ldm_cfg_ddim_invert_update")
  return xt_out


def _window_args(canvas, win, lead, window, stride, what):
  """The shared checks of window_gather / window_fold -> (B, H, W, c, h, w, sy, sx).  canvas [B,H,W,c] (fold:
  [halves,B,H,W,c], `lead` = halves), win = `lead` x [B,nW,h,w,c]; a window or stride outside the canvas is left to
  the launcher (it reports it), every valid grid has the batch's size checked here."""
  (h, w), (sy, sx) = (int(v) for v in window), (int(v) for v in stride)
  B, H, W, c = (int(v) for v in canvas.shape[-4:])
  assert canvas.is_contiguous() and win.is_contiguous(), what
  if 1 <= h <= H and 1 <= w <= W and 1 <= sy <= h and 1 <= sx <= w:
    n_win = (-((h - H) // sy) + 1) * (-((w - W) // sx) + 1)
    assert win.numel() == lead * B * n_win * h * w * c, (what, tuple(win.shape), (lead, B, n_win, h, w, c))
  return B, H, W, c, h, w, sy, sx


def window_gather(canvas, x_win, window, stride):
  """Panorama (include/ldm_hip.h): canvas [B,H,W,c] float32 -> x_win [2,B,nW,h,w,c] (float32 or
  bfloat16), both halves the crops of the `window` = (h, w) grid at `stride` = (sy, sx), last window clamped."""
  assert canvas.dim() == 4, tuple(canvas.shape)
  dims = _window_args(canvas, x_win, 2, window, stride, "window_gather")
  check(lib.ldm_window_gather(_ptr(_f32(canvas, "canvas")), _ptr(x_win), code(x_win.dtype), *dims, _stream()),
        "ldm_window_gather")
  return x_win


def window_fold(eps_win, eps_canvas, window, stride):
  """Panorama: eps_win [halves,B,nW,h,w,c] float32 -> eps_canvas [halves,B,H,W,c] float32, every canvas element the
  float32 mean of the windows covering it (ascending window index, one correctly rounded division); halves 1 or 2."""
  assert eps_canvas.dim() == 5, tuple(eps_canvas.shape)
  halves = int(eps_canvas.shape[0])
  dims = _window_args(eps_canvas, eps_win, halves, window, stride, "window_fold")
  check(lib.ldm_window_fold(_ptr(_f32(eps_win, "eps_win")), _ptr(_f32(eps_canvas, "eps_canvas")), halves, *dims,
                            _stream()), "ldm_window_fold")
  return eps_canvas


def _window_args_ex(canvas, win, lead, window, stride, wrap, what):
  """_window_args for a grid with `wrap` = (wrap_y, wrap_x): a wrapped axis has ceil(L / s) windows."""
  (h, w), (sy, sx), (wy, wx) = (int(v) for v in window), (int(v) for v in stride), (int(bool(v)) for v in wrap)
  B, H, W, c = (int(v) for v in canvas.shape[-4:])
  assert canvas.is_contiguous() and win.is_contiguous(), what
  if 1 <= h <= H and 1 <= w <= W and 1 <= sy <= h and 1 <= sx <= w:
    n = lambda L, l, s, wr: -(-L // s) if wr else -((l - L) // s) + 1
    n_win = n(H, h, sy, wy) * n(W, w, sx, wx)
    assert win.numel() == lead * B * n_win * h * w * c, (what, tuple(win.shape), (lead, B, n_win, h, w, c))
  return B, H, W, c, h, w, sy, sx, wy, wx


def window_gather_ex(canvas, x_win, window, stride, wrap):
  """window_gather with `wrap` = (wrap_y, wrap_x): along a wrapped axis the windows lie at
  i * stride without a clamp and cover the cells modulo the extent."""
  assert canvas.dim() == 4, tuple(canvas.shape)
  dims = _window_args_ex(canvas, x_win, 2, window, stride, wrap, "window_gather_ex")
  check(lib.ldm_window_gather_ex(_ptr(_f32(canvas, "canvas")), _ptr(x_win), code(x_win.dtype), *dims, _stream()),
        "ldm_window_gather_ex")
  return x_win


def window_fold_ex(eps_win, eps_canvas, window, stride, wrap, weights=None):
  """window_fold on the grid of window_gather_ex with `weights` = (wy [h], wx [w]) float32 device tables of positive
  window-profile weights: every canvas element the float32 sum(wy wx v) / sum(wy wx) over the covering windows
  (ascending window index, every operation rounded once).  None: uniform, window_fold's arithmetic."""
  assert eps_canvas.dim() == 5, tuple(eps_canvas.shape)
  halves = int(eps_canvas.shape[0])
  dims = _window_args_ex(eps_canvas, eps_win, halves, window, stride, wrap, "window_fold_ex")
  wy, wx = (None, None) if weights is None else weights
  for t, n, what in ((wy, dims[4], "wy"), (wx, dims[5], "wx")):
    assert t is None or (t.is_contiguous() and t.numel() == n), (what, tuple(t.shape), n)
  check(lib.ldm_window_fold_ex(_ptr(_f32(eps_win, "eps_win")), _ptr(_f32(eps_canvas, "eps_canvas")), halves, *dims,
                               _ptr(_f32(wy, "wy")), _ptr(_f32(wx, "wx")), _stream()), "ldm_window_fold_ex")
  return eps_canvas


def wrap_pad(x, pad, out=None):
  """Circular padding (include/ldm_hip.h): x [B,H,W,c] float32 -> [B,H+2py,W+2px,c] float32,
  `pad` = (py, px), out[b,y,x] = x[b,(y-py) mod H,(x-px) mod W].  `out`: where the result goes (contiguous;
  allocated when omitted)."""
  assert x.dim() == 4 and x.is_contiguous(), (tuple(x.shape), x.stride())
  B, H, W, c = (int(v) for v in x.shape)
  py, px = (int(v) for v in pad)
  shape = (B, H + 2 * max(py, 0), W + 2 * max(px, 0), c)
  if out is None:
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
  elif 0 <= py <= H and 0 <= px <= W:
    assert out.is_contiguous() and tuple(out.shape) == shape, (tuple(out.shape), shape)
  check(lib.ldm_wrap_pad_nhwc(_ptr(_f32(x, "x")), _ptr(_f32(out, "out")), B, H, W, c, py, px, _stream()),
        "ldm_wrap_pad_nhwc")
  return out


def resize_nhwc(x, size, mode, out=None):
  """Latent resize (include/ldm_hip.h): x [B,H,W,c] float32 -> [B,Ho,Wo,c] float32, `size` =
  (Ho, Wo), `mode` "nearest", "bilinear" or "bicubic" (the align_corners=False rules, no antialiasing; an int is
  handed to the launcher as it is).  `out`: where the result goes (contiguous; allocated when omitted)."""
  if isinstance(mode, str):
    if mode not in _lib.RESIZE_MODES:
      raise ValueError(f"resize mode must be one of {tuple(_lib.RESIZE_MODES)}, got {mode!r}")
    mode = _lib.RESIZE_MODES[mode]
  assert x.dim() == 4 and x.is_contiguous(), (tuple(x.shape), x.stride())
  B, H, W, c = (int(v) for v in x.shape)
  Ho, Wo = (int(v) for v in size)
  if out is None:
    out = torch.empty(B, max(Ho, 0), max(Wo, 0), c, dtype=torch.float32, device=x.device)
  elif Ho >= 1 and Wo >= 1:
    assert out.is_contiguous() and tuple(out.shape) == (B, Ho, Wo, c), (tuple(out.shape), (B, Ho, Wo, c))
  check(lib.ldm_resize_nhwc(_ptr(_f32(x, "x")), _ptr(_f32(out, "out")), B, H, W, c, Ho, Wo, int(mode), _stream()),
        "ldm_resize_nhwc")
  return out


def resample_nhwc(x, size, filter="lanczos3", out=None):
  """Antialiased resample (include/ldm_hip.h): x [B,H,W,c] float32 -> [B,Ho,Wo,c] float32, `size`
  = (Ho, Wo), `filter` "triangle", "cubic" or "lanczos3".  The per-axis tables come from resample.device_taps (built
  on the host on first use, cached per extents, filter and device); the W pass's result goes through a scratch
  tensor of this call.  `out`: where the result goes (contiguous; allocated when omitted)."""
  from . import resample as R
  R.check_filter(filter, "resample filter")
  assert x.dim() == 4 and x.is_contiguous(), (tuple(x.shape), x.stride())
  B, H, W, c = (int(v) for v in x.shape)
  Ho, Wo = (int(v) for v in size)
  if Ho < 1 or Wo < 1:
    raise ValueError(f"resample size must be positive, got {(Ho, Wo)}")
  if out is None:
    out = torch.empty(B, Ho, Wo, c, dtype=torch.float32, device=x.device)
  else:
    assert out.is_contiguous() and tuple(out.shape) == (B, Ho, Wo, c), (tuple(out.shape), (B, Ho, Wo, c))
  _ptr(x)                                        # (a host tensor is refused before any table is built)
  xs, xw, xt = R.device_taps(W, Wo, filter, x.device)
  ys, yw, yt = R.device_taps(H, Ho, filter, x.device)
  tmp = torch.empty(B, H, Wo, c, dtype=torch.float32, device=x.device)
  check(lib.ldm_resample_nhwc(_ptr(_f32(x, "x")), _ptr(tmp), _ptr(_f32(out, "out")), B, H, W, c, Ho, Wo, _ptr(xs),
                              _ptr(xw), xt, _ptr(ys), _ptr(yw), yt, _stream()), "ldm_resample_nhwc")
  return out


_pushpull_ws = {}


def pushpull_fill(x, keep, out=None, lds_tail=True):
  """Push-pull hole filling (include/ldm_hip.h): x [B,H,W,c] float32, keep [B,H,W] float32 (1 =
  keep) -> [B,H,W,c] float32, the kept cells bit for bit and every other cell a smooth continuation of them.
  `out`: where the result goes (contiguous; allocated when omitted; `x` itself is allowed).  `lds_tail` False gives
  every pyramid level its own launches (same bits).  The workspace is kept per (B, H, W, c, device)."""
  assert x.dim() == 4 and x.is_contiguous(), (tuple(x.shape), x.stride())
  B, H, W, c = (int(v) for v in x.shape)
  assert keep.is_contiguous() and tuple(keep.shape) == (B, H, W), (tuple(keep.shape), (B, H, W))
  if out is None:
    out = torch.empty(B, H, W, c, dtype=torch.float32, device=x.device)
  else:
    assert out.is_contiguous() and tuple(out.shape) == (B, H, W, c), (tuple(out.shape), (B, H, W, c))
  _ptr(x)                                        # (a host tensor is refused before the workspace is made)
  ws = pushpull_workspace(B, H, W, c, x.device)
  check(lib.ldm_pushpull_fill(_ptr(_f32(x, "x")), _ptr(_f32(keep, "keep")), _ptr(_f32(out, "out")), _ptr(ws), B, H, W,
                              c, int(bool(lds_tail)), _stream()), "ldm_pushpull_fill")
  return out


def pushpull_workspace(B, H, W, c, device):
  """pushpull_fill's workspace for this shape on `device`: a float32 tensor of ldm_pushpull_workspace_bytes, made on
  first use and kept (None for a 1 x 1 image, which needs none).  The launcher writes every element before it reads
  it, so what the tensor holds between calls does not matter."""
  key = (B, H, W, c, torch.device(device))
  if key not in _pushpull_ws:
    n = int(lib.ldm_pushpull_workspace_bytes(B, H, W, c))
    _pushpull_ws[key] = torch.empty(n // 4, dtype=torch.float32, device=device) if n else None
  return _pushpull_ws[key]


_feather_ws = {}
_stats_ws = {}


def _keep_arg(keep, B, H, W, what):
  """A [B,H,W] or [1,H,W] float32 map as (tensor, batch stride): the one map is read for every sample."""
  assert keep.dim() == 3 and keep.is_contiguous() and tuple(keep.shape[1:]) == (H, W) and keep.shape[0] in (1, B), \
      (what, tuple(keep.shape), (B, H, W))
  return _f32(keep, what), (H * W if keep.shape[0] == B and B > 1 else 0)


def mask_feather(keep, sigma, out=None, lds_tile=False):
  """The paste-back's weight map (include/ldm_hip.h): keep [B,H,W] float32 (kept iff >= 1) ->
  w [B,H,W] float32, 0 on every hole, 1 deep inside the kept region, between them a ramp of `sigma` pixels (0 ..
  16; taps by feather.device_taps) that lies inside the kept region; sigma = 0 returns the 0 / 1 map itself.
  `out`: where the result goes (contiguous; allocated when omitted).  `lds_tile` False (the default: the faster form
  where it was measured) runs the four launches through the workspace kept per (B, H, W,
  device), True the one LDS-tiled launch (same bits)."""
  from . import feather as F
  assert keep.dim() == 3 and keep.is_contiguous(), (tuple(keep.shape), keep.stride())
  B, H, W = (int(v) for v in keep.shape)
  r = F.feather_radius(sigma)
  if out is None:
    out = torch.empty(B, H, W, dtype=torch.float32, device=keep.device)
  else:
    assert out.is_contiguous() and tuple(out.shape) == (B, H, W), (tuple(out.shape), (B, H, W))
  _ptr(keep)                                     # (a host tensor is refused before the tables are made)
  taps, r = F.device_taps(sigma, keep.device)
  ws = mask_feather_workspace(B, H, W, keep.device)
  check(lib.ldm_mask_feather(_ptr(_f32(keep, "keep")), H * W, _ptr(taps), r, _ptr(_f32(out, "out")), _ptr(ws), B, H, W,
                             int(bool(lds_tile)), _stream()), "ldm_mask_feather")
  return out


def mask_feather_workspace(B, H, W, device):
  """mask_feather's workspace for this shape on `device`: a float32 tensor of ldm_mask_feather_workspace_bytes, made
  on first use and kept.  The launcher writes every element before it reads it."""
  key = (B, H, W, torch.device(device))
  if key not in _feather_ws:
    n = int(lib.ldm_mask_feather_workspace_bytes(B, H, W))
    _feather_ws[key] = torch.empty(max(n // 4, 1), dtype=torch.float32, device=device)
  return _feather_ws[key]


def keep_stats(o, d, keep):
  """Statistics of the kept pixels (include/ldm_hip.h): o, d [B,H,W,c] float32 (c <= 4), keep
  [B,H,W] or [1,H,W] float32 (kept iff >= 1) -> (stats [B,c,5] float64 = n, sum o, sum o^2, sum d, sum d^2 over the kept
  pixels; gain [B,c], offset [B,c] float32 that bring d's mean and variance there to o's).  Fresh tensors every call;
  the partial sums live in a buffer kept per (B, H, W, c, device)."""
  assert o.dim() == 4 and o.is_contiguous(), (tuple(o.shape), o.stride())
  B, H, W, c = (int(v) for v in o.shape)
  assert d.is_contiguous() and tuple(d.shape) == (B, H, W, c), (tuple(d.shape), (B, H, W, c))
  keep, kb = _keep_arg(keep, B, H, W, "keep")
  _ptr(o)
  key = (B, H, W, c, o.device)
  if key not in _stats_ws:
    n = B * max(int(lib.ldm_keep_stats_partials(H, W)), 1) * max(c, 1) * 5
    _stats_ws[key] = torch.empty(n, dtype=torch.float32, device=o.device)
  stats = torch.empty(B, c, 5, dtype=torch.float64, device=o.device)
  gain = torch.empty(B, c, dtype=torch.float32, device=o.device)
  offset = torch.empty(B, c, dtype=torch.float32, device=o.device)
  check(lib.ldm_keep_stats(_ptr(_f32(o, "o")), _ptr(_f32(d, "d")), _ptr(keep), kb, _ptr(_stats_ws[key]), _ptr(stats),
                           _ptr(gain), _ptr(offset), B, H, W, c, _stream()), "ldm_keep_stats")
  return stats, gain, offset


def paste_back(o, d, w, gain=None, offset=None, out=None):
  """The paste-back (include/ldm_hip.h): o, d [B,H,W,c] float32 (the source and the decoded
  images), w [B,H,W] or [1,H,W] float32 -> o where w >= 1 (the bits), d' where w <= 0, fma(w, o - d', d') between,
  d' = gain d + offset per sample and channel ([B,c] float32 each, both or neither; None: d itself, the bits).
  `out`: where the result goes (contiguous; allocated when omitted; `d` itself is allowed)."""
  assert o.dim() == 4 and o.is_contiguous(), (tuple(o.shape), o.stride())
  B, H, W, c = (int(v) for v in o.shape)
  assert d.is_contiguous() and tuple(d.shape) == (B, H, W, c), (tuple(d.shape), (B, H, W, c))
  w, wb = _keep_arg(w, B, H, W, "w")
  for t, what in ((gain, "gain"), (offset, "offset")):
    assert t is None or (t.is_contiguous() and tuple(t.shape) == (B, c)), (what, tuple(t.shape), (B, c))
  if out is None:
    out = torch.empty(B, H, W, c, dtype=torch.float32, device=o.device)
  else:
    assert out.is_contiguous() and tuple(out.shape) == (B, H, W, c), (tuple(out.shape), (B, H, W, c))
  check(lib.ldm_paste_back(_ptr(_f32(o, "o")), _ptr(_f32(d, "d")), _ptr(w), wb, _ptr(_f32(gain, "gain")),
                           _ptr(_f32(offset, "offset")), _ptr(_f32(out, "out")), B, H, W, c, _stream()),
        "ldm_paste_back")
  return out


def latent_preview(lat_a, proj, frames_a, freq, index=None, index_bias=0, lat_b=None, frames_b=None, scale=1,
                   mode="bilinear"):
  """Latent previews (include/ldm_hip.h): lat_a (and lat_b) [B,h,w,c] float32 -> RGB bytes in
  slot r of frames_a (frames_b) [R,B,s*h,s*w,3] uint8, s = `scale`, through proj [c+1,3] float32 (c weight rows, then
  the bias), an upscale (`mode` "nearest" or "bilinear"; an int is handed to the launcher as it is) and the 8-bit
  quantisation.  r = idx / freq for idx = index[0] + index_bias (`index` a device int32 tensor, None = 0) when idx is
  a non-negative multiple of `freq` and r < R; any other idx writes nothing.  The frames may start at any byte."""
  if isinstance(mode, str):
    if mode not in _lib.PREVIEW_MODES:
      raise ValueError(f"preview mode must be one of {tuple(_lib.PREVIEW_MODES)}, got {mode!r}")
    mode = _lib.PREVIEW_MODES[mode]
  assert lat_a.dim() == 4 and lat_a.is_contiguous(), (tuple(lat_a.shape), lat_a.stride())
  B, h, w, c = (int(v) for v in lat_a.shape)
  scale = int(scale)
  assert proj.is_contiguous() and tuple(proj.shape) == (c + 1, 3), (tuple(proj.shape), (c + 1, 3))
  assert frames_a.dim() == 5, tuple(frames_a.shape)
  R = int(frames_a.shape[0])
  shape = (R, B, scale * h, scale * w, 3)
  for lat, frames in ((lat_a, frames_a), (lat_b, frames_b)):
    if frames is not None:
      assert frames.dtype == torch.uint8 and frames.is_contiguous(), (frames.dtype, frames.stride())
      if 1 <= scale <= 16:
        assert tuple(frames.shape) == shape, (tuple(frames.shape), shape)
    if lat is not None:
      assert lat.is_contiguous() and tuple(lat.shape) == (B, h, w, c), (tuple(lat.shape), (B, h, w, c))
  if index is not None:
    assert index.dtype == torch.int32 and index.numel() >= 1
  check(lib.ldm_latent_preview(_ptr(_f32(lat_a, "lat_a")), _ptr(_f32(lat_b, "lat_b")), _ptr(_f32(proj, "proj")),
                               _ptr(frames_a), _ptr(frames_b), _ptr(index), int(index_bias), int(freq), R, B, h, w,
                               c, scale, int(mode), _stream()), "ldm_latent_preview")
  return frames_a


def xattn_map_supported(heads, tk, s, sp, dtype):
  """Whether ldm_xattn_map takes this shape (heads >= 1, 1 <= tk <= 80, s <= sp, sp one of layout.ATTN_SP)."""
  return bool(lib.ldm_xattn_map_supported(int(heads), int(tk), int(s), int(sp), code(dtype)))


def xattn_map(q, k, acc, heads, s, sp, log2_scale, step_w=None, index=None, index_bias=0):
  """Cross-attention heat maps (include/ldm_hip.h): acc [R,T,Tk] (or [R,h,w,Tk], T = h*w) float32
  += w * the mean over heads of softmax_j(log2_scale * q_h . k_h) in the exp2 domain, q [R,T,heads*sp] and
  k [R,Tk,heads*sp] float32 or bf16 with the true head size `s` (the dims from s to sp of every head are not read into
  the products).  q and k may be row slices such as q[B:] and may have a row pitch above heads*sp; acc is contiguous.
  w = step_w[index[0] + index_bias] (`step_w` device float32 [N], `index` a device int32 tensor, None = 0), 1 without
  `step_w`; an index outside the table or a zero weight writes nothing."""
  assert q.dim() == 3 and k.dim() == 3, (tuple(q.shape), tuple(k.shape))
  R, T, hs = (int(v) for v in q.shape)
  Tk = int(k.shape[1])
  assert hs == heads * sp and tuple(k.shape) == (R, Tk, hs), (tuple(q.shape), tuple(k.shape), heads, sp)
  assert q.dtype == k.dtype and q.stride(2) == 1 and k.stride(2) == 1, (q.dtype, k.dtype, q.stride(), k.stride())
  assert acc.dtype == torch.float32 and acc.is_contiguous() and acc.numel() == R * T * Tk and acc.shape[0] == R and \
      acc.shape[-1] == Tk, (acc.dtype, tuple(acc.shape), (R, T, Tk))
  n_w = 0
  if step_w is not None:
    assert step_w.dtype == torch.float32 and step_w.dim() == 1 and step_w.is_contiguous(), (step_w.dtype, step_w.shape)
    n_w = int(step_w.numel())
  if index is not None:
    assert index.dtype == torch.int32 and index.numel() >= 1
  check(lib.ldm_xattn_map(_ptr(q), q.stride(1), q.stride(0), _ptr(k), k.stride(1), k.stride(0), _ptr(acc), R,
                          int(heads), T, Tk, int(s), int(sp), float(log2_scale), code(q.dtype), _ptr(step_w), n_w,
                          _ptr(index), int(index_bias), _stream()), "ldm_xattn_map")
  return acc


def eps_contrast_accum(eps_all, acc, counter=None):
  """DiffEdit's contrast accumulator (include/ldm_hip.h): eps_all [2B,...,c] float32 = [e_src;
  e_tgt], acc [B,...] float32 (one value per cell) += sum_j |e_tgt[j] - e_src[j]| in float32, j ascending.  `counter`
  (a device int32 tensor): decremented by one after the launch has read everything.  Any view of contiguous memory
  passes; c = 4 needs both 16-byte aligned."""
  assert eps_all.is_contiguous() and acc.is_contiguous(), (eps_all.stride(), acc.stride())
  assert eps_all.dim() >= 2 and eps_all.shape[0] % 2 == 0, tuple(eps_all.shape)
  B, c = int(eps_all.shape[0]) // 2, int(eps_all.shape[-1])
  assert B >= 1 and acc.shape[0] == B and acc.numel() * c * 2 == eps_all.numel(), (tuple(eps_all.shape), tuple(acc.shape))
  if counter is not None:
    assert counter.dtype == torch.int32 and counter.numel() >= 1
  check(lib.ldm_eps_contrast_accum(_ptr(_f32(eps_all, "eps_all")), _ptr(_f32(acc, "acc")), _ptr(counter), B,
                                   acc.numel() // B, c, _stream()), "ldm_eps_contrast_accum")
  return acc


def contrast_mask_supported(h, w, dilate=0):
  """Whether ldm_contrast_mask takes this shape (h w <= 65536, dilate in 0..3)."""
  return bool(lib.ldm_contrast_mask_supported(int(h), int(w), int(dilate)))


def contrast_mask(acc, mask_out, tau, dilate=0, mean_out=None, thr_out=None, count_out=None):
  """DiffEdit's mask (include/ldm_hip.h): acc [B,h,w] float32 -> mask_out [B,h,w] float32, 1 =
  keep: edit = acc > tau * mean of the sample, dilated by `dilate` cells, mask = 1 - edit.  mean_out, thr_out float32
  [B] and count_out int32 [B] (the edited cells) are optional."""
  assert acc.dim() == 3 and acc.is_contiguous(), (tuple(acc.shape), acc.stride())
  B, h, w = (int(v) for v in acc.shape)
  assert mask_out.is_contiguous() and tuple(mask_out.shape) == (B, h, w), (tuple(mask_out.shape), (B, h, w))
  for t, dt in ((mean_out, torch.float32), (thr_out, torch.float32), (count_out, torch.int32)):
    assert t is None or (t.dtype == dt and t.is_contiguous() and t.numel() == B), (t.dtype, tuple(t.shape), B)
  check(lib.ldm_contrast_mask(_ptr(_f32(acc, "acc")), _ptr(_f32(mask_out, "mask_out")), _ptr(mean_out), _ptr(thr_out),
                              _ptr(count_out), B, h, w, float(tau), int(dilate), _stream()), "ldm_contrast_mask")
  return mask_out


def store_row(src, table, index, index_sign=1, index_bias=0):
  """table[index_sign * index[0] + index_bias] = src (float32; `index` a device int32 tensor): the inverse of
  select_row.  A row outside the table writes nothing.  table [rows,...] with the rows `src.numel()` floats or more
  apart."""
  assert src.is_contiguous() and table.dim() >= 2 and table[0].is_contiguous() and table[0].numel() == src.numel(), \
      (tuple(src.shape), tuple(table.shape), table.stride())
  assert index.dtype == torch.int32 and index.numel() >= 1
  check(lib.ldm_store_row(_ptr(_f32(src, "src")), _ptr(_f32(table, "table")), table.stride(0), table.shape[0],
                          _ptr(index), int(index_sign), int(index_bias), src.numel(), _stream()), "ldm_store_row")
  return table


def post_quant(latents, scale_factor, kernel_io, bias, out):
  Cc = latents.shape[-1]
  check(lib.ldm_post_quant(_ptr(_f32(latents, "latents")), float(scale_factor),
                           _ptr(_f32(kernel_io, "kernel")), _ptr(_f32(bias, "bias")), _ptr(out),
                           code(out.dtype), latents.numel() // Cc, Cc, _stream()), "ldm_post_quant")
  return out


def gaussian_sample(moments, out, noise=None, out_scale=1.0):
  Cc = out.shape[-1]
  assert moments.shape[-1] == 2 * Cc and moments.is_contiguous() and out.is_contiguous()
  assert noise is None or (noise.is_contiguous() and noise.numel() == out.numel())
  check(lib.ldm_gaussian_sample(_ptr(_f32(moments, "moments")), _ptr(_f32(noise, "noise")),
                                _ptr(_f32(out, "out")), float(out_scale), out.numel() // Cc, Cc,
                                _stream()), "ldm_gaussian_sample")
  return out


def vq_nearest(z, codebook, out, indices=None):
  Cc = z.shape[-1]
  check(lib.ldm_vq_nearest(_ptr(_f32(z, "z")), _ptr(_f32(codebook, "codebook")),
                           _ptr(_f32(out, "out")), _ptr(indices), z.numel() // Cc,
                           codebook.shape[0], Cc, _stream()), "ldm_vq_nearest")
  return out


def embedding(ids, tok_emb, pos_emb, out):
  rows, T = ids.shape
  assert ids.dtype == torch.int64 and ids.is_contiguous()
  check(lib.ldm_embedding(_ptr(ids), _ptr(_f32(tok_emb, "tok_emb")), _ptr(_f32(pos_emb, "pos_emb")),
                          _ptr(out), rows, T, tok_emb.shape[1], tok_emb.shape[0], code(out.dtype),
                          _stream()), "ldm_embedding")
  return out


def minmax_u8(x, out, scratch=None):
  B = x.shape[0]
  n = x.numel() // B
  assert x.is_contiguous() and out.dtype == torch.uint8
  if scratch is None:
    scratch = torch.empty(B * 128, dtype=torch.float32, device=x.device)
  check(lib.ldm_minmax_u8(_ptr(x), code(x.dtype), _ptr(out), _ptr(scratch), B, n, _stream()),
        "ldm_minmax_u8")
  return out


def cast(x, out):
  cols = x.shape[-1]
  rows = x.numel() // cols
  check(lib.ldm_cast(_ptr(x), row_ld(x), code(x.dtype), _ptr(out), row_ld(out), code(out.dtype),
                     rows, cols, _stream()), "ldm_cast")
  return out
