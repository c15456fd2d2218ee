"""ldm_xattn_map against its restatement (tests/attn_map_ref.py).

Gate, the project's "twice the float32 emulation's error" rule: e32 = max |maps32 - maps64| of the exact values handed
to the kernel, delta = max(2 e32, 8 * 2^-24 * w) with w the largest possible entry (the weights of the launches
summed) -- eight half-ulps of it, one per rounding between a logit and the store (exp2, denominator, reciprocal,
product, head sum, 1 / heads, w, accumulate), which also holds a hardware exp2 or reciprocal that is 1 ulp off.  Every
case prints e32, delta and the measured maximum.

The module's name puts it behind the older GPU modules in the collection order, as tests/test_zz_preview_gpu.py does."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_map_ref as A  # noqa: E402
from ldm_tf2_amd import _lib, ops  # noqa: E402

ROWS = 64                                          # queries per workgroup of the kernel (xattn_map.hip kRows)
PAD = 256
CANARY = 12345.5
DTYPES = [torch.float32, torch.bfloat16]


def _dev_pair(dev, q, k, dtype, extra_ld=0):
  """q, k (float32 NumPy [R,T,hs], [R,Tk,hs]) as the UPPER half of [2R, ., hs + extra_ld] device buffers of `dtype`
  (the lower half NaN), so that the batch strides -- and with extra_ld a row pitch above heads*sp -- apply; also the
  exact float32 values of what the kernel reads."""
  out = []
  for a in (q, k):
    R, n, hs = a.shape
    full = torch.full((2 * R, n, hs + extra_ld), float("nan"), dtype=dtype, device=dev)
    full[R:, :, :hs] = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).to(dtype)
    view = full[R:, :, :hs]
    out += [view, view.float().cpu().numpy()]
  return out[0], out[2], out[1], out[3]


def _acc(dev, R, T, Tk, acc0=None):
  buf = torch.full((PAD + R * T * Tk + PAD,), CANARY, dtype=torch.float32, device=dev)
  acc = buf[PAD:PAD + R * T * Tk].view(R, T, Tk)
  if acc0 is None:
    acc.zero_()
  else:
    acc.copy_(torch.from_numpy(np.ascontiguousarray(acc0, np.float32)).to(dev))
  return buf, acc


def _pads_ok(buf):
  return bool((buf[:PAD] == CANARY).all() and (buf[-PAD:] == CANARY).all())


def _inputs(seed, R, T, Tk, heads, S, sp, nan_pad=False, spread=4.0):
  g = np.random.default_rng(seed)
  q = g.standard_normal((R, T, heads * sp)).astype(np.float32)
  k = (spread * g.standard_normal((R, Tk, heads * sp))).astype(np.float32)
  if nan_pad:
    pad = (np.arange(heads * sp) % sp) >= S
    q[..., pad] = np.nan
    k[..., pad] = np.nan
  return q, k


def _check(what, got, q32, k32, heads, S, sp, ls, w, acc0, w_max=None):
  want, e32, delta = A.gate(q32, k32, heads, S, sp, ls, w, acc0)
  delta = max(delta, 8. * 2. ** -24 * (w if w_max is None else w_max))
  err = float(np.abs(got.astype(np.float64) - want).max())
  print(f"{what}: e32={e32:.3e} delta={delta:.3e} max err={err:.3e}")
  assert np.isfinite(got).all(), what
  assert err <= delta, f"{what}: max err {err:.3e} above delta {delta:.3e} (e32 {e32:.3e})"


SHAPES = [(2, 4, 77, 8, 8, 32), (1, 1, 1, 1, 32, 32), (2, 70, 77, 8, 40, 48), (1, 130, 5, 2, 80, 80),
          (1, 64, 80, 8, 160, 160), (1, ROWS - 1, 77, 8, 16, 32), (1, ROWS, 77, 8, 16, 32), (1, ROWS + 1, 77, 8, 16, 32)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,T,Tk,heads,S,sp", SHAPES)
def test_kernel_against_restatement(dev, R, T, Tk, heads, S, sp, dtype):
  assert ops.xattn_map_supported(heads, Tk, S, sp, dtype)
  q, k = _inputs(R + T + Tk + S, R, T, Tk, heads, S, sp)
  ls = S ** -0.5 * 1.4426950408889634
  qd, kd, q32, k32 = _dev_pair(dev, q, k, dtype)
  buf, acc = _acc(dev, R, T, Tk)
  ops.xattn_map(qd, kd, acc, heads, S, sp, ls)
  first = acc.cpu().numpy()
  assert _pads_ok(buf), "a canary beside acc was written"
  _check(f"{(R, T, Tk, heads, S, sp)} {dtype}", first, q32, k32, heads, S, sp, ls, 1., np.zeros_like(first))
  # every row of probabilities sums to 1
  assert np.abs(first.sum(-1) - 1.).max() <= 1e-5
  # the same launch again from zero: bit-identical
  buf2, acc2 = _acc(dev, R, T, Tk)
  ops.xattn_map(qd, kd, acc2, heads, S, sp, ls)
  assert np.array_equal(acc2.cpu().numpy(), first)
  # a second launch into the same acc, with a weight from a table: the restatement started from the first result
  tab = torch.tensor([9., 0.75, 9.], dtype=torch.float32, device=dev)
  idx = torch.tensor([3], dtype=torch.int32, device=dev)
  ops.xattn_map(qd, kd, acc, heads, S, sp, ls, step_w=tab, index=idx, index_bias=-2)
  second = acc.cpu().numpy()
  assert idx.item() == 3 and _pads_ok(buf)
  _check("  second launch", second, q32, k32, heads, S, sp, ls, 0.75, first, w_max=1.75)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_row_pitch_and_unaligned_rows(dev, dtype):
  """ldq / ldk above heads*sp: a pitch that keeps the 16-byte loads (+8 elements) and one that does not (+1, +3)."""
  R, T, Tk, heads, S, sp = 2, 70, 77, 8, 40, 48
  q, k = _inputs(5, R, T, Tk, heads, S, sp)
  ls = S ** -0.5 * 1.4426950408889634
  res = []
  for extra in (0, 8, 1, 3):
    qd, kd, q32, k32 = _dev_pair(dev, q, k, dtype, extra_ld=extra)
    assert qd.stride(1) == heads * sp + extra
    buf, acc = _acc(dev, R, T, Tk)
    ops.xattn_map(qd, kd, acc, heads, S, sp, ls)
    res.append(acc.cpu().numpy())
    assert _pads_ok(buf)
    _check(f"pitch +{extra} {dtype}", res[-1], q32, k32, heads, S, sp, ls, 1., np.zeros_like(res[-1]))
  for r in res[1:]:
    assert np.array_equal(r, res[0])               # the vector and the element loads read the same values


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("S,sp", [(40, 48), (8, 32), (33, 48)])
def test_padded_dims_are_not_read(dev, S, sp, dtype):
  """NaN in every dim d in [S, sp) of q and k: the result is finite and bit for bit what zeros there give."""
  R, T, Tk, heads = 2, 70, 77, 8
  ls = S ** -0.5 * 1.4426950408889634
  res = []
  for nan_pad in (False, True):
    q, k = _inputs(11, R, T, Tk, heads, S, sp, nan_pad=nan_pad)
    if not nan_pad:
      pad = (np.arange(heads * sp) % sp) >= S
      q[..., pad] = 0.
      k[..., pad] = 0.
    qd, kd, q32, k32 = _dev_pair(dev, q, k, dtype)
    buf, acc = _acc(dev, R, T, Tk)
    ops.xattn_map(qd, kd, acc, heads, S, sp, ls)
    res.append(acc.cpu().numpy())
    assert _pads_ok(buf)
  assert np.isfinite(res[1]).all() and np.array_equal(res[0], res[1])
  _check(f"NaN padding S={S} {dtype}", res[1], q32, k32, heads, S, sp, ls, 1., np.zeros_like(res[1]))


def test_launches_that_write_nothing(dev):
  R, T, Tk, heads, S, sp = 2, 70, 77, 8, 40, 48
  q, k = _inputs(13, R, T, Tk, heads, S, sp)
  qd, kd, _, _ = _dev_pair(dev, q, k, torch.float32)
  acc0 = np.random.default_rng(1).standard_normal((R, T, Tk)).astype(np.float32)
  acc0[0, 3, 5] = acc0[1, 69, 76] = np.nan           # canaries inside acc
  tab = torch.tensor([1., 0., 2.], dtype=torch.float32, device=dev)
  for index, bias in ((0, -1), (2, 1), (1, 0), (-5, 2), (0, 3)):      # idx -1, n_w, a zero weight, -3, n_w again
    buf, acc = _acc(dev, R, T, Tk, acc0)
    idx = torch.tensor([index], dtype=torch.int32, device=dev)
    ops.xattn_map(qd, kd, acc, heads, S, sp, 0.2, step_w=tab, index=idx, index_bias=bias)
    got = acc.cpu().numpy()
    assert idx.item() == index
    assert np.array_equal(got.view(np.uint32), acc0.view(np.uint32)), (index, bias)
    assert _pads_ok(buf)
  # index_bias moves the selected weight; no index tensor reads entry index_bias
  outs = {}
  for index, bias in ((0, 0), (0, 2), (1, 1), (None, 2)):
    buf, acc = _acc(dev, R, T, Tk)
    idx = None if index is None else torch.tensor([index], dtype=torch.int32, device=dev)
    ops.xattn_map(qd, kd, acc, heads, S, sp, 0.2, step_w=tab, index=idx, index_bias=bias)
    outs[index, bias] = acc.cpu().numpy()
  assert np.array_equal(outs[0, 2], outs[1, 1]) and np.array_equal(outs[0, 2], outs[None, 2])
  assert np.array_equal(outs[0, 2], 2. * outs[0, 0]) and outs[0, 0].max() > 0


def _probe(R, T, Tk, heads, S, sp, amp):
  """Keys: Tk distinct +-1 sign vectors (the bits of j in dims 0..6, +1 above); q[r,t,h] = amp * k[j*(r,t,h)].  Two
  distinct keys differ in at least one dim, so the winner's logit amp * S leads every other by at least 2 amp."""
  assert 2 ** min(S, 7) >= Tk
  signs = np.ones((Tk, S), np.float32)
  for d in range(min(S, 7)):
    signs[:, d] = np.where((np.arange(Tk) >> d) & 1, 1., -1.)
  r_, t_, h_ = np.meshgrid(np.arange(R), np.arange(T), np.arange(heads), indexing="ij")
  jstar = (t_ * heads + h_ + 3 * r_) % Tk
  one = (t_ % 5 == 0)
  jstar = np.where(one, (7 * t_ + r_) % Tk, jstar)               # some (r, t): all heads on one key
  k = np.full((R, Tk, heads, sp), np.nan, np.float32)
  q = np.full((R, T, heads, sp), np.nan, np.float32)
  k[..., :S] = signs[None, :, None, :]
  q[..., :S] = amp * signs[jstar]
  want = np.zeros((R, T, Tk), np.float64)
  np.add.at(want, (r_, t_, jstar), 1.)
  assert (want.sum(1) > 0).all()                                  # every key is hit in every row
  return q.reshape(R, T, heads * sp), k.reshape(R, Tk, heads * sp), want


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("S,sp", [(8, 32), (40, 48)])
def test_exact_probes(dev, S, sp, dtype):
  """Every p is exactly 1 or 0 (the winner leads by 256 in the log2 domain, exp2 of the rest underflows to 0), so with
  8 heads and w = 0.5, acc[r,t,j] = 0.5 * #{h : j*(r,t,h) = j} / 8 exactly, in both dtypes: every query row, head
  and key is accounted for."""
  R, T, Tk, heads = 2, 70, 77, 8
  q, k, count = _probe(R, T, Tk, heads, S, sp, 128.)
  qd, kd, _, _ = _dev_pair(dev, q, k, dtype)
  buf, acc = _acc(dev, R, T, Tk)
  tab = torch.tensor([0.5], dtype=torch.float32, device=dev)
  ops.xattn_map(qd, kd, acc, heads, S, sp, 1.0, step_w=tab)
  got = acc.cpu().numpy()
  assert _pads_ok(buf)
  assert np.array_equal(got.astype(np.float64), 0.5 * count / heads)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_ranges(dev, dtype):
  R, T, Tk, heads, S, sp = 1, 70, 77, 8, 40, 48
  # logits near +-1e4: finite, and every row still sums to 1
  q, k, _ = _probe(R, T, Tk, heads, S, sp, 1.)
  g = np.random.default_rng(3)
  q = np.nan_to_num(q) * g.uniform(0.5, 1., size=q.shape).astype(np.float32) * 250.
  qd, kd, q32, k32 = _dev_pair(dev, q, np.nan_to_num(k), dtype)
  assert np.abs(np.einsum("rtd,rjd->rtj", q32[..., :S], k32[..., :S])).max() > 5e3
  buf, acc = _acc(dev, R, T, Tk)
  ops.xattn_map(qd, kd, acc, heads, S, sp, 1.0)
  got = acc.cpu().numpy()
  assert np.isfinite(got).all() and np.abs(got.sum(-1) - 1.).max() <= 1e-5 and _pads_ok(buf)
  # all-equal logits: w / Tk in every column
  qd, kd, q32, k32 = _dev_pair(dev, np.zeros_like(q), np.nan_to_num(k), dtype)
  buf, acc = _acc(dev, R, T, Tk)
  ops.xattn_map(qd, kd, acc, heads, S, sp, 1.0)
  got = acc.cpu().numpy()
  _check(f"equal logits {dtype}", got, q32, k32, heads, S, sp, 1.0, 1., np.zeros_like(got))
  assert np.abs(got.astype(np.float64) - 1. / Tk).max() <= 8. * 2. ** -24


def test_argument_errors(dev):
  assert not ops.xattn_map_supported(8, 81, 40, 48, torch.float32)
  assert not ops.xattn_map_supported(8, 77, 40, 40, torch.float32)       # 40 is not a padded head size
  assert not ops.xattn_map_supported(8, 77, 49, 48, torch.float32)
  assert not ops.xattn_map_supported(0, 77, 40, 48, torch.float32)
  assert not ops.xattn_map_supported(8, 0, 40, 48, torch.float32)
  assert ops.xattn_map_supported(1, 80, 160, 160, torch.bfloat16)
  q = torch.zeros(1, 4, 8 * 48, device=dev)
  k = torch.zeros(1, 81, 8 * 48, device=dev)
  acc = torch.zeros(1, 4, 81, device=dev)
  with pytest.raises(_lib.LdmHipError, match="ldm_xattn_map"):
    ops.xattn_map(q, k, acc, 8, 40, 48, 1.0)
  assert (acc == 0).all()
  with pytest.raises(AssertionError):
    ops.xattn_map(q, k[:, :77], acc, 8, 40, 48, 1.0)                     # acc's shape does not match
