"""The flags of ldm_gemm_tile_info tell the truth about what ldm_gemm launches.

Every tile of the query x {float32, bf16} x {no activation, GEGLU} x {the family's base form, the phase form, a second A
operand} is forced with tile = t at the smallest shape its family takes:

  ring tiles   plain rows, M = 8, N = bn, K = one K-tile (64 bf16 / 32 float32 elements);
  persistent   plain rows, M = 256, N = bn, K = 64;
  halo-staged  a 3x3 convolution over one 16x16 image, Cin = 64, N = bn;
  phase form   upsample = 2 over one 2x2 image, Cin = one K-tile, N = bn;
  second A     the base form with one more K-tile of columns from a second matrix / image.

The call is accepted exactly where the flags say so -- not a bf16-only tile on float32, GEGLU only with the GEGLU flag
(and never in the phase form, which takes no GEGLU on any tile), the phase form only with the phase flag of the dtype,
a second operand only with the a2 flag -- and returns LDM_ERR_ARG otherwise (ops raises LdmHipError on it).  A rejection
is a host argument check: the NaN-filled output is untouched.  An accepted call must fill that output with exactly the float64 result.  The operands
are small integers, so every sum is exact in either dtype; the GEGLU gates are >= 8, where gelu(g) rounds to g in float32
(1 - erf(8 / sqrt 2) = 1.2e-15) and the product value x gate is again an integer.  A launch case that instantiates
nothing would leave the NaN behind.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
FORMS = ("base", "phase", "a2")


def _table():
  from ldm_tf2_amd import _lib as L
  info, rows = L.TileInfo(), {}
  for t in range(1, L.lib.ldm_gemm_tile_count()):
    assert L.lib.ldm_gemm_tile_info(t, C.byref(info)) == 0
    rows[t] = (info.bm, info.bn, info.flags)
  return rows


def _accepted(L, flags, dtype, geglu, form):
  if flags & L.TILE_BF16_ONLY and dtype == torch.float32:
    return False
  if geglu and (form == "phase" or not flags & L.TILE_GEGLU):
    return False
  if form == "phase":
    return bool(flags & (L.TILE_PHASE_BF16 if dtype == torch.bfloat16 else L.TILE_PHASE_F32))
  return form != "a2" or bool(flags & L.TILE_A2)


def _ints(g, shape, lo, hi):
  return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _weights(g, N, K, geglu):
  """[N, K] integers in -1..1; GEGLU: the gate rows (the upper 32 of every block of 64) in 0..1, their bias 8."""
  w, b = _ints(g, (N, K), -1, 1), _ints(g, (N,), -3, 3)
  if geglu:
    gate = (torch.arange(N) % 64) >= 32
    w[gate] = w[gate].abs()
    b[gate] = 8.0
  return w, b


def _finish(z, geglu):
  if not geglu or z.shape[1] % 64:       # (GEGLU at a width without whole 64-column blocks is rejected: never compared)
    return z
  zb = z.reshape(z.shape[0], -1, 2, 32)
  gate = zb[:, :, 1]
  return (zb[:, :, 0] * 0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))).reshape(z.shape[0], -1)


def _patches(img, taps, oy, ox):
  """[B*H*W, taps*taps*C]: the taps x taps neighbourhood whose first pixel is (y + oy, x + ox), zero outside."""
  B, H, W, Cc = img.shape
  pad = torch.zeros(B, H + 4, W + 4, Cc, dtype=F64)
  pad[:, 2:2 + H, 2:2 + W] = img
  cols = [pad[:, 2 + oy + dy:2 + oy + dy + H, 2 + ox + dx:2 + ox + dx + W]
          for dy in range(taps) for dx in range(taps)]
  return torch.cat(cols, dim=-1).reshape(B * H * W, -1)


def _case(ops, L, dev, t, bm, bn, flags, dtype, geglu, form, g):
  """(params, out, reference, keep-alive) of one launch."""
  bke = 64 if dtype == torch.bfloat16 else 32
  on = lambda v, dt=dtype: v.to(dt).to(dev)
  act = L.ACT_GEGLU if geglu else L.ACT_NONE
  nout = bn // 2 if geglu else bn
  nan = lambda *shape: torch.full(shape, float("nan"), dtype=dtype, device=dev)
  if form == "phase":
    img, (w, b) = _ints(g, (1, 2, 2, bke), 0, 2), _weights(g, 4 * bn, 4 * bke, False)
    w4 = w.reshape(4, bn, 4 * bke)
    out = nan(1, 4, 4, bn)
    ref = torch.empty(1, 4, 4, bn, dtype=F64)
    for a in range(2):
      for c in range(2):
        ref[:, a::2, c::2] = (_patches(img, 2, a - 1, c - 1) @ w4[2 * a + c].T + b[:bn]).reshape(1, 2, 2, bn)
    keep = (on(img), on(w4).contiguous(), on(b[:bn], torch.float32))
    p = ops._up2_params(keep[0], keep[1], out, keep[2], t, 0)
  elif flags & L.TILE_HALO:
    k2 = 64 if form == "a2" else 0
    img, x2, (w, b) = _ints(g, (1, 16, 16, 64), 0, 2), _ints(g, (1, 16, 16, 64), 0, 2), _weights(g, bn, 576 + k2, geglu)
    out = nan(1, 16, 16, bn)
    z = _patches(img, 3, -1, -1) @ w[:, :576].T + b
    if k2:
      z = z + x2.reshape(256, 64) @ w[:, 576:].T
    ref = _finish(z, geglu).reshape(1, 16, 16, -1)
    keep = (on(img), on(w), on(b, torch.float32), on(x2))
    p = ops._conv_params(keep[0], keep[1], out, keep[2], 1, False, None, None, t, 0, False, keep[3] if k2 else None)
  else:
    M, K = (256, 64) if flags & L.TILE_PERSISTENT else (8, bke)
    k2 = bke if form == "a2" else 0
    x, x2, (w, b) = _ints(g, (M, K), 0, 2), _ints(g, (M, bke), 0, 2), _weights(g, bn, K + k2, geglu)
    out = nan(M, nout)
    z = x @ w[:, :K].T + b
    if k2:
      z = z + x2 @ w[:, K:].T
    ref = _finish(z, geglu)
    keep = (on(x), on(w), on(b, torch.float32), on(x2))
    p = ops._row_params(keep[0], keep[1], out, M, bn, K + k2, keep[2], x2=keep[3] if k2 else None, tile=t)
  p.act = act
  return p, out, ref, keep


@pytest.mark.parametrize("t", sorted(_table()))
def test_tile_flags_tell_what_launches(dev, t):
  from ldm_tf2_amd import _lib as L, ops
  bm, bn, flags = _table()[t]
  g = torch.Generator().manual_seed(1000 + t)
  failed = []
  for dtype in (torch.float32, torch.bfloat16):
    for geglu in (False, True):
      for form in FORMS:
        name = f"tile {t} {str(dtype)[6:]} {'geglu' if geglu else 'none'} {form}"
        want = _accepted(L, flags, dtype, geglu, form)
        p, out, ref, keep = _case(ops, L, dev, t, bm, bn, flags, dtype, geglu, form, g)
        ws = ops.workspace(dev)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        st = L.lib.ldm_gemm(C.byref(p), ops._stream())        # (the C entry itself: no plan table, no second try)
        ran, why = st == L.OK, L.last_error()
        assert st in (L.OK, L.ERR_ARG), (name, st, why)
        torch.cuda.synchronize()
        got = out.cpu()
        if ran != want:
          failed.append(f"{name}: the flags say {'accepted' if want else 'rejected'}, ldm_gemm "
                        f"{'ran' if ran else 'said: ' + why}")
        elif not ran:
          if not bool(torch.isnan(got).all()):
            failed.append(f"{name}: rejected ({why}) but the output was written")
        else:
          plan_t, plan_s = C.c_int(), C.c_int()
          assert L.lib.ldm_gemm_plan(C.byref(p), C.byref(plan_t), C.byref(plan_s)) == 0
          if plan_t.value != t:
            failed.append(f"{name}: ran tile {plan_t.value}")
          if not torch.equal(got.to(F64), ref.to(dtype).to(F64)):
            bad = int((got.to(F64) != ref.to(dtype).to(F64)).sum())
            failed.append(f"{name}: {bad} of {ref.numel()} elements differ from the float64 result "
                          f"({int(torch.isnan(got).sum())} still NaN)")
  assert not failed, "\n".join(failed)
