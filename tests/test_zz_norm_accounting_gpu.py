"""Every element of the GroupNorm and LayerNorm kernels accounted for with integer inputs whose correct output is known
exactly (tests/norm_probes.py: census, sweep, gates, case matrix): the single-launch GroupNorm in each of its nine
reachable (NT, MAXCH) forms, the two-launch pair, the ten ldm_layernorm instantiations, the GEMM's LayerNorm output and
its LayerNorm fold.  The norm kernels run through the raw C ABI; every fused case asserts its launch form through
ldm_groupnorm_fused_form.

Input and output are channel slices of wider buffers: the foreign input channels and the rows behind the last sample
hold NaN, the foreign output channels a bit pattern that must survive, the output slice is pre-filled with NaN, and two
runs of every launch must give identical bits.  A failure prints the first differing element as (sample, pixel, channel,
group, thread slot).

The module's name puts it behind the older GPU modules in the collection order: it extends the suite's run at its end and
moves no earlier test."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_probes as P  # noqa: E402

NAN = float("nan")
BF, F32, F64 = P.BF, P.F32, P.F64


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


def slices(c, dev, e):
  """(input slice [rows, C], output slice, the wide output buffer, its offset): pitches C + 3 e and C + 5 e, channel
  offsets e and 2 e elements (e = 16 bytes of the dtype, or 8 where the GEMM asks for it)."""
  rows = c.B * c.HW
  wide_in = torch.full((rows + 2, c.C + 3 * e), NAN, dtype=c.dt, device=dev)
  wide_out = torch.full((rows + 2, c.C + 5 * e), P.FOREIGN, dtype=c.dt, device=dev)
  return wide_in[:rows, e:e + c.C], wide_out[:rows, 2 * e:2 * e + c.C], wide_out, 2 * e


def set_census(c, xs, launch, last):
  """Writes the launch's deviants into the device slice (and the base values back where the last launch had its own)."""
  m = P.unit_values(c).reshape(-1)
  for ln, sign in ((last, 0.0), (launch, 1.0)):
    if ln is None:
      continue
    r, ch, delta, unit = P.deviants(c, ln)
    xs[r.to(xs.device), ch.to(xs.device)] = (m[unit] + sign * delta).to(c.dt).to(xs.device)


def take(out_slice, wide_out, off, c):
  """The output slice as a contiguous tensor; everything else in the wide buffer must still hold its pattern."""
  torch.cuda.synchronize()
  got = out_slice.clone(memory_format=torch.contiguous_format)
  w = wide_out.clone()
  w[:c.B * c.HW, off:off + c.C] = P.FOREIGN
  assert bool((w == P.FOREIGN).all()), "the launch wrote outside its output slice"
  out_slice.fill_(NAN)
  return got


def launch_norm(c, xs, os, gd, bd, scratch):
  o = ops()
  lib, code, st = o.lib, o.code(c.dt), o._stream()
  ldx, ldo = xs.stride(0), os.stride(0)
  if c.kind == "fused":
    o.check(lib.ldm_groupnorm_fused(xs.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), os.data_ptr(), ldo, c.B, c.HW, c.C,
                                    c.G, P.EPS, int(c.silu), code, st), "ldm_groupnorm_fused")
  elif c.kind == "pair":
    nch = c.form[0]
    scratch.fill_(NAN)
    o.check(lib.ldm_groupnorm_partial(xs.data_ptr(), ldx, scratch.data_ptr(), c.B, c.HW, c.C, c.G, nch, code, st),
            "ldm_groupnorm_partial")
    o.check(lib.ldm_groupnorm_apply(xs.data_ptr(), ldx, scratch.data_ptr(), gd.data_ptr(), bd.data_ptr(), os.data_ptr(),
                                    ldo, c.B, c.HW, c.C, c.G, nch, P.EPS, int(c.silu), code, st), "ldm_groupnorm_apply")
  else:
    o.check(lib.ldm_layernorm(xs.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), os.data_ptr(), ldo, c.B, c.C, P.EPS, code,
                              st), "ldm_layernorm")


def account(dev, c):
  o = ops()
  e = P.epc(c.dt)
  gamma, beta = P.params(c)
  gd, bd = gamma.to(dev), beta.to(dev)
  xs, os, wide_out, off = slices(c, dev, e)
  xs.copy_(P.base(c).to(c.dt).to(dev))
  scratch = torch.empty(c.B * c.form[0] * c.G * 2, dtype=F32, device=dev) if c.kind == "pair" else None
  if c.kind == "fused":
    f = (C.c_int32 * 4)()
    assert o.lib.ldm_groupnorm_fused_form(c.B, c.HW, c.C, c.G, o.code(c.dt), f) == 0 and tuple(f) == c.form, tuple(f)
  if c.kind == "pair" and not c.nchunks:
    assert o.lib.ldm_groupnorm_nchunks(c.B, c.HW, c.C) == c.form[0]
  failed, worst, last = [], 0.0, None
  for launch in range(P.sweep_launches(c)):
    set_census(c, xs, launch, last)
    last = launch
    launch_norm(c, xs, os, gd, bd, scratch)
    got = take(os, wide_out, off, c)
    launch_norm(c, xs, os, gd, bd, scratch)
    again = take(os, wide_out, off, c)
    same = torch.equal(got.view(torch.int16 if c.dt == BF else torch.int32), again.view(torch.int16 if c.dt == BF else torch.int32))
    ref = P.reference(c, xs.to(F64), gamma, beta)
    msg, w = P.gates(c, got, ref, beta, launch, f"{P.case_id(c)} launch {launch}")
    worst = max(worst, w)
    if not same:
      msg = "two runs differ" + (": " + msg if msg else "")
    if msg:
      print(f"LAUNCH {launch}: {msg}")
      failed.append(f"launch {launch}: {msg}")
  print(f"ACCT {P.case_id(c)} launches {P.sweep_launches(c)} worst deviant {worst:.3f} x gate {'FAILED' if failed else 'ok'}")
  assert not failed, "\n".join(failed[:4])


def _cases(kind):
  return [c for c in P.all_cases() if c.kind == kind]


@pytest.mark.parametrize("c", _cases("fused"), ids=P.case_id)
def test_groupnorm_fused_accounting(dev, c):
  account(dev, c)


@pytest.mark.parametrize("c", _cases("pair"), ids=P.case_id)
def test_groupnorm_two_launch_accounting(dev, c):
  account(dev, c)


@pytest.mark.parametrize("c", _cases("ln"), ids=P.case_id)
def test_layernorm_accounting(dev, c):
  account(dev, c)


@pytest.mark.parametrize("c", _cases("ln_out"), ids=P.case_id)
def test_gemm_layernorm_output_accounting(dev, c):
  """out = A . I through ops.linear(..., ln=...): the product of the census rows is stored exactly, its LayerNorm goes
  to a channel slice (ld_ln is a slice pitch)."""
  o = ops()
  assert o.linear_ln_supported(c.C, c.dt)
  gamma, beta = P.params(c)
  gd, bd = gamma.to(dev), beta.to(dev)
  xs, ls, wide_ln, off = slices(c, dev, 8)
  xs.copy_(P.base(c).to(c.dt).to(dev))
  eye = torch.eye(c.C, dtype=c.dt, device=dev)
  failed, worst, last = [], 0.0, None
  for launch in range(P.sweep_launches(c)):
    set_census(c, xs, launch, last)
    last = launch
    outs = []
    for _ in range(2):
      out = torch.full((c.B, c.C), NAN, dtype=c.dt, device=dev)
      o.linear(xs, eye, out, ln=(gd, bd, ls, P.EPS))
      outs.append((out, take(ls, wide_ln, off, c)))
    assert torch.equal(outs[0][0], xs), "A . I is not A"
    ref = P.reference(c, outs[0][0].to(F64), gamma, beta)
    msg, w = P.gates(c, outs[0][1], ref, beta, launch)
    worst = max(worst, w)
    if not (torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])):
      msg = "two runs differ" + (": " + msg if msg else "")
    if msg:
      print(f"LAUNCH {launch}: {msg}")
      failed.append(f"launch {launch}: {msg}")
  print(f"ACCT {P.case_id(c)} launches {P.sweep_launches(c)} worst deviant {worst:.3f} x gate {'FAILED' if failed else 'ok'}")
  assert not failed, "\n".join(failed[:4])


@pytest.mark.parametrize("c", _cases("ln_fold"), ids=P.case_id)
def test_gemm_layernorm_fold_accounting(dev, c):
  """One-hot weight rows: ln_cs[n] = 1 and out[m][n] = rstd_m (x[m][k(n)] - mean_m) + bias[n]; persistent tiles 13 / 14
  with one workgroup per panel (deal 0) and the default deal (deal 1)."""
  o = ops()
  tile, deal = c.form
  N, sel, bias = P.fold_operands(c)
  w = torch.zeros(N, c.C, dtype=F32)
  w[torch.arange(N), sel] = 1.0
  wd, cs, bd = w.to(BF).to(dev), torch.ones(N, dtype=F32, device=dev), bias.to(dev)
  xs, _, _, _ = slices(c, dev, 8)
  failed, worst = [], 0.0
  for launch in range(P.sweep_launches(c)):
    x = P.census(c, launch)
    xs.copy_(x.to(BF).to(dev))
    outs = []
    for _ in range(2):
      flat = torch.full((c.B + 2, N + 16), NAN, dtype=BF, device=dev)
      o.linear(xs, wd, flat[:c.B, 8:8 + N], bias=bd, ln_fold=(cs, P.EPS), tile=tile, split_k=0 if deal else -1)
      torch.cuda.synchronize()
      outs.append(flat)
    got = outs[0][:c.B, 8:8 + N].clone(memory_format=torch.contiguous_format)
    msg, w_ = P.fold_gates(c, got.cpu(), P.fold_reference(c, x, sel, bias))
    worst = max(worst, w_)
    rest = outs[0].clone()
    rest[:c.B, 8:8 + N] = NAN
    if not bool(torch.isnan(rest).all()):
      msg = "the launch wrote outside its output slice"
    if not torch.equal(got, outs[1][:c.B, 8:8 + N]):
      msg = "two runs differ" + (": " + msg if msg else "")
    if msg:
      print(f"LAUNCH {launch}: {msg}")
      failed.append(f"launch {launch}: {msg}")
  print(f"ACCT {P.case_id(c)} worst element {worst:.3f} bf16 ulp {'FAILED' if failed else 'ok'}")
  assert not failed, "\n".join(failed[:4])
