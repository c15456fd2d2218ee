"""Every element of the small sampling-path kernels accounted for (csrc/misc.hip, softmax_rows_kernel): exact probes
gated by torch.equal and float64 comparisons gated by measured figures, on each kernel's own edges
(tests/small_probes.py: the case lists, the expected outputs, the gates and how they were set).

Every operand is a view of a NaN-filled buffer; after a launch the output buffer must still be NaN outside the region
the launch owns.  All calls go through ldm_tf2_amd.ops.  One `ACCT small ...` line per case.

No case repeats a launch: a case that launches more than once gives each launch other data (probe, phase, activation
form, in place).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import small_probes as P  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
NAN = float("nan")


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


def take(view, flat):
  """The values of `view` on the host in its own type; everything else in `flat` must still be NaN."""
  torch.cuda.synchronize()
  got = view.detach().cpu().clone()
  view.fill_(NAN)
  assert bool(torch.isnan(flat).all()), "the launch wrote outside its output region"
  return got


def acct(entry, cid, text):
  print(f"ACCT small {entry} {cid} {text}")


def judge(entry, cid, got, orc, ref, odt, gate, ceiling):
  """Prints the figure of one float64 comparison, then asserts gate and ceiling."""
  kerr, oerr, fig = P.figure(got, orc, ref, odt)
  ceil = P.within(got, ref, *ceiling)
  acct(entry, cid, f"kernel_err {kerr:.3e} oracle_err {oerr:.3e} figure {fig:.3f} gate {gate} ceiling_used {ceil:.3f}")
  assert fig <= gate, f"{entry} {cid}: figure {fig} above the gate {gate}"
  assert ceil <= 1.0, f"{entry} {cid}: {ceil} times the older test's tolerance (rtol, atol) = {ceiling}"


# ---- ldm_conv3x3_small ---------------------------------------------------------------------------------------
def run_conv(dev, c, x, w, bias):
  o = ops()
  npix = c.B * c.H * c.W
  _, xv = P.strided(npix, c.Cin, c.xoff, c.xpad, c.idt, x, dev)
  oflat, ov = P.strided(npix, c.Cout, c.ooff, c.opad, c.odt, None, dev)
  o.conv3x3_small(xv.view(c.B, c.H, c.W, c.Cin), w.to(F32).to(dev).contiguous(),
                  None if bias is None else bias.to(F32).to(dev), ov.view(c.B, c.H, c.W, c.Cout))
  return take(ov, oflat).view(c.B, c.H, c.W, c.Cout)


def test_conv_cases_cover_every_kernel_and_input_type():
  seen = {(c.kernel, c.idt) for c in P.conv_cases()}
  assert seen == {(k, t) for k in ("lds", "in", "out") for t in (F32, BF)}


@pytest.mark.parametrize("c", P.conv_cases(), ids=lambda c: c.id)
def test_conv3x3_small(dev, c):
  assert c.kernel == P.conv_kernel_of(c)
  failed = []
  x, w, bias, exp = P.conv_census(c)
  got = run_conv(dev, c, x, w, bias)
  if not torch.equal(got, exp.to(c.odt)):
    bad = (got.to(F64) != exp) | torch.isnan(got.to(F64))
    failed.append(f"census: {int(bad.sum())} differ, first (b, y, x, co) = {bad.nonzero()[0].tolist()}")
  for ph in c.phases:
    x, w, _, exp = P.conv_selection(c, ph)
    got = run_conv(dev, c, x, w, None)
    if not torch.equal(got, exp.to(c.odt)):
      bad = (got.to(F64) != exp) | torch.isnan(got.to(F64))
      i = bad.nonzero()[0].tolist()
      failed.append(f"selection {ph}: {int(bad.sum())} differ, first (b, y, x, co) = {i}: got {float(got[tuple(i)])}, "
                    f"want {float(exp[tuple(i)])}")
  npass, grid = P.passes(*P.conv_items(c))
  acct("conv3x3_small", c.id, f"kernel {c.kernel} items {P.conv_items(c)[0]} workgroups {grid} passes {npass} "
       f"{'FAILED' if failed else 'exact'}")
  assert not failed, "\n".join(failed)
  if c.rand:
    x, w, bias = P.conv_random(c)
    ref = P.conv_ref64(x, w, bias)
    orc = O.conv2d(x.to(F32), w.to(F32), None if bias is None else bias.to(F32)).to(c.odt).to(F64)
    got = run_conv(dev, c, x, w, bias).to(F64)
    judge("conv3x3_small", c.id, got, orc, ref, c.odt, P.gate("conv_" + c.kernel, c.idt, c.odt), P.conv_ceiling(c))


# ---- ldm_gemv ----------------------------------------------------------------------------------------------------
def run_gemv(dev, c, x, w, b, act_in, act_out):
  o = ops()
  _, xv = P.strided(c.rows, c.K, 0, c.xpad, F32, x, dev)
  yflat, yv = P.strided(c.rows, c.N, 0, c.ypad, F32, None, dev)
  o.gemv(xv, w.to(c.wdt).to(dev).contiguous(), b.to(F32).to(dev), yv, act_in=act_in, act_out=act_out)
  return take(yv, yflat).to(F64)


@pytest.mark.parametrize("c", P.gemv_cases(), ids=lambda c: c.id)
def test_gemv(dev, c):
  o = ops()
  x, w, b = P.gemv_exact(c)
  got = run_gemv(dev, c, x, w, b, o.ACT_NONE, o.ACT_NONE)
  exact = torch.equal(got, x @ w.t() + b)
  acct("gemv", c.id, "exact" if exact else "FAILED")
  assert exact, (got - (x @ w.t() + b)).abs().max()
  x, w, b = P.gemv_random(c)
  for name, (ai, ao) in P.GEMV_ACTS.items():
    got = run_gemv(dev, c, x, w, b, o.ACT_SILU if ai else o.ACT_NONE, o.ACT_SILU if ao else o.ACT_NONE)
    judge("gemv", f"{c.id}-{name}", got, P.gemv_oracle(x, w, b, ai, ao, O), P.gemv_ref64(x, w, b, ai, ao), F32,
          P.gate("gemv", c.wdt), (2e-4, 2e-4))


# ---- ldm_vq_nearest --------------------------------------------------------------------------------------------
def run_vq(dev, z, cb, with_indices):
  o = ops()
  rows, Cc = z.shape
  oflat, ov = P.strided(rows, Cc, 0, 0, F32, None, dev)
  ind = torch.full((rows + 8,), -7, dtype=torch.int64, device=dev) if with_indices else None
  o.vq_nearest(z.to(F32).to(dev), cb.to(F32).to(dev), ov, None if ind is None else ind[:rows])
  out = take(ov, oflat)
  if ind is not None:
    assert bool((ind[rows:] == -7).all())
    return out, ind[:rows].cpu()
  return out, None


@pytest.mark.parametrize("c", P.vq_cases(), ids=lambda c: c.id)
def test_vq_nearest(dev, c):
  z, cb, idx, q = P.vq_data(c)
  out, ind = run_vq(dev, z, cb, True)
  out2, _ = run_vq(dev, z, cb, False)
  ok = torch.equal(ind, idx) and torch.equal(out.to(F64), q) and torch.equal(out2.to(F64), q)
  acct("vq_nearest", c.id, f"plants {P.vq_plants(c.V, c.C)} {'exact' if ok else 'FAILED'}")
  assert torch.equal(ind, idx), (ind != idx).nonzero().flatten().tolist()[:8]
  assert torch.equal(out.to(F64), q) and torch.equal(out2.to(F64), q)


def test_vq_nearest_all_distances_infinite(dev):
  """Finite z whose squared norm overflows float32: every distance is +inf; the answer is the oracle's (argmin: row 0)."""
  z, cb = P.vq_overflow_data()
  qr, ir = O.vq_nearest(z, cb)
  assert int(ir[1]) == 0 and bool(torch.isfinite(z).all()) and bool(torch.isinf((z * z).sum(1))[[1, 4, 9]].all())
  out, ind = run_vq(dev, z, cb, True)
  acct("vq_nearest", "overflow", f"indices {ind.tolist()}")
  assert torch.equal(ind, ir)
  assert torch.equal(out, qr)


# ---- ldm_minmax_u8 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.minmax_cases(), ids=lambda c: c.id)
def test_minmax_u8(dev, c):
  o = ops()
  x = P.minmax_data(c)
  xd = x.to(c.dt).to(dev)
  out = torch.full((c.B * c.n + 64,), 77, dtype=torch.uint8, device=dev)
  o.minmax_u8(xd, out[:c.B * c.n].view(c.B, c.n))
  torch.cuda.synchronize()
  got = out[:c.B * c.n].view(c.B, c.n).cpu()
  ok = torch.equal(got.to(torch.int64), x)
  acct("minmax_u8", c.id, "exact" if ok else "FAILED")
  assert bool((out[c.B * c.n:] == 77).all())
  assert ok, (got.to(torch.int64) != x).nonzero()[:4].tolist()
  assert np.array_equal(got.numpy(), O.tensor_to_image(x.to(c.dt).float().numpy()))


@pytest.mark.parametrize("dt", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 37, 41, 3), (2, 1, 1, 2), (1, 250, 250, 3)], ids=str)
def test_minmax_u8_random_images(dev, dt, shape):
  """The bit-exact comparison with the oracle's tensor_to_image, at sizes that are not multiples of 256."""
  o = ops()
  img = (P.rnd(shape, 800 + shape[1], 3.0)).to(dt)
  u8 = torch.empty(shape, dtype=torch.uint8, device=dev)
  o.minmax_u8(img.to(dev), u8)
  assert np.array_equal(u8.cpu().numpy(), O.tensor_to_image(img.float().numpy()))


# ---- ldm_cast ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.cast_cases(), ids=lambda c: c.id)
def test_cast(dev, c):
  o = ops()
  x = P.cast_data(c)
  xflat, xv = P.strided(c.rows, c.cols, c.xoff, c.xpad, c.idt, None, dev)
  xv.copy_(x.to(dev))                                             # (a device copy keeps every bit pattern)
  assert P.same_bits(xv.cpu(), x)
  oflat, ov = P.strided(c.rows, c.cols, c.ooff, c.opad, c.odt, None, dev)
  o.cast(xv, ov)
  got = take(ov, oflat)
  ok = P.same_bits(got, x.to(c.odt))
  acct("cast", c.id, "bit-exact" if ok else "FAILED")
  if not ok:
    want = x.to(c.odt)
    bad = (P.bits_of(got) != P.bits_of(want)) & ~(torch.isnan(want) & torch.isnan(got))
    i = tuple(bad.nonzero()[0].tolist())
    pytest.fail(f"{int(bad.sum())} differ; first at {i}: in {int(P.bits_of(x)[i]):#x} got {int(P.bits_of(got)[i]):#x} "
                f"want {int(P.bits_of(want)[i]):#x}")


# ---- ldm_embedding -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.embedding_cases(), ids=lambda c: c.id)
def test_embedding(dev, c):
  o = ops()
  ids, tok, pos = P.embedding_data(c)
  oflat, ov = P.strided(c.rows * c.T, c.D, 0, 0, c.odt, None, dev)
  o.embedding(ids.to(dev), tok.to(dev), pos.to(dev), ov.view(c.rows, c.T, c.D))
  got = take(ov, oflat).view(c.rows, c.T, c.D)
  want = (tok[ids.clamp(0, c.vocab - 1)] + pos[None]).to(c.odt)
  ok = torch.equal(got, want)
  acct("embedding", c.id, "exact" if ok else "FAILED")
  assert ok, (got != want).nonzero()[:4].tolist()


# ---- ldm_post_quant, ldm_gaussian_sample ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.post_quant_cases(), ids=lambda c: c.id)
def test_post_quant(dev, c):
  o = ops()
  z, k, b = P.post_quant_data(c)
  npix = z.numel() // c.C
  oflat, ov = P.strided(npix, c.C, 0, 0, c.odt, None, dev)
  o.post_quant(z.to(dev), c.sf, k.to(dev), None if b is None else b.to(dev), ov.view(z.shape))
  got = take(ov, oflat).view(z.shape).to(F64)
  orc = O.dense(z / c.sf, k, b).to(c.odt).to(F64)
  judge("post_quant", c.id, got, orc, P.post_quant_ref64(c, z, k, b), c.odt, P.gate("post_quant", c.odt),
        P.post_quant_ceiling(c))


@pytest.mark.parametrize("c", P.gaussian_cases(), ids=lambda c: c.id)
def test_gaussian_sample(dev, c):
  o = ops()
  mom, noise = P.gaussian_data(c)
  npix = mom.numel() // (2 * c.C)
  oflat, ov = P.strided(npix, c.C, 0, 0, F32, None, dev)
  o.gaussian_sample(mom.to(dev), ov.view(c.shape + (c.C,)), noise=None if noise is None else noise.to(dev), out_scale=c.scale)
  got = take(ov, oflat).view(c.shape + (c.C,)).to(F64)
  _, _, sample = O.diagonal_gaussian(mom, noise)
  orc = (sample * c.scale).to(F64)
  judge("gaussian_sample", c.id, got, orc, P.gaussian_ref64(c, mom, noise), F32, P.gate("gaussian_sample", F32),
        P.GAUSSIAN_CEILING)


# ---- ldm_softmax_rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.softmax_cases(), ids=lambda c: c.id)
def test_softmax_rows(dev, c):
  o = ops()
  x = P.softmax_data(c)
  ref = P.softmax_ref64(c, x)
  orc = torch.softmax(x.to(F32) * c.scale, dim=-1).to(c.odt).to(F64)
  xflat, xv = P.strided(c.rows, c.cols, 0, c.xpad, c.idt, x, dev)         # logits[:, :n] of a wider buffer
  outs = []
  oflat, ov = P.strided(c.rows, c.cols, 0, c.opad, c.odt, None, dev)
  o.softmax_rows(xv, ov, c.scale)
  outs.append(("", take(ov, oflat).to(F64)))
  if c.idt == c.odt:
    o.softmax_rows(xv, xv, c.scale)                                      # in place
    outs.append(("-inplace", take(xv, xflat).to(F64)))
  for tag, got in outs:
    if c.odt == F32:
      dev_sum = float((got.sum(1) - 1.0).abs().max())
      acct("softmax_rows", c.id + tag, f"row_sum_error {dev_sum:.3e} bound {P.ROW_SUM_BOUND:.3e}")
      assert dev_sum <= P.ROW_SUM_BOUND
    judge("softmax_rows", c.id + tag, got, orc, ref, c.odt, P.gate("softmax_rows", c.idt, c.odt), P.softmax_ceiling(c))


# ---- ldm_time_embedding ----------------------------------------------------------------------------------------------
def run_time(dev, rows, channels, **kw):
  o = ops()
  oflat, ov = P.strided(rows, channels, 0, 0, F32, None, dev)
  o.time_embedding(ov, channels, **{k: v.to(dev) for k, v in kw.items()})
  return take(ov, oflat)


@pytest.mark.parametrize("channels", P.TIME_CHANNELS)
def test_time_embedding_every_t(dev, channels):
  t = torch.arange(1000, dtype=torch.int32)
  got = run_time(dev, 1000, channels, t_rows=t)
  if channels % 2:
    assert bool((got[:, -1] == 0).all())
  judge("time_embedding", f"c{channels}-t0..999", got.to(F64), O.get_time_embedding(t.numpy(), channels).to(F64),
        P.time_ref64(t, channels), F32, P.gate("time_embedding", F32), P.TIME_CEILING)


@pytest.mark.parametrize("i", range(len(P.step_table())))
def test_time_embedding_every_index_of_a_step_table(dev, i):
  steps = P.step_table()
  got = run_time(dev, 3, 320, steps=steps, index=torch.tensor([i], dtype=torch.int32))
  assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
  ref = P.time_ref64(steps[i:i + 1], 320).expand(3, -1)
  orc = O.get_time_embedding(steps[i:i + 1].numpy(), 320).to(F64).expand(3, -1)
  judge("time_embedding", f"steps-index{i}-t{int(steps[i])}", got.to(F64), orc, ref, F32, P.gate("time_embedding", F32),
        P.TIME_CEILING)


@pytest.mark.parametrize("channels", (320, 321, 1280))
def test_time_embedding_frequencies(dev, channels):
  got = run_time(dev, 2, channels, t_rows=torch.tensor([1, 1], dtype=torch.int32))
  f, k = P.freqs_from_sines(got[1], channels)
  want = P.freqs64(channels)[k]
  rel = float(((f - want).abs() / want).max())
  fo, _ = P.freqs_from_sines(O.get_time_embedding(np.array([1]), channels)[0], channels)
  relo = float(((fo - want).abs() / want).max())
  acct("time_embedding", f"c{channels}-frequencies", f"rel_err {rel:.3e} oracle_rel_err {relo:.3e} bound {P.FREQ_BOUND}")
  assert rel <= P.FREQ_BOUND
