"""Every element of the sampler kernels accounted for (csrc/sampler.hip): the exact probes of tests/sampler_probes.py
through ldm_tf2_amd.ops, gated by equality with no tolerance; a table of calls every wide entry must reject with its own
message and without touching an output; and in-place calls that must give the bits of the out-of-place ones.

Every operand is a view into a NaN-filled buffer (a read outside it poisons the result), every output has NaN canaries
before and after it, and what the header says is not read holds NaN (sampler_probes.build).  Drawn noise is compared,
bit for bit, with what ldm_normal_fill gives for the same stream; ldm_normal_fill is tied to the words of
ldm_philox_u32, and those, exactly, to tests/philox_ref.py.  One `ACCT sampler ...` line per case.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import philox_ref as R  # noqa: E402
import sampler_probes as P  # noqa: E402

F32, BF, F64, I32 = torch.float32, torch.bfloat16, torch.float64, torch.int32
NAN = float("nan")
PAD = 64                                       # elements of NaN before and after every array (a multiple of 16 bytes)
UPD, FILL = P.update_cases(), P.fill_cases()


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


def guard(data, dev, dtype=F32):
  """(flat, view): `data` (1-D, on the CPU) in `dtype` between two runs of PAD NaNs, on the device."""
  n = data.numel()
  flat = torch.full((n + 2 * PAD,), NAN, dtype=dtype)
  flat[PAD:PAD + n] = data.to(dtype)
  flat = flat.to(dev)
  return flat, flat[PAD:PAD + n]


def blank(n, dev, dtype=F32):
  return guard(torch.full((n,), NAN, dtype=F64), dev, dtype)


def pads_intact(flat):
  return bool(torch.isnan(flat[:PAD]).all()) and bool(torch.isnan(flat[-PAD:]).all())


def rng_state(dev):
  w = np.array([P.SEED & 0xffffffff, P.SEED >> 32, P.FIRST, 0], dtype=np.uint32)
  return torch.from_numpy(w.view(np.int32).copy()).to(dev)


def device_draws(dev, c):
  """stream -> float64 [B n]: what ldm_normal_fill gives for the stream at the case's shape."""
  def f(stream):
    flat, out = blank(c.B * c.n, dev)
    ops().normal_fill(out.view(c.B, c.n), rng_state(dev), stream)
    torch.cuda.synchronize()
    assert pads_intact(flat)
    return out.cpu().to(F64)
  return f


def acct(c, text):
  print(f"ACCT sampler {c.entry} {c.id} {text}")


# ---- the operands of an update launch on the device ------------------------------------------------------------------
def make(dev, c, p):
  """Device tensors of one update launch: A.<name> the tensor the wrapper takes, A.flat[<name>] its guarded buffer."""
  total, npix = c.B * c.n, c.n // c.ch
  s3 = (c.B, npix, c.ch)
  A = P.NS(flat={})

  def put(name, data, shape=None, dtype=F32):
    if data is None:
      setattr(A, name, None)
      return
    A.flat[name], v = guard(data, dev, dtype)
    setattr(A, name, v if shape is None else v.view(shape))

  put("eps", p.eps, (2 * c.B, npix, c.ch))
  put("xt", p.xt, s3)
  if c.alias:
    A.xt_out = A.xt
  else:
    put("xt_out", torch.full((total,), NAN, dtype=F64), s3)
  put("pred", torch.full((total,), NAN, dtype=F64) if c.pred else None, s3)
  put("xu", torch.full((2 * total,), NAN, dtype=F64) if c.xd is not None else None, (2 * c.B, npix, c.ch), c.xd or F32)
  put("coef", p.coef, (P.N_ROWS, 4))
  put("gtab", p.gtab)
  put("ring", p.ring, (4,) + s3)
  put("weights", p.weights)
  if A.weights is not None:
    A.weights = torch.as_strided(A.weights, (P.N_ROWS, 4, 4), (c.pitch, 4, 1))
  put("noise", p.noise)
  put("z0", p.z0, s3)
  put("mask", p.mask, (c.B, npix))
  put("q", p.q)
  put("qcoef", p.qcoef, (P.N_ROWS, 2))
  A.index = torch.tensor([p.idx], dtype=I32, device=dev)
  A.start = torch.tensor([p.start], dtype=I32, device=dev)
  A.rng = rng_state(dev)
  return A


def launch(c, A):
  o = ops()
  common = dict(x_unet_out=A.xu, dec_index=c.dec, pred_x0_out=A.pred)
  blend = dict(z0=A.z0, mask=A.mask, q_coef=A.qcoef)
  table = dict(q_noise=A.q, q_index_stride=c.q_stride)
  gs = float(c.gs)
  e = c.entry
  if e == "ddim":
    o.cfg_ddim_update(A.eps, A.xt, A.xt_out, A.coef, A.index, gs, noise=A.noise, clip_denoised=c.clip,
                      noise_index_stride=c.noise_stride, **common)
  elif e == "ddim_masked":
    o.cfg_ddim_update_masked(A.eps, A.xt, A.xt_out, A.coef, A.index, gs, A.z0, A.mask, A.q, A.qcoef, noise=A.noise,
                             clip_denoised=c.clip, noise_index_stride=c.noise_stride, q_index_stride=c.q_stride, **common)
  elif e == "ddim_rng":
    o.cfg_ddim_update_rng(A.eps, A.xt, A.xt_out, A.coef, A.index, A.rng, gs, clip_denoised=c.clip, **common, **blend)
  elif e == "plms":
    o.cfg_plms_update(A.eps, A.xt, A.xt_out, A.ring, A.coef, A.index, A.start, gs, **common, **blend, **table)
  elif e == "plms_rng":
    o.cfg_plms_update_rng(A.eps, A.xt, A.xt_out, A.ring, A.coef, A.index, A.start, A.rng, gs, **common, **blend)
  elif e == "ms":
    o.cfg_ms_update(A.eps, A.xt, A.xt_out, A.ring, A.coef, A.index, A.start, A.weights, gs, **common, **blend, **table)
  elif e == "ms_rng":
    o.cfg_ms_update_rng(A.eps, A.xt, A.xt_out, A.ring, A.coef, A.index, A.start, A.weights, A.rng, gs, **common, **blend)
  elif e == "sched":
    o.cfg_sched_update(A.eps, A.xt, A.xt_out, A.coef, A.gtab, A.index, c.guided, ring=A.ring, start=A.start,
                       weights=A.weights, rng=A.rng if c.rng else None, **common, **blend, **table)
  else:
    o.cfg_ddim_invert_update(A.eps, A.xt, A.xt_out, A.coef, A.index, c.guided, guidance_scale=gs, **common)


def collect(c, A):
  """The outputs on the host (float64), after checking every canary and every input the launch must not write."""
  torch.cuda.synchronize()
  for name, flat in A.flat.items():
    assert pads_intact(flat), f"{name}: a canary was overwritten"
  out = P.NS(xt_out=A.xt_out.reshape(-1).cpu().to(F64), index=int(A.index.item()))
  out.pred_x0 = None if A.pred is None else A.pred.reshape(-1).cpu().to(F64)
  out.ring = None if A.ring is None else A.ring.reshape(-1).cpu().to(F64)
  out.x_unet = None if A.xu is None else A.xu.reshape(-1).cpu().to(F64)
  return out


def bits(t):
  return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16).cpu()


def run_update(dev, c, p):
  A = make(dev, c, p)
  before = {k: bits(A.flat[k]) for k in A.flat if k not in ("xt_out", "pred", "xu") and not (k == "xt" and c.alias)}
  launch(c, A)
  out = collect(c, A)
  total = c.B * c.n
  for k, b in before.items():
    now = bits(A.flat[k])
    if k == "ring" and P.has_hist(c):                       # the slot written is compared with the reference; the
      s = PAD + (c.idx & 3) * total                         # other three keep their bits
      now, b = torch.cat([now[:s], now[s + total:]]), torch.cat([b[:s], b[s + total:]])
    assert torch.equal(now, b), f"{k} was written"
  return out


# ---- 1. the probe matrix -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", UPD, ids=lambda c: c.id)
def test_update_probe(dev, c):
  p = P.build(c, device_draws(dev, c))
  want = P.reference(c, p)
  got = run_update(dev, c, p)
  bad = P.differing(got, want)
  if bad:
    k = bad[0]
    g, w = getattr(got, k), getattr(want, k)
    where = ((g != w) & ~(torch.isnan(g) & torch.isnan(w))).nonzero()[:4].flatten().tolist() if torch.is_tensor(g) else [g, w]
    acct(c, f"NOT EQUAL in {bad}: {k} first at {where}")
  else:
    acct(c, "equal")
  assert bad == []


def _words(dev, c):
  flat = torch.full((c.B * c.n + 2 * PAD,), -7777, dtype=I32, device=dev)
  out = flat[PAD:PAD + c.B * c.n]
  ops().philox_u32(out.view(c.B, c.n), rng_state(dev), c.stream)
  torch.cuda.synchronize()
  assert bool((flat[:PAD] == -7777).all()) and bool((flat[-PAD:] == -7777).all())
  return out.cpu().numpy().view(np.uint32).reshape(c.B, c.n)


@pytest.mark.parametrize("c", FILL, ids=lambda c: c.id)
def test_fill_probe(dev, c):
  o = ops()
  total = c.B * c.n
  if c.entry == "philox_u32":
    equal = np.array_equal(_words(dev, c), R.words(P.SEED, P.FIRST, c.stream, c.B, c.n))
    acct(c, "equal" if equal else "NOT EQUAL")
    assert equal
    return
  xf, xt_out = blank(total, dev)
  uf, xu = blank(2 * total, dev, c.xd) if c.xd is not None else (None, None)
  xu2 = None if xu is None else xu.view(2 * c.B, c.n)
  if c.entry == "normal_fill":
    # tied to the words of ldm_philox_u32 by the bound of test_device_noise_gpu.py: 4 x the error of the float32
    # restatement against the float64 one (an element of another counter is off by the order of 1)
    o.normal_fill(xt_out.view(c.B, c.n), rng_state(dev), c.stream, x_unet_out=xu2)
    torch.cuda.synchronize()
    w = _words(dev, c)
    z64, z32 = R.normals_from_words(w, np.float64), R.normals_from_words(w, np.float32)
    base = float(np.abs(z32.astype(np.float64) - z64).max())
    got = xt_out.cpu()
    err = float(np.abs(got.numpy().astype(np.float64).reshape(c.B, c.n) - z64).max())
    acct(c, f"max |normal - float64 Box-Muller of the device's words| {err:.3e}, bound {4 * base:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= 4 * base
    want = P.NS(xt_out=got.to(F64), x_unet=None if xu is None else torch.cat([got, got]).to(c.xd).to(F64))
  else:
    p = P.build(c, device_draws(dev, c))
    want = P.reference(c, p)
    _, x0 = guard(p.x0, dev)
    t = p.t.to(I32).to(dev)
    _, sac = guard(p.sac, dev)
    _, s1m = guard(p.s1m, dev)
    if c.entry == "q_sample":
      _, noise = guard(p.noise, dev)
      index = torch.tensor([p.idx], dtype=I32, device=dev) if c.use_index else None
      o.q_sample(x0.view(c.B, c.n), noise, t, sac, s1m, xt_out.view(c.B, c.n), x_unet_out=xu2, index=index,
                 noise_index_stride=c.noise_stride if c.use_index else 0)
      torch.cuda.synchronize()
      assert index is None or int(index.item()) == p.idx
    else:
      o.q_sample_rng(x0.view(c.B, c.n), rng_state(dev), c.stream, t, sac, s1m, xt_out.view(c.B, c.n), x_unet_out=xu2)
  torch.cuda.synchronize()
  assert pads_intact(xf) and (uf is None or pads_intact(uf))
  ok = P.same(xt_out.cpu().to(F64), want.xt_out) and (xu is None or P.same(xu.cpu().to(F64), want.x_unet))
  acct(c, "equal" if ok else "NOT EQUAL")
  assert ok


# ---- 2. in place ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", P.UPDATE_ENTRIES)
def test_in_place_gives_the_bits_of_out_of_place(dev, entry):
  small = [c for c in UPD if c.entry == entry and c.probe == "census" and not c.alias and c.B * c.n < 100000]
  c = next((c for c in small if P.blend_on(c)), small[0])
  p = P.build(c, device_draws(dev, c))
  a = run_update(dev, c, p)
  b = run_update(dev, P.NS(**{**vars(c), "alias": True}), p)
  assert P.differing(a, b) == [] and P.differing(a, P.reference(c, p)) == []


# ---- 3. what every wide entry must reject ----------------------------------------------------------------------------
ALIGNED = "arrays must be 16-byte aligned"
MULT4 = r"bad args \(n_per_sample=6 must be a positive multiple of 4\)"
CNAME = {"ddim_masked": "ldm_cfg_ddim_update_masked", "plms": "ldm_cfg_plms_update", "ddim_rng": "ldm_cfg_ddim_update_rng",
         "plms_rng": "ldm_cfg_plms_update_rng", "ms": "ldm_cfg_ms_update", "ms_rng": "ldm_cfg_ms_update_rng",
         "sched": "ldm_cfg_sched_update", "invert": "ldm_cfg_ddim_invert_update"}
WIDE_UPDATES = ("plms", "ddim_rng", "plms_rng", "ms", "ms_rng", "sched", "invert")
TABLE_Q = ("plms", "ms", "sched")
RING = ("plms", "plms_rng", "ms", "ms_rng", "sched")
WEIGHTS = ("ms", "ms_rng", "sched")
BLENDS = ("plms", "ddim_rng", "plms_rng", "ms", "ms_rng", "sched")


def _rejections():
  rows = []
  for e in WIDE_UPDATES:
    for arg in ("eps", "xt", "xt_out", "pred", "xu_f32", "xu_bf16"):
      rows.append((e, "shift:" + arg, ALIGNED))
    rows += [(e, "n=6", MULT4), (e, "null:eps", "null pointer"), (e, "null:xt_out", "null pointer")]
  rows += [(e, "shift:ring", ALIGNED) for e in RING] + [(e, "null:ring", "null pointer") for e in RING if e != "sched"]
  rows += [(e, "shift:z0", ALIGNED) for e in BLENDS] + [(e, "null:mask", "z0 without mask") for e in BLENDS]
  rows += [(e, "channels=5", r"bad args \(n_per_sample=12, channels=5\)") for e in BLENDS + ("ddim_masked",)]
  rows += [(e, "shift:q", ALIGNED) for e in TABLE_Q] + [(e, "q_stride=38", ALIGNED) for e in TABLE_Q]
  rows += [(e, "pitch=12", "weights_pitch=12") for e in WEIGHTS]
  rows += [(e, "null:weights", "null pointer") for e in ("ms", "ms_rng")]
  rows += [(e, "null:rng", "null pointer") for e in ("ddim_rng", "plms_rng", "ms_rng")]
  rows += [("sched", "null:gtab", "null pointer"), ("sched", "null:ring", "weights without ring")]
  return rows


def _raw_call(c, A, ch):
  """The C entry of case `c` called directly (the wrappers assert some of these away before the library sees them):
  `ch` maps an argument's name to its value."""
  from ldm_tf2_amd import _lib
  ptr = lambda t: None if t is None else t.data_ptr()
  v = dict(eps=ptr(A.eps), xt=ptr(A.xt), xt_out=ptr(A.xt_out), pred=ptr(A.pred), xu=ptr(A.xu), coef=ptr(A.coef),
           index=ptr(A.index), start=ptr(A.start), ring=ptr(A.ring), weights=ptr(A.weights), gtab=ptr(A.gtab), rng=ptr(A.rng),
           z0=ptr(A.z0), mask=ptr(A.mask), q=ptr(A.q), qcoef=ptr(A.qcoef), noise=ptr(A.noise), n=c.n, channels=c.ch,
           q_stride=c.q_stride, pitch=c.pitch, xd=ops().code(c.xd))
  v.update(ch)
  stream = torch.cuda.current_stream().cuda_stream
  head = [v["eps"], v["xt"]]
  mid = [v["xt_out"], v["pred"], v["xu"], v["xd"], v["coef"]]
  tail_q = [v["z0"], v["mask"], v["q"], v["q_stride"], v["qcoef"], v["channels"], stream]
  tail_r = [v["z0"], v["mask"], v["qcoef"], v["channels"], stream]
  gs, e, L = float(c.gs), c.entry, _lib.lib
  if e == "ddim_masked":
    st = L.ldm_cfg_ddim_update_masked(*head, v["noise"], c.noise_stride, *mid, v["index"], 1, gs, 0, c.B, v["n"], *tail_q)
  elif e == "plms":
    st = L.ldm_cfg_plms_update(*head, v["ring"], *mid, v["index"], v["start"], 1, gs, c.B, v["n"], *tail_q)
  elif e == "ddim_rng":
    st = L.ldm_cfg_ddim_update_rng(*head, v["rng"], *mid, v["index"], 1, gs, 0, c.B, v["n"], *tail_r)
  elif e == "plms_rng":
    st = L.ldm_cfg_plms_update_rng(*head, v["ring"], *mid, v["index"], v["start"], v["rng"], 1, gs, c.B, v["n"], *tail_r)
  elif e == "ms":
    st = L.ldm_cfg_ms_update(*head, v["ring"], *mid, v["index"], v["start"], v["weights"], v["pitch"], 1, gs, c.B, v["n"], *tail_q)
  elif e == "ms_rng":
    st = L.ldm_cfg_ms_update_rng(*head, v["ring"], *mid, v["index"], v["start"], v["weights"], v["pitch"], v["rng"], 1, gs,
                                 c.B, v["n"], *tail_r)
  elif e == "sched":
    st = L.ldm_cfg_sched_update(*head, v["ring"], *mid, v["gtab"], v["index"], v["start"], v["weights"], v["pitch"], None, 1, 1,
                                c.B, v["n"], *tail_q)
  else:
    st = L.ldm_cfg_ddim_invert_update(*head, *mid, v["index"], 1, 1, gs, c.B, v["n"], stream)
  _lib.check(st, "raw")


@pytest.mark.parametrize("entry, what, message", _rejections(), ids=lambda v: str(v).replace(" ", "_")[:40])
def test_rejected_calls_raise_and_write_nothing(dev, entry, what, message):
  from ldm_tf2_amd._lib import LdmHipError
  kind, _, arg = what.partition(":")
  xd = BF if arg == "xu_bf16" else F32
  c = P._u(entry, "census", n=12, ch=4, idx=1, xd=xd, blend=entry in BLENDS + ("ddim_masked",), qc=(2, 0), gs=3, d=2,
           guided=1, rng=0, weights=1)
  p = P.build(c)
  A = make(dev, c, p)
  name = "xu" if arg.startswith("xu") else arg
  if kind == "shift":                                       # 4 bytes off; every buffer has PAD elements of slack
    change = {name: getattr(A, name).data_ptr() + 4}
  elif kind == "null":
    change = {name: None}
  elif what == "n=6":
    change = {"n": 6}
  elif what == "channels=5":
    change = {"channels": 5}
  elif what == "q_stride=38":
    change = {"q_stride": 38}
  else:
    assert what == "pitch=12"
    change = {"pitch": 12}
  before = {k: bits(f) for k, f in A.flat.items()}
  with pytest.raises(LdmHipError, match=f"{CNAME[entry]}: {message}"):
    _raw_call(c, A, change)
  torch.cuda.synchronize()
  for k, b in before.items():
    assert torch.equal(bits(A.flat[k]), b), f"{k} was written by a rejected call"
  assert int(A.index.item()) == c.idx


def test_sched_without_weights_touches_neither_ring_nor_start(dev):
  """weights == NULL: `ring and start may be NULL and are not touched` (the wrapper passes NULL for both, so this is a
  direct call): a NaN ring keeps its bits and poisons nothing, whatever *start holds."""
  c = P._u("sched", "census", n=12, idx=1, gs=3, a_prev=0, guided=1, rng=0, weights=0, blend=1, mask="mix", qc=(2, 1))
  p = P.build(c)
  A = make(dev, c, p)
  rf, ring = blank(4 * c.B * c.n, dev)
  A.start.fill_(c.idx + 2)
  _raw_call(c, A, {"ring": ring.data_ptr()})
  assert P.differing(collect(c, A), P.reference(c, p)) == []
  assert bool(torch.isnan(rf).all()) and int(A.start.item()) == c.idx + 2


FILL_REJECTIONS = [(e, w) for e in ("q_sample_rng", "normal_fill", "philox_u32")
                   for w in ("shift:out", "shift:xu_f32", "shift:xu_bf16", "shift:x0", "n=6", "null:out", "null:rng")
                   if not (e == "philox_u32" and "xu" in w) and not (e != "q_sample_rng" and w == "shift:x0")]


@pytest.mark.parametrize("entry, what", FILL_REJECTIONS, ids=lambda v: str(v))
def test_rejected_fill_calls_raise_and_write_nothing(dev, entry, what):
  from ldm_tf2_amd import _lib
  B, n = 3, 12
  kind, _, arg = what.partition(":")
  xd = BF if arg == "xu_bf16" else F32
  of, out = blank(B * n, dev)
  uf, xu = blank(2 * B * n, dev, xd)
  _, x0 = guard(torch.arange(B * n, dtype=F64), dev)
  _, tab = guard(torch.ones(P.Q_STEPS, dtype=F64), dev)
  t = torch.zeros(B, dtype=I32, device=dev)
  v = dict(out=out.data_ptr(), xu=xu.data_ptr() if entry != "philox_u32" else None, x0=x0.data_ptr(),
           rng=rng_state(dev).data_ptr(), n=n)
  name = "xu" if arg.startswith("xu") else arg
  if kind == "shift":
    v[name] += 4
  elif kind == "null":
    v[name] = None
  else:
    v["n"] = 6
  stream = torch.cuda.current_stream().cuda_stream
  message = "null pointer" if kind == "null" else f"n_per_sample={v['n']} must be a positive multiple of 4, .*16-byte aligned"
  with pytest.raises(_lib.LdmHipError, match=f"ldm_{entry}: {message}"):
    if entry == "philox_u32":
      _lib.check(_lib.lib.ldm_philox_u32(v["out"], v["rng"], 7, B, v["n"], stream), entry)
    elif entry == "normal_fill":
      _lib.check(_lib.lib.ldm_normal_fill(v["out"], v["rng"], 7, B, v["n"], v["xu"], ops().code(xd), stream), entry)
    else:
      _lib.check(_lib.lib.ldm_q_sample_rng(v["x0"], v["rng"], 7, t.data_ptr(), tab.data_ptr(), tab.data_ptr(), P.Q_STEPS,
                                           v["out"], v["xu"], ops().code(xd), B, v["n"], stream), entry)
  torch.cuda.synchronize()
  assert bool(torch.isnan(of).all()) and bool(torch.isnan(uf).all())
