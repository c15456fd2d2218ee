"""DDIM inversion on the GPU, all through the C ABI: the update kernel against the float64
restatement (tests/inversion_ref.py), the inverse against the forward kernel, every element accounted for, the device
counter and the captured graph, whole loops against the restatement driven by the oracle's U-Net, sampling from a
given level, and the edit loop.

Gates.
  Kernel: the error of the existing ldm_cfg_ddim_update against its restatement on the same inputs at sigma = 0,
    measured in the same run, floored at 2^-23 relative, times 2 for rounding order.  The float32 NumPy emulation of
    the two directions gives inversion / forward error ratios of 0.43 .. 0.89 (x') and 0.31 .. 0.64 (x0) on these
    inputs, all below 2, so the factor stays 2.
  Round trip: 4 * 2^-23 relative L2 (the emulation gives 0.12 .. 0.59 at unit-variance eps; 4 covers fma contraction).
  Loops: the error of ddim_p_sample_loop against O.ddim_p_sample_loop at the same scale, weights and dtype, measured
    in the same run, times LOOP_MARGIN = 8: between a float32 and a float64 run of the two restatements on the oracle's
    U-Net at these shapes the inversion drifts 3.92 (g = 1) and 5.46 (g = 3) times as far as the sampling loop, rounded
    up to a power of two.
Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deis_ref as D  # noqa: E402
import inversion_ref as I  # noqa: E402
import plms_ref as P  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd._lib import LdmHipError  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, HW, N, LDM = T.B, T.HW, T.N, T.LDM
SHAPE = [B, HW, HW, 4]
FLOOR = 2.0 ** -23
LOOP_MARGIN = 8.
CANARY = -12288.                               # (exact in bfloat16)
PAD = 64                                       # floats around every output (a multiple of 4: the views stay aligned)


def _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="ddim", use_graph=True, temb_table=True, skip_unguided=True):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**T.UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=T.CTX_DIM)
  ae = AutoencoderKL(**T.KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**T.TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, temb_table=temb_table,
                                     sampler=sampler, skip_unguided=skip_unguided, **LDM)


def _x_T():
  return np.random.default_rng(9).standard_normal((B, HW, HW, 4)).astype(np.float32)


def _z0():
  return (0.8 * np.random.default_rng(12).standard_normal((B, HW, HW, 4))).astype(np.float32)


def _other_ids():
  ids = T._ids().copy()
  ids[B:] = np.random.default_rng(2).integers(0, 1000, size=(1, 77))
  return ids


def rel64(got, ref):
  got = np.asarray(got.detach().float().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
  ref = np.asarray(ref.detach().cpu() if isinstance(ref, torch.Tensor) else ref, dtype=np.float64)
  return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def _model():
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  m = LatentDiffusionModel(None, None, None, **LDM)
  return m, I.make_tables(m._alphas_cumprod, m._ddim_steps)


def _kernel_inputs():
  g = torch.Generator().manual_seed(4)
  return dict(eps_all=torch.randn(2 * B, HW, HW, 4, generator=g), xt=torch.randn(B, HW, HW, 4, generator=g))


def _run_invert(dev, m, eps_all, xt, idx, guided, gs, x_dtype=torch.float32, dec=False):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty_like(xt, device=dev), torch.empty_like(xt, device=dev)
  xu = torch.empty((2 * xt.shape[0],) + tuple(xt.shape[1:]), device=dev, dtype=x_dtype)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  ops.cfg_ddim_invert_update(d(eps_all), d(xt), out, m._coef_dev, index, guided, gs, x_unet_out=xu, dec_index=dec,
                             pred_x0_out=px)
  assert index.item() == (idx - 1 if dec else idx)
  return out.cpu(), px.cpu(), xu.cpu()


def _run_ddim(dev, m, eps_all, xt, idx, gs):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty_like(xt, device=dev), torch.empty_like(xt, device=dev)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  ops.cfg_ddim_update(d(eps_all), d(xt), out, m._coef_dev, index, gs, pred_x0_out=px)
  return out.cpu(), px.cpu()


def _kernel_gate(dev, m, tab, t, idx, gs):
  """2 * max(error of ldm_cfg_ddim_update against its restatement on the same inputs, 2^-23), for x' and x0."""
  d = lambda a: a.double().numpy()
  b = t["xt"].shape[0]
  e = I.guided(d(t["eps_all"][:b]), d(t["eps_all"][b:]), gs)
  want, want0 = I.forward_update(d(t["xt"]), e, idx, tab)
  got, got0 = _run_ddim(dev, m, t["eps_all"], t["xt"], idx, gs)
  return 2 * max(rel64(got, want), FLOOR), 2 * max(rel64(got0, want0), FLOOR)


# ---- 1. the kernel against the float64 restatement -------------------------------------------------------
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("guided", [True, False], ids=["g5", "cond_only"])
def test_kernel_against_float64_restatement(dev, guided, x_dtype):
  m, tab = _model()
  t = _kernel_inputs()
  gs = 5. if guided else 1.
  d = lambda a: a.double().numpy()
  for idx in (N - 1, 5, 1, 0):
    gate, gate0 = _kernel_gate(dev, m, tab, t, idx, gs)
    want, want0 = I.invert_update(d(t["xt"]), d(t["eps_all"][:B]), d(t["eps_all"][B:]), gs, idx, tab)
    # (the conditional-only form is handed a scale it must ignore)
    got, got0, xu = _run_invert(dev, m, t["eps_all"], t["xt"], idx, guided, gs if guided else 7., x_dtype)
    r, r0 = rel64(got, want), rel64(got0, want0)
    print(f"invert idx={idx} guided={guided}: x {r:.3e} (gate {gate:.3e}, ratio to forward {2 * r / gate:.2f}); "
          f"x0 {r0:.3e} (gate {gate0:.3e}, ratio {2 * r0 / gate0:.2f})")
    assert r <= gate and r0 <= gate0, (idx, r, gate, r0, gate0)
    assert torch.equal(xu[:B], got.to(x_dtype)) and torch.equal(xu[B:], got.to(x_dtype))   # rounded once
    # in place, and with the decrement: the same bits, the counter one lower
    dec, _, _ = _run_invert(dev, m, t["eps_all"], t["xt"], idx, guided, gs, x_dtype, dec=True)
    assert torch.equal(dec, got)
    x = t["xt"].to(dev)
    index = torch.tensor([idx], dtype=torch.int32, device=dev)
    ops.cfg_ddim_invert_update(t["eps_all"].to(dev), x, x, m._coef_dev, index, guided, gs)
    assert torch.equal(x.cpu(), got)


# ---- 2. the inverse undoes the forward kernel ------------------------------------------------------------
@pytest.mark.parametrize("guided", [True, False], ids=["guided_g1", "cond_only"])
def test_inverse_undoes_the_forward_kernel(dev, guided):
  """Unit-variance eps, the same bits on both sides: guided, both kernels form e_u + 1 * (e_c - e_u); conditional-only,
  the forward kernel is given a zero unconditional half (0 + 1 * (e_c - 0) = e_c exactly) and the inverse reads e_c
  alone.  (g = 5 is printed: its eps is 6.4 times as large as x, and the bound is relative to x.)"""
  m, _ = _model()
  t = _kernel_inputs()
  eps_all = t["eps_all"].clone()
  if not guided:
    eps_all[:B] = 0.
  for idx in range(N):
    fwd, _ = _run_ddim(dev, m, eps_all, t["xt"], idx, 1.)
    back, _, _ = _run_invert(dev, m, eps_all, fwd, idx, guided, 1.)
    r = rel64(back, t["xt"])
    f5, _ = _run_ddim(dev, m, t["eps_all"], t["xt"], idx, 5.)
    r5 = rel64(_run_invert(dev, m, t["eps_all"], f5, idx, True, 5.)[0], t["xt"])
    print(f"round trip idx={idx} guided={guided}: {r / FLOOR:.2f} x 2^-23   (g = 5: {r5 / FLOOR:.2f} x 2^-23)")
    assert r <= 4 * FLOOR, (idx, r / FLOOR)


# ---- 3. accounting ---------------------------------------------------------------------------------------
def _padded(dev, numel, dtype=torch.float32):
  buf = torch.full((numel + 2 * PAD,), CANARY, dtype=dtype, device=dev)
  return buf, buf[PAD:PAD + numel]


@pytest.mark.parametrize("shape", [(1, 4), (2, 1024), (5, 262144)], ids=["1x4", "2x1024", "5x262144"])
@pytest.mark.parametrize("guided", [True, False], ids=["g5", "cond_only"])
def test_every_element_is_written_once_and_nothing_else(dev, guided, shape):
  m, tab = _model()
  b, n = shape
  g = torch.Generator().manual_seed(7)
  eps_all, xt = torch.randn(2 * b, n, generator=g), torch.randn(b, n, generator=g)
  gs, idx = (5. if guided else 1.), 5
  want, want0 = I.invert_update(xt.double().numpy(), eps_all[:b].double().numpy(), eps_all[b:].double().numpy(), gs,
                                idx, tab)
  gate, gate0 = _kernel_gate(dev, m, tab, dict(eps_all=eps_all, xt=xt), idx, gs)     # (the gate of test 1, these inputs)
  if not guided:
    eps_all[:b] = float("nan")                 # the conditional-only form never loads the unconditional half
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  for x_dtype in (torch.float32, torch.bfloat16):
    (bo, out), (bp, px), (bu, xu) = _padded(dev, b * n), _padded(dev, b * n), _padded(dev, 2 * b * n, x_dtype)
    ops.cfg_ddim_invert_update(eps_all.to(dev), xt.to(dev), out.view(b, n), m._coef_dev, index, guided, gs,
                               x_unet_out=xu.view(2 * b, n), pred_x0_out=px.view(b, n))
    for buf in (bo, bp, bu):                   # nothing outside
      assert (buf[:PAD] == CANARY).all() and (buf[-PAD:] == CANARY).all()
    for o in (out, px, xu):                    # every element written, with a finite value
      assert torch.isfinite(o.float()).all() and not (o == CANARY).any()
    assert rel64(out.view(b, n), want) <= gate and rel64(px.view(b, n), want0) <= gate0
    half = out.view(b, n).to(x_dtype)
    assert torch.equal(xu.view(2, b, n)[0], half) and torch.equal(xu.view(2, b, n)[1], half)


def test_rejects_what_it_cannot_vectorise(dev):
  m, _ = _model()
  i = torch.tensor([3], dtype=torch.int32, device=dev)
  z = lambda *s: torch.zeros(*s, device=dev)
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.cfg_ddim_invert_update(z(4, 6), z(2, 6), z(2, 6), m._coef_dev, i, True, 5.)
  for bad in ("xt", "xt_out", "pred_x0_out", "x_unet_out", "eps_all"):
    a = dict(eps_all=z(4, 8), xt=z(2, 8), xt_out=z(2, 8), pred_x0_out=z(2, 8), x_unet_out=z(4, 8))
    numel = a[bad].numel()
    a[bad] = z(numel + 4)[1:1 + numel].view(-1, 8)                       # 4 bytes off a 16-byte boundary
    with pytest.raises(LdmHipError, match="16-byte aligned"):
      ops.cfg_ddim_invert_update(a["eps_all"], a["xt"], a["xt_out"], m._coef_dev, i, False, 1.,
                                 x_unet_out=a["x_unet_out"], pred_x0_out=a["pred_x0_out"])
  with pytest.raises(LdmHipError, match="null pointer"):
    ops.check(ops.lib.ldm_cfg_ddim_invert_update(None, None, None, None, None, 0, None, None, 0, 0, 1., 2, 8, None),
              "ldm_cfg_ddim_invert_update")
  assert i.item() == 3


# ---- 4. the counter and the graph ------------------------------------------------------------------------
@pytest.mark.parametrize("temb_table", [True, False])
def test_counter_after_k_steps(dev, unet_w, txt_w, kl_w, temb_table):
  """Route (b): the counter walks down over reversed tables.  From reset it holds N (a pre-decrementing step) or
  N - 1 (the four temb launches; the update decrements afterwards); after k steps that value minus k."""
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False, temb_table=temb_table)
  for strength, k in ((0.3, 3), (1.0, N)):
    rec = []
    s.ddim_invert_loop(T._ids(), latents=_z0(), strength=strength, record=rec)
    assert len(rec) == k and s._index_dev.item() == (N if temb_table else N - 1) - k
  coef, t_rev = s._invert_tables()
  assert torch.equal(coef, s._coef_dev.flip(0)) and t_rev.tolist() == I.t_in(s._ddim_steps)[::-1].tolist()


@pytest.mark.parametrize("gs", [1., 3.])
def test_graph_replay_equals_eager_and_captures_once(dev, unet_w, txt_w, kl_w, gs):
  ids, z0 = T._ids(), _z0()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=True)
  e = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  a3 = s.ddim_invert_loop(ids, latents=z0, guidance_scale=gs, strength=0.3)
  g = s._inv_graph
  assert g is not None and s._graph is None and s._inv_graph_key[0] == "invert"
  aN = s.ddim_invert_loop(ids, latents=z0, guidance_scale=gs, strength=1.0)
  assert s._inv_graph is g and s._index_dev.item() == 0                  # one capture serves every depth
  for strength, got in ((0.3, a3), (1.0, aN)):
    rec = []
    want = e.ddim_invert_loop(ids, latents=z0, guidance_scale=gs, strength=strength, record=rec)
    assert e._inv_graph is None and torch.equal(rec[-1], want)
    assert torch.equal(got, want) and got.dtype == torch.float32 and tuple(got.shape) == tuple(SHAPE)
  assert torch.equal(s._xt, aN) and aN.data_ptr() != s._xt.data_ptr()
  # the sampling graph lives beside it: inverting and sampling in turn recaptures nothing
  img = s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=aN, start_index=N)
  gd = s._graph
  assert gd is not None and s._inv_graph is g
  for _ in range(2):
    assert torch.equal(s.ddim_invert_loop(ids, latents=z0, guidance_scale=gs), aN)
    assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=aN, start_index=N), img)
    assert s._graph is gd and s._inv_graph is g
  # another scale is another captured argument (1 <-> a float: another form); the same scale again is not
  other = s.ddim_invert_loop(ids, latents=z0, guidance_scale=2.)
  assert s._inv_graph is not g and not torch.equal(other, aN)
  g2 = s._inv_graph
  s.ddim_invert_loop(ids, latents=z0, guidance_scale=2., strength=0.5)
  assert s._inv_graph is g2


def test_rejections(dev, unet_w, txt_w, kl_w):
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  ids, z0 = T._ids(), _z0()
  with pytest.raises(ValueError, match="schedule"):
    s.ddim_invert_loop(ids, latents=z0, guidance_scale=[1.] * N)
  with pytest.raises(ValueError, match="exactly one"):
    s.ddim_invert_loop(ids)
  with pytest.raises(ValueError, match="exactly one"):
    s.ddim_invert_loop(ids, init_images=T._inputs(0.)[0], latents=z0)
  for strength in (0., 1.5, 0.05):
    with pytest.raises(ValueError, match="strength"):
      s.ddim_invert_loop(ids, latents=z0, strength=strength)
  with pytest.raises(ValueError, match="start_index"):
    s.ddim_p_sample_loop(ids, SHAPE, 5., start_index=3)
  for k in (0, N + 1):
    with pytest.raises(ValueError, match="start_index"):
      s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=z0, start_index=k)
  assert s._graph is None and s._inv_graph is None


# ---- 5. loops against the reference composition ----------------------------------------------------------
_CACHE = {}


def _eps_fn(w, ids, gs):
  """The oracle's U-Net in float32 as inversion_ref's callback: the conditional rows alone at g = 1."""
  ctx = O.text_encoder(ids, w["cond_stage_model"], torch.float32)

  def fn(x, t):
    x = torch.from_numpy(np.ascontiguousarray(x))
    if gs == 1:
      return None, O.unet_forward(x, np.full([B], t, np.int32), ctx[B:], w["unet"], torch.float32).numpy()
    e = O.unet_forward(torch.cat([x, x]), np.full([2 * B], t, np.int32), ctx, w["unet"], torch.float32).numpy()
    return e[:B], e[B:]
  return fn


def _ref(kind, w, **kw):
  """Reference loops in float32 on the oracle's U-Net, computed once (arrays are keyed by the names given along)."""
  key = (kind,) + tuple(sorted((k, v if np.ndim(v) == 0 else "arr") for k, v in kw.items()))
  if key in _CACHE:
    return _CACHE[key]
  m, _ = _model()
  tab, steps = I.make_tables(m._alphas_cumprod, m._ddim_steps, np.float32), m._ddim_steps
  if kind == "invert":
    out = I.invert_loop(_eps_fn(w, kw["ids"], kw["gs"]), kw["z0"], kw["gs"], kw["k"], steps, tab, dtype=np.float32)
  elif kind == "sample":
    out = I.sample_loop(_eps_fn(w, kw["ids"], kw["gs"]), kw["x"], kw["gs"], kw["k"], steps, tab, dtype=np.float32)
  else:
    rec = []
    O.ddim_p_sample_loop(T._ids(), _x_T(), w, LDM, guidance_scale=kw["gs"], record=rec)
    out = rec[-1].numpy()
  assert out.dtype == np.float32
  _CACHE[key] = out
  return out


def _sampling_error(dev, dtype, w, gs):
  """The yardstick: ddim_p_sample_loop's latents against O.ddim_p_sample_loop's, same scale, weights, x_T, dtype."""
  key = ("base", dtype, gs)
  if key not in _CACHE:
    s = _sampler(dev, dtype, w["unet"], w["cond_stage_model"], w["autoencoder"])
    s.ddim_p_sample_loop(T._ids(), SHAPE, gs, x_T=_x_T())
    _CACHE[key] = rel64(s._xt, _ref("ddim", w, gs=gs))
  return _CACHE[key]


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("gs", [1., 3.])
def test_invert_loop_against_reference(dev, dtype, gs, unet_w, txt_w, kl_w):
  """Margin 8: inversion drift / sampling drift between float32 and float64 runs of the restatements on the oracle's
  U-Net, measured on the CPU at these shapes: 3.92 (g = 1), 5.46 (g = 3)."""
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = _sampling_error(dev, dtype, w, gs)
  ref = _ref("invert", w, ids=T._ids(), idn="ids", z0=_z0(), gs=gs, k=N)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  got = s.ddim_invert_loop(T._ids(), latents=_z0(), guidance_scale=gs)
  r = rel64(got, ref)
  print(f"invert loop g={gs} [{dtype}]: {r:.3e}; sampling loop {base:.3e}; gate {LOOP_MARGIN * base:.3e}")
  assert r <= LOOP_MARGIN * base, (r, base)


# ---- 6. conditional-only equals guided at g = 1 ----------------------------------------------------------
def test_cond_only_equals_guided_at_scale_one(dev, unet_w, txt_w, kl_w, monkeypatch):
  """Per step, from the same x: the B-row evaluation against the 2B-row one (other GEMM plans, so not bit for bit),
  within the kernel gate of test 1."""
  from ldm_tf2_amd.unet import UNet
  ids, z0 = T._ids(), _z0()
  rows = []
  fwd = UNet.forward
  monkeypatch.setattr(UNet, "forward", lambda self, x, *a, **k: (rows.append(x.shape[0]), fwd(self, x, *a, **k))[1])
  a = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False, skip_unguided=True)
  b = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False, skip_unguided=False)
  ra, rb = [], []
  a.ddim_invert_loop(ids, latents=z0, record=ra)
  assert rows == [B] * N
  del rows[:]
  b.ddim_invert_loop(ids, latents=z0, record=rb)
  assert rows == [2 * B] * N
  m, tab = _model()
  t = _kernel_inputs()
  for i in range(N):
    # one step of the conditional-only sampler from the guided loop's x
    x = torch.from_numpy(z0).to(dev) if i == 0 else rb[i - 1]
    a._xt.copy_(x), a._x2[:B].copy_(x), a._x2[B:].copy_(x)
    a._index_dev.fill_(a._invert_counter_start() - i)
    a._step_invert(1., True)
    gate = _kernel_gate(dev, m, tab, t, i, 1.)[0]
    r = rel64(a._xt, rb[i])
    print(f"cond-only vs guided, step {i}: {r:.3e} (gate {gate:.3e}); free-running {rel64(ra[i], rb[i]):.3e}")
    assert r <= gate, (i, r, gate)


# ---- 7. sampling from a given level ----------------------------------------------------------------------
def test_start_index_is_the_tail_of_a_full_loop(dev, unet_w, txt_w, kl_w):
  ids, x_T = T._ids(), _x_T()
  e = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=True)
  rec = []
  full = e.ddim_p_sample_loop(ids, SHAPE, 5., x_T=x_T, record=rec)
  assert torch.equal(full, s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=x_T))
  assert torch.equal(full, s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=x_T, start_index=N))
  g = s._graph
  for k in (N - 1, 3, 1):
    x = rec[N - 1 - k]                          # after the step at index k: on the level of steps[k-1]
    tail = []
    got = e.ddim_p_sample_loop(ids, SHAPE, 5., x_T=x, start_index=k, record=tail)
    assert len(tail) == k and all(torch.equal(p, q) for p, q in zip(tail, rec[N - k:]))
    assert torch.equal(got, full)
    assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=x, start_index=k), full) and s._graph is g
  # a guidance schedule walks its first k entries
  sched = [5.] * 4 + [1.] * (N - 4)
  rec = []
  full = e.ddim_p_sample_loop(ids, SHAPE, sched, x_T=x_T, record=rec)
  assert torch.equal(e.ddim_p_sample_loop(ids, SHAPE, sched, x_T=rec[N - 1 - 6], start_index=6), full)


@pytest.mark.parametrize("name", ["plms", "deis"])
def test_multistep_start_index_has_no_history(dev, name, unet_w, txt_w, kl_w):
  """Against the solver's own restatement (deis_ref.ms_update) started at index k - 1 without history, eps from the
  oracle's U-Net in float32.  Gate: the DDIM sampling loop's error times the largest sum_m |w[m]| of the weight rows
  the loop walks -- what a row does to a rounding error in eps, the reasoning of test_plms_gpu.py: 20 / 3 for PLMS (its
  third-order row); the DEIS rows of this coarse uniform table reach 72.1 (index 1, three earlier steps)."""
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  k, gs = 6, 5.
  base = _sampling_error(dev, torch.float32, w, gs)
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name)
  x = _x_T()
  s.ddim_p_sample_loop(T._ids(), SHAPE, gs, x_T=x, start_index=k)
  assert s._start.item() == k - 1
  # the specification as test_deis_gpu.py composes it: float32, the tables and the weight table cast to float32 first
  tab = I.make_tables(s._alphas_cumprod, s._ddim_steps, np.float32)
  wtab = D.weight_table(s._alphas_cumprod, s._ddim_steps).astype(np.float32) if name == "deis" else None
  pair = _eps_fn(w, T._ids(), gs)
  ref, hist = x, []
  for i in range(k - 1, -1, -1):
    e_u, e_c = pair(ref, int(s._ddim_steps[i]))
    hist.insert(0, e_u + np.float32(gs) * (e_c - e_u))
    del hist[4:]
    j = min(k - 1 - i, 3)
    wj = np.array(P.WEIGHTS[j], dtype=np.float32) if wtab is None else wtab[i, j]
    ref, _ = D.ms_update(ref, hist, i, j, wj, tab["c1"], tab["c2"], tab["a_prev"])
    assert ref.dtype == np.float32
  amp = 20. / 3.
  if name == "deis":
    w64 = D.weight_table(s._alphas_cumprod, s._ddim_steps)
    amp = max(amp, max(float(np.abs(w64[i, min(k - 1 - i, 3)]).sum()) for i in range(k)))
  r = rel64(s._xt, ref)
  print(f"{name} from start_index={k}: {r:.3e}; ddim loop {base:.3e}; sum|w| {amp:.2f}; gate {base * amp:.3e}")
  assert r <= base * amp, (r, base, amp)


# ---- 8. the edit loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_edit_loop(dev, dtype, unet_w, txt_w, kl_w):
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  ids, other = T._ids(), _other_ids()
  img, E, _, _, _ = T._inputs(0.)
  strength, k = 0.5, 5
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w)
  # reconstruction: the same ids, both scales 1
  base = _sampling_error(dev, dtype, w, 1.)
  out = s.ddim_p_sample_loop_edit(ids, ids, img, guidance_scale=1., strength=strength, encode_noise=E)
  assert tuple(out.shape) == (B, 8 * HW, 8 * HW, 3) and s._index_dev.item() == 0
  g_inv, g_smp = s._inv_graph, s._graph
  z0 = s._z0_buf.cpu().numpy()                 # the device's own z0: both sides start from the same latents
  up = _ref("invert", w, ids=ids, idn="ids", z0=z0, zn=str(dtype), gs=1., k=k)
  back = _ref("sample", w, ids=ids, idn="ids", x=up, xn="recon" + str(dtype), gs=1., k=k)
  d_got, d_ref = rel64(s._xt, z0), rel64(back, z0)
  print(f"reconstruction [{dtype}]: distance to z0 {d_got:.4e}, reference {d_ref:.4e}, "
        f"|diff| / reference {abs(d_got - d_ref) / d_ref:.3e} (gate {LOOP_MARGIN * base:.3e}); "
        f"latents against the reference round trip {rel64(s._xt, back):.3e}")
  assert abs(d_got - d_ref) <= LOOP_MARGIN * base * d_ref
  # another target prompt at g = 5: the composition of the two reference loops
  base5 = _sampling_error(dev, dtype, w, 5.)
  s.ddim_p_sample_loop_edit(ids, other, img, guidance_scale=5., strength=strength, encode_noise=E)
  assert s._inv_graph is g_inv and s._graph is not None                  # the same context shape: no recapture
  edit = _ref("sample", w, ids=other, idn="other", x=up, xn="edit" + str(dtype), gs=5., k=k)
  r = rel64(s._xt, edit)
  gate = LOOP_MARGIN * max(base, base5)
  print(f"edit [{dtype}]: {r:.3e}; sampling loops {base:.3e} (g = 1), {base5:.3e} (g = 5); gate {gate:.3e}")
  assert r <= gate, (r, gate)
  assert rel64(edit, back) > 100 * gate or dtype == torch.bfloat16       # (an edit is not the reconstruction)
  g5 = s._graph
  s.ddim_p_sample_loop_edit(ids, ids, img, guidance_scale=5., strength=0.3, encode_noise=E)
  assert s._graph is g5 and s._inv_graph is g_inv and g_smp is not None


@pytest.mark.parametrize("temb_table", [True, False])
def test_inversion_step_has_an_unguided_steps_launches(dev, unet_w, txt_w, kl_w, monkeypatch, temb_table):
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False, temb_table=temb_table)
  ids = T._ids()
  sched = [1.] * N
  s.ddim_p_sample_loop(ids, SHAPE, sched, x_T=_x_T(), record=[])          # allocates everything, fills the table
  s.ddim_invert_loop(ids, latents=_z0(), record=[])
  calls = {}
  for what in ("unguided", "invert"):
    proxy = T._CountingLib(ops.lib)
    if what == "unguided":
      s._index_dev.fill_(s._loop_start_index(4))
      monkeypatch.setattr(ops, "lib", proxy)
      s._step_sched(False, True)
    else:
      s._index_dev.fill_(s._invert_counter_start())
      monkeypatch.setattr(ops, "lib", proxy)
      s._step_invert(1., True)
    monkeypatch.setattr(ops, "lib", proxy._lib)
    torch.cuda.synchronize()
    calls[what] = proxy.calls
  print({k: len(v) for k, v in calls.items()})
  swap = lambda cs: ["ldm_cfg_ddim_invert_update" if c == "ldm_cfg_sched_update" else c for c in cs]
  assert calls["invert"] == swap(calls["unguided"]) and calls["invert"].count("ldm_cfg_ddim_invert_update") == 1
  assert calls["invert"][0] == ("ldm_select_row" if temb_table else "ldm_time_embedding")
