"""Step tables and the table-weighted multistep sampler on the GPU, all through the C ABI: the
fused update kernel against the float64 restatement (tests/deis_ref.py), against the PLMS kernel when fed its
constants, the slots it must not read, whole loops on the non-uniform tables against the oracle composition with the
restated tables, graph replay, the calls of a step and the untouched default.

Gates.  Kernel: the error of the existing ldm_cfg_ddim_update(_masked) against the same restatement on the same
inputs at sigma = 0, floored at 2^-23 relative, times 2 * sum_m |w_m| of the weight row in use (computed from the
float32 weights the kernel reads: what they do to a rounding error in eps; 2 for rounding order).  Loops: the
uniform-table DDIM loop's error against O.ddim_p_sample_loop on the same weights, x_T and dtype, measured in the same
run, times 20/3, and the project's loop gates (1.3e-5 f32 / 8e-2 bf16).
Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deis_ref as D  # noqa: E402
import plms_ref as P  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, HW, N, LDM = T.B, T.HW, T.N, T.LDM
GS = 5.
SHAPE = [B, HW, HW, 4]
FLOOR = 2.0 ** -23
SEED = (1 << 32) + 7
AB = D.alphas_cumprod(LDM["num_steps"], LDM["beta_start"], LDM["beta_end"])
# (sampler, step table, eta): the three forms the loops are checked in
FORMS = {"ddim": ("ddim", "logsnr", 1.), "plms": ("plms", "logsnr", 0.), "deis": ("deis", "karras", 0.)}


def _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="deis", spacing="karras", eta=0., use_graph=True,
             temb_table=True, noise_source="host", kwarg=True):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**T.UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=T.CTX_DIM)
  ae = AutoencoderKL(**T.KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**T.TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  kw = dict(step_spacing=spacing) if kwarg else {}
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, temb_table=temb_table,
                                     sampler=sampler, noise_source=noise_source, **kw, **dict(LDM, eta=eta))


def _x_T():
  return np.random.default_rng(9).standard_normal((B, HW, HW, 4)).astype(np.float32)


def rel64(got, ref):
  got = np.asarray(got.detach().float().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
  return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def _rng(dev, seed=SEED, first=0):
  seed = int(seed) % (1 << 64)
  w = np.array([seed & 0xffffffff, seed >> 32, first, 0], dtype=np.uint32)
  return torch.from_numpy(w.view(np.int32).copy()).to(dev)


# ---- 1. the kernel against the float64 restatement ------------------------------------------------------
def _kernel_weights(m):
  """float32 [N][4][4] for the kernel tests: the product's table on its step table; the rows (idx, j) with
  idx + j > N - 1, which no loop reaches (their history would lie above the table), hold the Adams-Bashforth
  constants so that every (idx, j) the test visits has a row."""
  w = m.multistep_weights().astype(np.float32)
  for i in range(N):
    for j in range(4):
      if i + j > N - 1:
        w[i, j, :j + 1] = np.array(P.WEIGHTS[j], dtype=np.float32)
  return w


def _kernel_inputs(dev, spacing="karras"):
  from ldm_tf2_amd.model_runners import LatentDiffusionModel
  m = LatentDiffusionModel(None, None, None, step_spacing=spacing, **LDM)
  assert m._ddim_steps.tolist() == D.step_table(AB, N, spacing).tolist()
  g = torch.Generator().manual_seed(4)
  t = dict(eps_all=torch.randn(2 * B, HW, HW, 4, generator=g), xt=torch.randn(B, HW, HW, 4, generator=g),
           ring=torch.randn(4, B, HW, HW, 4, generator=g), z0=torch.randn(B, HW, HW, 4, generator=g),
           Q=torch.randn(N, B, HW, HW, 4, generator=g), mask=torch.rand(B, HW, HW, generator=g))
  t["mask"][:, 0, :] = 1.
  t["mask"][:, 1, :] = 0.
  f = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
  tab = dict(c1=f(m._ddim_sqrt_recip_alphas_cumprod), c2=f(m._ddim_sqrt_recipm1_alphas_cumprod),
             a_prev=f(m._ddim_alphas_cumprod_prev), qa=f(m._sqrt_alphas_cumprod)[m._ddim_steps],
             qb=f(m._sqrt_one_minus_alphas_cumprod)[m._ddim_steps])
  return m, t, tab


def _device_Q(dev, t):
  """The Q table the fused path draws: row i = stream Q_STREAM + i (ldm_normal_fill forms the same numbers)."""
  from ldm_tf2_amd import model_runners as R
  rng = _rng(dev)
  q = torch.stack([ops.normal_fill(torch.empty(B, HW, HW, 4, device=dev), rng, R.Q_STREAM + i) for i in range(N)])
  return dict(t, Q=q.cpu())


def _restated(t, tab, w64, idx, j, masked):
  """(x', x0, e_i) of the specification in float64 on the float32 inputs and the float32 weights, widened."""
  d = lambda a: a.double().numpy()
  eu, ec = d(t["eps_all"][:B]), d(t["eps_all"][B:])
  e_i = eu + GS * (ec - eu)
  hist = [e_i] + [d(t["ring"][(idx + k) & 3]) for k in range(1, j + 1)]
  x, x0 = D.ms_update(d(t["xt"]), hist, idx, j, w64[idx, j], tab["c1"], tab["c2"], tab["a_prev"])
  if masked and idx >= 1:
    q = tab["qa"][idx - 1] * d(t["z0"]) + tab["qb"][idx - 1] * d(t["Q"][idx - 1])
    mk = d(t["mask"])[..., None]
    x = mk * q + (1 - mk) * x
  return x, x0, e_i


def _run_ms(dev, m, t, w32, idx, start, masked, x_dtype, dec, ring=None, draws=False):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
  xu = torch.empty(2 * B, HW, HW, 4, device=dev, dtype=x_dtype)
  ring = d(t["ring"] if ring is None else ring)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  st = torch.tensor([start], dtype=torch.int32, device=dev)
  wd = torch.from_numpy(np.ascontiguousarray(w32)).to(dev)
  kw = {}
  if masked:
    kw = dict(z0=d(t["z0"]), mask=d(t["mask"]), q_coef=m._device_q_tables()[2])
    if not draws:
      kw.update(q_noise=d(t["Q"]), q_index_stride=t["Q"][0].numel())
  if draws:
    ops.cfg_ms_update_rng(d(t["eps_all"]), d(t["xt"]), out, ring, m._coef_dev, index, st, wd, _rng(dev), GS,
                          x_unet_out=xu, dec_index=dec, pred_x0_out=px, **kw)
  else:
    ops.cfg_ms_update(d(t["eps_all"]), d(t["xt"]), out, ring, m._coef_dev, index, st, wd, GS, x_unet_out=xu,
                      dec_index=dec, pred_x0_out=px, **kw)
  assert index.item() == (idx - 1 if dec else idx) and st.item() == start
  return out.cpu(), px.cpu(), xu.cpu(), ring.cpu()


def _run_plms(dev, m, t, idx, start, masked, x_dtype):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
  xu = torch.empty(2 * B, HW, HW, 4, device=dev, dtype=x_dtype)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  st = torch.tensor([start], dtype=torch.int32, device=dev)
  kw = {}
  if masked:
    kw = dict(z0=d(t["z0"]), mask=d(t["mask"]), q_noise=d(t["Q"]), q_coef=m._device_q_tables()[2],
              q_index_stride=t["Q"][0].numel())
  ops.cfg_plms_update(d(t["eps_all"]), d(t["xt"]), out, d(t["ring"]), m._coef_dev, index, st, GS, x_unet_out=xu,
                      pred_x0_out=px, **kw)
  return out.cpu(), px.cpu(), xu.cpu()


def _run_ddim(dev, m, t, idx, masked):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  if masked:
    ops.cfg_ddim_update_masked(d(t["eps_all"]), d(t["xt"]), out, m._coef_dev, index, GS, d(t["z0"]), d(t["mask"]),
                               d(t["Q"]), m._device_q_tables()[2], q_index_stride=t["Q"][0].numel(), pred_x0_out=px)
  else:
    ops.cfg_ddim_update(d(t["eps_all"]), d(t["xt"]), out, m._coef_dev, index, GS, pred_x0_out=px)
  return out.cpu(), px.cpu()


@pytest.mark.parametrize("noise", ["table", "device"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_kernel_against_float64_restatement(dev, x_dtype, masked, noise):
  m, t, tab = _kernel_inputs(dev)
  draws = noise == "device"
  if draws:
    t = _device_Q(dev, t)                       # the table kernels and the restatement read what the launch draws
  w32 = _kernel_weights(m)
  w64 = w32.astype(np.float64)
  ident = np.zeros_like(w64)
  ident[:, :, 0] = 1.
  worst = {}
  for idx in (N - 1, 5, 1, 0):
    want_d, want_d0, _ = _restated(t, tab, ident, idx, 0, masked)   # sigma = 0 DDIM == order 0
    dd, dd0 = _run_ddim(dev, m, t, idx, masked)
    base, base0 = max(rel64(dd, want_d), FLOOR), max(rel64(dd0, want_d0), FLOOR)
    for j in range(4):
      want, want0, e_i = _restated(t, tab, w64, idx, j, masked)
      dec = bool((idx + j) & 1)
      got, px, xu, ring = _run_ms(dev, m, t, w32, idx, idx + j, masked, x_dtype, dec, draws=draws)
      r, r0 = rel64(got, want), rel64(px, want0)
      gate = 2 * float(np.abs(w64[idx, j, :j + 1]).sum())
      print(f"idx={idx} j={j} masked={masked} noise={noise}: ms {r:.3e} / x0 {r0:.3e}; ddim {base:.3e} / x0 "
            f"{base0:.3e}; sum|w| {gate / 2:.3f}; gate x{gate:.2f}; ratios {r / base:.3f} / {r0 / base0:.3f}")
      worst[j] = max(worst.get(j, 0.), r / base, r0 / base0)
      assert r <= gate * base and r0 <= gate * base0, (idx, j, r, r0, base, base0, gate)
      assert torch.equal(xu[:B], got.to(x_dtype)) and torch.equal(xu[B:], got.to(x_dtype))
      assert rel64(ring[idx & 3], e_i) <= 8 * 2.0 ** -24
      for k in range(1, 4):
        assert torch.equal(ring[(idx + k) & 3], t["ring"][(idx + k) & 3])
      if masked:
        plain = _run_ms(dev, m, t, w32, idx, idx + j, False, x_dtype, dec, draws=draws)
        assert torch.equal(px, plain[1]) and torch.equal(ring, plain[3])
        if idx == 0:                                                # nothing is blended (or drawn) at index 0
          assert torch.equal(got, plain[0]) and torch.equal(xu, plain[2])
        else:
          assert not torch.equal(got, plain[0]) and torch.equal(got[:, 1], plain[0][:, 1])
      if draws:                                                     # the drawn Q is the table's: same bits
        tabled = _run_ms(dev, m, t, w32, idx, idx + j, masked, x_dtype, dec, draws=False)
        assert all(torch.equal(a, b_) for a, b_ in zip((got, px, xu, ring), tabled))
  print("worst error in units of the DDIM kernel's:", {j: round(v, 3) for j, v in worst.items()})


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fed_the_plms_constants_it_agrees_with_the_plms_kernel(dev, x_dtype, masked):
  """Same gate as above, both kernels against the restatement with the float32 constants; bit equality is not
  required (the PLMS kernel carries numerators over a denominator) and what is observed is printed."""
  m, t, tab = _kernel_inputs(dev, spacing="uniform")
  w32 = np.zeros((N, 4, 4), dtype=np.float32)
  for j in range(4):
    w32[:, j, :j + 1] = np.array(P.WEIGHTS[j], dtype=np.float32)
  w64 = w32.astype(np.float64)
  equal = {}
  for idx in (N - 1, 5, 1, 0):
    dd, _ = _run_ddim(dev, m, t, idx, masked)
    base = max(rel64(dd, _restated(t, tab, w64, idx, 0, masked)[0]), FLOOR)
    for j in range(4):
      got = _run_ms(dev, m, t, w32, idx, idx + j, masked, x_dtype, False)
      ref = _run_plms(dev, m, t, idx, idx + j, masked, x_dtype)
      gate = 2 * float(np.abs(w64[idx, j]).sum()) * base
      d = rel64(got[0], ref[0].double().numpy())
      same = torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
      equal[j] = equal.get(j, True) and same
      print(f"idx={idx} j={j} masked={masked}: ms vs plms kernel rel {d:.3e} (gate {gate:.3e}), bit-identical {same}")
      assert d <= gate, (idx, j, d, gate)
  print("bit-identical to the PLMS kernel for every idx:", equal)


def test_start_below_index_and_far_above_clamp(dev):
  m, t, _ = _kernel_inputs(dev)
  w32 = _kernel_weights(m)
  a = _run_ms(dev, m, t, w32, 5, 5, False, torch.float32, False)
  b = _run_ms(dev, m, t, w32, 5, 2, False, torch.float32, False)    # start < idx: order 0
  assert torch.equal(a[0], b[0])
  c = _run_ms(dev, m, t, w32, 5, 8, False, torch.float32, False)
  e = _run_ms(dev, m, t, w32, 5, 9, False, torch.float32, False)    # start - idx > 3: order 3
  assert torch.equal(c[0], e[0]) and not torch.equal(a[0], c[0])
  dd, _ = _run_ddim(dev, m, t, 5, False)                            # order 0 is the DDIM step at sigma = 0
  assert rel64(a[0], dd.double().numpy()) <= 4 * FLOOR


def test_rejects_what_it_cannot_vectorise(dev):
  from ldm_tf2_amd._lib import LdmHipError
  i = torch.zeros(1, dtype=torch.int32, device=dev)
  coef = torch.zeros(10, 4, device=dev)
  w = torch.zeros(10, 4, 4, device=dev)
  x = torch.zeros(2, 3, 3, 3, device=dev)                           # n_per_sample = 27
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.cfg_ms_update(torch.zeros(4, 3, 3, 3, device=dev), x, x.clone(), torch.zeros(4, 2, 3, 3, 3, device=dev),
                      coef, i, i.clone(), w, GS)
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.cfg_ms_update_rng(torch.zeros(4, 3, 3, 3, device=dev), x, x.clone(), torch.zeros(4, 2, 3, 3, 3, device=dev),
                          coef, i, i.clone(), w, _rng(dev), GS)
  y = torch.zeros(2 * 16 + 1, device=dev)[1:].view(2, 4, 4, 1)      # 4-byte aligned only
  with pytest.raises(LdmHipError, match="aligned"):
    ops.cfg_ms_update(torch.zeros(4, 4, 4, 1, device=dev), y, torch.zeros(2, 4, 4, 1, device=dev),
                      torch.zeros(4, 2, 4, 4, 1, device=dev), coef, i, i.clone(), w, GS)


# ---- 2. slots beyond j are not read -----------------------------------------------------------------------
def test_slots_beyond_j_are_not_read(dev, unet_w, txt_w, kl_w):
  m, t, _ = _kernel_inputs(dev)
  w32 = _kernel_weights(m)
  for draws in (False, True):
    for idx in (N - 1, 5, 0):
      for j in (0, 1, 2):
        rings = []
        for fill in (float("nan"), 0.):
          ring = torch.full_like(t["ring"], fill)
          for k in range(1, j + 1):
            ring[(idx + k) & 3] = t["ring"][(idx + k) & 3]
          rings.append(_run_ms(dev, m, t, w32, idx, idx + j, True, torch.float32, False, ring=ring, draws=draws))
        (a, a0, au, _), (z, z0, zu, _) = rings
        assert bool(torch.isfinite(a).all() and torch.isfinite(a0).all() and torch.isfinite(au).all())
        assert torch.equal(a, z) and torch.equal(a0, z0) and torch.equal(au, zu)
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  first = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T()).clone()
  s._ring.fill_(float("nan"))
  again = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T())
  assert bool(torch.isfinite(again).all()) and torch.equal(first, again)


# ---- 3. whole loops on the non-uniform tables against the oracle composition ---------------------------------
_CACHE = {}


def _schedule(spacing, eta):
  """O.make_schedule's dictionary with every table restated from tests/deis_ref.py's step table."""
  sched = O.make_schedule(LDM["num_steps"], LDM["beta_start"], LDM["beta_end"], eta, N)
  assert np.array_equal(sched["alphas_cumprod"], AB)
  steps = D.step_table(AB, N, spacing).astype(np.int32)
  ab, ab_prev = D.derived_tables(AB, steps)
  return dict(ddim_steps=steps, alphas_cumprod=AB, ddim_alphas_cumprod_prev=ab_prev,
              ddim_sigmas=eta * np.sqrt((1 - ab_prev) / (1 - ab) * (1 - ab / ab_prev)),
              ddim_sqrt_recip_alphas_cumprod=np.sqrt(1. / AB)[steps],
              ddim_sqrt_recipm1_alphas_cumprod=np.sqrt(1. / AB - 1)[steps])


def _oracle_steps(form, context, w_unet, x, start, blend=None, noises=None):
  """`start + 1` steps of the specification in float32 torch on the restated tables: O.unet_forward on [x; x], CFG,
  then O.ddim_update (ddim) or deis_ref.ms_update with the Adams-Bashforth rows (plms) or the restated weight table
  cast to float32 (deis).  Returns [(x after the step, its pred_x0)]."""
  name, spacing, eta = FORMS[form]
  sched = _schedule(spacing, eta)
  f = lambda key: np.asarray(sched[key]).astype(np.float32)
  c1, c2, a_prev = f("ddim_sqrt_recip_alphas_cumprod"), f("ddim_sqrt_recipm1_alphas_cumprod"), f("ddim_alphas_cumprod_prev")
  steps = sched["ddim_steps"]
  wtab = D.weight_table(AB, steps).astype(np.float32) if name == "deis" else None
  x = torch.as_tensor(x, dtype=torch.float32)
  hist, rec = [], []
  for i in range(start, -1, -1):
    t = np.full([2 * B], steps[i], dtype=np.int32)
    eps_all = O.unet_forward(torch.cat([x, x], 0), t, context, w_unet, torch.float32)
    if name == "ddim":
      nz = torch.zeros_like(x) if noises is None else noises[i]
      x, x0 = O.ddim_update(x, eps_all[:B], eps_all[B:], sched, i, GS, nz)
    else:
      hist.insert(0, eps_all[:B] + np.float32(GS) * (eps_all[B:] - eps_all[:B]))
      del hist[4:]
      j = min(start - i, 3)
      w = np.array(P.WEIGHTS[j], dtype=np.float32) if wtab is None else wtab[i, j]
      x, x0 = D.ms_update(x, hist, i, j, w, c1, c2, a_prev)
    assert x.dtype == torch.float32
    if blend is not None and i >= 1:
      mask, z0, Q = blend
      x = T.blend_ref(mask, T.q_sample_ref(AB, z0, [steps[i - 1]] * B, Q[i - 1]), x)
    rec.append((x.clone(), x0.clone()))
  return rec


def _noises(eta):
  return np.random.default_rng(33).standard_normal((N, B, HW, HW, 4)).astype(np.float32) if eta else None


def _oracle(form, kind, w):
  key = (form, kind)
  if key in _CACHE:
    return _CACHE[key]
  eta = FORMS[form][2]
  context = O.text_encoder(T._ids(), w["cond_stage_model"], torch.float32)
  dec = lambda z: O.decoder_forward(z / LDM["scale_factor"], w["autoencoder"])
  nz = _noises(eta)
  nz_t = None if nz is None else torch.from_numpy(nz)
  if kind == "txt2img":
    rec = _oracle_steps(form, context, w["unet"], _x_T(), N - 1, noises=nz_t)
  else:
    k, masked = kind
    img, E, Q, _, mask = T._inputs(0.)
    _, _, sample = O.diagonal_gaussian(O.encoder_forward(torch.from_numpy(img), w["autoencoder"]), E)
    z0 = np.float32(LDM["scale_factor"]) * sample
    steps = D.step_table(AB, N, FORMS[form][1])
    x = T.q_sample_ref(AB, z0, [steps[k - 1]] * B, Q[k - 1])
    rec = _oracle_steps(form, context, w["unet"], x, k - 1, (mask, z0, Q) if masked else None, noises=nz_t)
  _CACHE[key] = dict(images=dec(rec[-1][0]), rec=rec)
  return _CACHE[key]


def _ddim_loop_error(dev, dtype, w):
  """The DDIM loop on the uniform table against O.ddim_p_sample_loop, same weights, x_T and dtype: the base of the
  loop gates."""
  key = ("base", dtype)
  if key not in _CACHE:
    s = _sampler(dev, dtype, w["unet"], w["cond_stage_model"], w["autoencoder"], sampler="ddim", kwarg=False)
    got = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T())
    _CACHE[key] = T.rel_err(got, O.ddim_p_sample_loop(T._ids(), _x_T(), w, LDM, guidance_scale=GS))[0]
  return _CACHE[key]


def _loop_check(what, got, ref, dtype, base):
  r = T.rel_err(got, ref)[0]
  print(f"{what} [{dtype}]: loop {r:.3e}; uniform ddim loop {base:.3e}; gate {base * 20 / 3:.3e}; "
        f"the project's loop gate {T.LOOP_REL[dtype]:.1e}")
  assert r <= base * 20. / 3., (what, r, base)
  assert r <= T.LOOP_REL[dtype], (what, r)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_loops_against_oracle(dev, form, dtype, unet_w, txt_w, kl_w):
  """txt2img, img2img k = 3, inpainting (k = 8) and the progressive frames of one form."""
  name, spacing, eta = FORMS[form]
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = _ddim_loop_error(dev, dtype, w)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, eta=eta)
  assert s._ddim_steps.tolist() == D.step_table(AB, N, spacing).tolist()
  nz = _noises(eta)
  ref = _oracle(form, "txt2img", w)
  got = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T(), noises=nz).clone()
  _loop_check(f"{form}/{spacing} txt2img latents", s._xt, ref["rec"][-1][0], dtype, base)
  _loop_check(f"{form}/{spacing} txt2img images", got, ref["images"], dtype, base)
  # the table matters: the same solver on the uniform table lands elsewhere
  uni = _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler=name, spacing="uniform", eta=eta)
  other = uni.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=_x_T(), noises=nz)
  assert T.rel_err(other, ref["images"])[0] > 10 * T.LOOP_REL[torch.float32]
  img, E, Q, _, mask = T._inputs(0.)
  for strength, msk, kind in ((0.3, None, (3, False)), (0.8, mask, (8, True))):
    ref = _oracle(form, kind, w)
    got = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=strength, mask=msk, encode_noise=E, q_noises=Q,
                                       noises=nz)
    what = f"{form}/{spacing} " + ("inpainting" if kind[1] else "img2img") + f" k={kind[0]}"
    _loop_check(what + " latents", s._xt, ref["rec"][-1][0], dtype, base)
    _loop_check(what + " images", got, ref["images"], dtype, base)
  ref = _oracle(form, "txt2img", w)
  freq = 5
  gi, gsm, gx = s.ddim_p_sample_loop_progressive(T._ids(), SHAPE, GS, record_freq=freq, x_T=_x_T(), noises=nz)
  assert tuple(gsm.shape) == (B, N // freq, 8 * HW, 8 * HW, 3) and tuple(gx.shape) == tuple(gsm.shape)
  dec = lambda z: O.decoder_forward(z / LDM["scale_factor"], w["autoencoder"])
  _loop_check(f"{form}/{spacing} progressive images", gi, ref["images"], dtype, base)
  for r in range(N // freq):                                        # slot r keeps the step at index r * freq
    x, x0 = ref["rec"][N - 1 - r * freq]
    _loop_check(f"{form}/{spacing} progressive sample frame {r}", gsm[:, r], dec(x), dtype, base)
    _loop_check(f"{form}/{spacing} progressive pred_x0 frame {r}", gx[:, r], dec(x0), dtype, base)


@pytest.mark.parametrize("form", list(FORMS))
def test_device_noise_runs_on_any_table(dev, form, unet_w, txt_w, kl_w):
  """noise_source="device" on the non-uniform tables: the fused draws against the same loop fed ldm_normal_fill's
  tables (txt2img with eta noise for ddim; inpainting with the blend's Q for every form).  plms and deis: bit for bit
  (the table and the drawing launch share their arithmetic).  ddim: the table entries are the scalar kernels, whose
  roundings differ from the four-wide drawing kernel's, so the gate is tests/test_device_noise_gpu.py's for the same
  comparison on the uniform table, 1e-5 relative."""

  def same(a, b_, what):
    r = T.rel_err(a, b_.cpu())[0]
    print(f"{form}/{spacing} {what}: fused against tabled rel {r:.3e}, bit-equal {torch.equal(a, b_)}")
    return r < 1e-5 if name == "ddim" else torch.equal(a, b_)
  from ldm_tf2_amd import model_runners as R
  name, spacing, eta = FORMS[form]
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, eta=eta, noise_source="device")
  img, E, _, _, mask = T._inputs(0.)
  x_T = _x_T()
  rng = _rng(dev)
  fill = lambda stream: torch.stack([ops.normal_fill(torch.empty(B, HW, HW, 4, device=dev), rng, stream + i)
                                     for i in range(N)])
  eta_tab, q_tab = (fill(R.ETA_STREAM) if eta else None), fill(R.Q_STREAM)
  fused = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=x_T, seed=SEED).clone()
  tabled = s.ddim_p_sample_loop(T._ids(), SHAPE, GS, x_T=x_T, seed=SEED, noises=eta_tab)
  assert bool(torch.isfinite(fused).all()) and same(fused, tabled, "txt2img")
  fused = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=0.8, mask=mask, encode_noise=E, seed=SEED).clone()
  tabled = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=0.8, mask=mask, encode_noise=E, seed=SEED,
                                        q_noises=q_tab, noises=eta_tab)
  assert bool(torch.isfinite(fused).all()) and same(fused, tabled, "inpainting")


# ---- 4. graph ---------------------------------------------------------------------------------------------
def test_graph_replay_eager_and_one_graph_for_every_start_and_seed(dev, unet_w, txt_w, kl_w):
  ids, x_T = T._ids(), _x_T()
  img, E, Q, _, mask = T._inputs(0.)
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=True)
  got = s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T).clone()
  g = s._graph
  assert g is not None and s._graph_key[-1] == "deis" and "karras" in s._graph_key
  assert torch.equal(got, s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T))          # a second replay
  e = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  assert torch.equal(got, e.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T)) and e._graph is None
  assert torch.equal(s._ring, e._ring) and e._start.item() == N - 1
  # img2img: its first loop allocates the init-latent buffers (a new buffer drops the graph) and captures again;
  # every start index, and txt2img, then replay that one graph
  g = None
  for strength in (0.3, 0.5, 1.0):
    out = s.ddim_p_sample_loop_img2img(ids, img, GS, strength=strength, encode_noise=E, q_noises=Q).clone()
    assert torch.equal(out, e.ddim_p_sample_loop_img2img(ids, img, GS, strength=strength, encode_noise=E, q_noises=Q))
    assert s._start.item() == int(strength * N) - 1
    assert g is None or s._graph is g
    g = s._graph
  assert torch.equal(got, s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T)) and s._graph is g
  # device noise: one graph for every seed
  d = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, noise_source="device")
  de = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, noise_source="device", use_graph=False)
  a = d.ddim_p_sample_loop_img2img(ids, img, GS, strength=0.8, mask=mask, encode_noise=E, seed=1).clone()
  gd = d._graph
  b_ = d.ddim_p_sample_loop_img2img(ids, img, GS, strength=0.5, mask=mask, encode_noise=E, seed=2).clone()
  assert d._graph is gd and not torch.equal(a, b_)
  assert torch.equal(a, de.ddim_p_sample_loop_img2img(ids, img, GS, strength=0.8, mask=mask, encode_noise=E, seed=1))
  assert torch.equal(b_, de.ddim_p_sample_loop_img2img(ids, img, GS, strength=0.5, mask=mask, encode_noise=E, seed=2))


def test_no_stale_history_between_loops(dev, unet_w, txt_w, kl_w):
  ids, x_T = T._ids(), _x_T()
  img, E, Q, _, mask = T._inputs(0.)
  kw = dict(strength=0.5, encode_noise=E, q_noises=Q)
  fresh_img = _sampler(dev, torch.float32, unet_w, txt_w, kl_w).ddim_p_sample_loop_img2img(ids, img, GS, **kw).clone()
  fresh_txt = _sampler(dev, torch.float32, unet_w, txt_w, kl_w).ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T).clone()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T), fresh_txt)
  assert torch.equal(s.ddim_p_sample_loop_img2img(ids, img, GS, **kw), fresh_img)
  assert s._start.item() == 4
  assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T), fresh_txt)


# ---- 5. the calls of a step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_source", ["host", "device"])
@pytest.mark.parametrize("temb_table", [True, False])
def test_deis_step_makes_the_plms_steps_calls(dev, unet_w, txt_w, kl_w, monkeypatch, temb_table, noise_source):
  img, E, Q, _, mask = T._inputs(0.)
  rng = noise_source == "device"
  calls = {}
  for name in ("plms", "deis"):
    s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, use_graph=False, temb_table=temb_table,
                 noise_source=noise_source)
    kw = {} if rng else dict(q_noises=Q)
    s.ddim_p_sample_loop_img2img(T._ids(), img, GS, strength=0.5, mask=mask, encode_noise=E, record=[], **kw)
    for masked in (False, True):
      s._index_dev.fill_(s._loop_start_index(4))
      s._set_loop_start(3)
      proxy = T._CountingLib(ops.lib)
      monkeypatch.setattr(ops, "lib", proxy)
      s._step(GS, False, None, dec_index=True, masked=masked, rng=rng)
      monkeypatch.setattr(ops, "lib", proxy._lib)
      torch.cuda.synchronize()
      calls[name, masked] = proxy.calls
  suffix = "_rng" if rng else ""
  for masked in (False, True):
    assert calls["plms", masked].count("ldm_cfg_plms_update" + suffix) == 1
    assert calls["deis", masked].count("ldm_cfg_ms_update" + suffix) == 1
    assert not any(c.startswith("ldm_cfg_plms") or c.startswith("ldm_cfg_ddim") for c in calls["deis", masked])
    swapped = ["ldm_cfg_ms_update" + suffix if c == "ldm_cfg_plms_update" + suffix else c for c in calls["plms", masked]]
    assert swapped == calls["deis", masked] and len(swapped) > 1
  print({k: len(v) for k, v in calls.items()})


# ---- 6. the defaults are untouched -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "plms"])
def test_uniform_kwarg_equals_no_kwarg(dev, name, unet_w, txt_w, kl_w):
  ids, x_T = T._ids(), _x_T()
  img, E, Q, _, mask = T._inputs(0.)
  a = _sampler(dev, torch.bfloat16, unet_w, txt_w, kl_w, sampler=name, kwarg=False)
  b_ = _sampler(dev, torch.bfloat16, unet_w, txt_w, kl_w, sampler=name, spacing="uniform")
  for t1, t2 in zip(a._device_tables()[:2] + a._device_q_tables(), b_._device_tables()[:2] + b_._device_q_tables()):
    assert torch.equal(t1, t2)
  assert torch.equal(a.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T), b_.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T))
  assert a._graph_key == b_._graph_key and a._graph_key[-1] == name
  assert not hasattr(a, "_ms_weights") or a._ms_weights is None
  kw = dict(strength=0.8, mask=mask, encode_noise=E, q_noises=Q)
  assert torch.equal(a.ddim_p_sample_loop_img2img(ids, img, GS, **kw), b_.ddim_p_sample_loop_img2img(ids, img, GS, **kw))
