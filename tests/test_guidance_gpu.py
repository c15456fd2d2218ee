"""Guidance schedules on the GPU, all through the C ABI: the scheduled update kernel against the
float64 restatement (tests/guidance_ref.py) and, bit for bit, against ldm_cfg_ms_update; what it must not read; the
U-Net on the conditional half of a resident context; whole loops against the oracle composition; the two captured
graphs; the calls of a step; device noise.

Gates.  Kernel: the error of the existing ldm_cfg_ms_update against the same restatement on the same inputs, measured
in the same run (for an unguided step: that kernel fed eps_u := eps_c, where eu + s (ec - eu) is ec exactly), floored
at 2^-23 relative, times 2 * sum_m |w_m| of the weight row in use.  U-Net: the project's gates tests/
test_img2img_gpu.py REL.  Loops: the constant-guidance DDIM loop's error against O.ddim_p_sample_loop on the same
weights, x_T and dtype, measured in the same run, times tests/test_deis_gpu.py's factor 20/3, and the project's loop
gates (1.3e-5 f32 / 8e-2 bf16).  Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deis_ref as D  # noqa: E402
import guidance_ref as G  # noqa: E402
import plms_ref as P  # noqa: E402
import test_deis_gpu as TD  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, HW, N, LDM = T.B, T.HW, T.N, T.LDM
GS = TD.GS
SHAPE = [B, HW, HW, 4]
FLOOR = 2.0 ** -23
AB = TD.AB
rel64 = TD.rel64
# (sampler, step table): the three forms the loops are checked in
FORMS = {"ddim": ("ddim", "logsnr"), "plms": ("plms", "uniform"), "deis": ("deis", "karras")}


def _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler="deis", spacing="karras", use_graph=True, noise_source="host",
             temb_table=True, **kw):
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**T.UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=T.CTX_DIM)
  ae = AutoencoderKL(**T.KL_CFG, weights=kl_w, dtype=dtype, device=dev)
  txt = TransformerModel(**T.TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
  return LatentDiffusionModelSampler(unet, ae, txt, use_graph=use_graph, verbose=False, temb_table=temb_table,
                                     sampler=sampler, noise_source=noise_source, step_spacing=spacing, **kw, **LDM)


def _schedules(steps):
  """name -> kwargs of a loop: an interval over the middle of the table, one that covers nothing, a ramp."""
  return {"middle": dict(guidance_scale=GS, guidance_interval=(int(steps[3]), int(steps[6]))),
          "nothing": dict(guidance_scale=GS, guidance_interval=(0, 0)),
          "ramp": dict(guidance_scale=[float(v) for v in np.linspace(7.5, 1.5, N)])}


def _gtab(kw, steps):
  return G.table(steps, kw["guidance_scale"], kw.get("guidance_interval"))


# ---- 1. the kernel against the float64 restatement -------------------------------------------------------
def _plms_w32():
  return G.plms_weight_table(N).astype(np.float32)


def _run_sched(dev, m, t, gtab, w32, idx, start, guided, masked, x_dtype, dec, ring=None, draws=False, eps_all=None):
  d = lambda a: a.to(dev).contiguous()
  out, px = torch.empty(B, HW, HW, 4, device=dev), torch.empty(B, HW, HW, 4, device=dev)
  xu = torch.empty(2 * B, HW, HW, 4, device=dev, dtype=x_dtype)
  ring = d(t["ring"] if ring is None else ring)
  index = torch.tensor([idx], dtype=torch.int32, device=dev)
  st = torch.tensor([start], dtype=torch.int32, device=dev)
  kw = {}
  if w32 is not None:
    kw = dict(ring=ring, start=st, weights=torch.from_numpy(np.ascontiguousarray(w32)).to(dev))
  if masked:
    kw.update(z0=d(t["z0"]), mask=d(t["mask"]), q_coef=m._device_q_tables()[2])
    if not draws:
      kw.update(q_noise=d(t["Q"]), q_index_stride=t["Q"][0].numel())
  ops.cfg_sched_update(d(t["eps_all"] if eps_all is None else eps_all), d(t["xt"]), out, m._coef_dev,
                       torch.from_numpy(np.asarray(gtab, dtype=np.float32)).to(dev), index, guided,
                       rng=TD._rng(dev) if draws else None, x_unet_out=xu, dec_index=dec, pred_x0_out=px, **kw)
  assert index.item() == (idx - 1 if dec else idx) and st.item() == start
  return out.cpu(), px.cpu(), xu.cpu(), ring.cpu()


def _run_ms_at(dev, m, t, w32, idx, start, masked, x_dtype, draws, scale):
  """test_deis_gpu._run_ms (ldm_cfg_ms_update / _rng) with the scalar `scale` in place of that module's constant."""
  keep = TD.GS
  TD.GS = scale
  try:
    return TD._run_ms(dev, m, t, w32, idx, start, masked, x_dtype, False, draws=draws)
  finally:
    TD.GS = keep


def _restated(t, tab, w64, gtab, idx, j, guided, masked):
  d = lambda a: a.double().numpy()
  eu, ec = d(t["eps_all"][:B]), d(t["eps_all"][B:])
  g = np.asarray(gtab, dtype=np.float64).copy()
  if not guided:
    g[idx] = 1.
  hist = [d(t["ring"][(idx + k) & 3]) for k in range(1, 4)]
  x, x0, e_i = G.sched_step(d(t["xt"]), None if not guided else eu, ec, hist, g, idx, j, w64[idx, j], tab["c1"],
                            tab["c2"], tab["a_prev"])
  if masked and idx >= 1:
    q = tab["qa"][idx - 1] * d(t["z0"]) + tab["qb"][idx - 1] * d(t["Q"][idx - 1])
    mk = d(t["mask"])[..., None]
    x = mk * q + (1 - mk) * x
  return x, x0, e_i


@pytest.mark.parametrize("noise", ["table", "device"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_kernel_against_float64_restatement(dev, x_dtype, masked, noise):
  m, t, tab = TD._kernel_inputs(dev)
  draws = noise == "device"
  if draws:
    t = TD._device_Q(dev, t)
  w32 = TD._kernel_weights(m)
  w64 = w32.astype(np.float64)
  gtab = np.linspace(7.5, 1.5, N).astype(np.float32)                # no entry is 1
  worst = 0.
  for idx in range(N):                                              # every index, 0 included
    for j in range(4):
      for guided in (True, False):
        # the comparator: ldm_cfg_ms_update on the same inputs (unguided: fed eps_u := eps_c) against the restatement
        gc = t if guided else dict(t, eps_all=torch.cat([t["eps_all"][B:], t["eps_all"][B:]]))
        want, want0, e_i = _restated(t, tab, w64, gtab, idx, j, guided, masked)
        cmp_ = _run_ms_at(dev, m, gc, w32, idx, idx + j, masked, x_dtype, draws, float(gtab[idx]))
        base, base0 = max(rel64(cmp_[0], want), FLOOR), max(rel64(cmp_[1], want0), FLOOR)
        dec = bool((idx + j) & 1)
        got, px, xu, ring = _run_sched(dev, m, t, gtab, w32, idx, idx + j, guided, masked, x_dtype, dec, draws=draws)
        r, r0 = rel64(got, want), rel64(px, want0)
        gate = 2 * float(np.abs(w64[idx, j, :j + 1]).sum())
        print(f"idx={idx} j={j} guided={guided} masked={masked} noise={noise}: sched {r:.3e} / x0 {r0:.3e}; "
              f"ms {base:.3e} / x0 {base0:.3e}; gate x{gate:.2f}; ratios {r / base:.3f} / {r0 / base0:.3f}")
        worst = max(worst, r / base, r0 / base0)
        assert r <= gate * base and r0 <= gate * base0, (idx, j, guided, r, r0, base, base0, gate)
        assert torch.equal(xu[:B], got.to(x_dtype)) and torch.equal(xu[B:], got.to(x_dtype))   # both halves, always
        if guided:
          assert rel64(ring[idx & 3], e_i) <= 8 * 2.0 ** -24
        else:
          assert torch.equal(ring[idx & 3], t["eps_all"][B:])       # eps_c arrives in the ring bit for bit
        for k in range(1, 4):
          assert torch.equal(ring[(idx + k) & 3], t["ring"][(idx + k) & 3])
  print("worst error in units of ldm_cfg_ms_update's:", round(worst, 3))
  # no history (weights = NULL): the DDIM step at sigma = 0 == order 0 of the table kernel, and no ring is touched
  ident = np.zeros_like(w64)
  ident[:, :, 0] = 1.
  for idx in (N - 1, 4, 0):
    for guided in (True, False):
      want, want0, _ = _restated(t, tab, ident, gtab, idx, 0, guided, masked)
      got, px, xu, ring = _run_sched(dev, m, t, gtab, None, idx, idx + 2, guided, masked, x_dtype, False, draws=draws)
      one = _run_sched(dev, m, t, gtab, ident.astype(np.float32), idx, idx, guided, masked, x_dtype, False, draws=draws)
      assert torch.equal(got, one[0]) and torch.equal(px, one[1]) and torch.equal(xu, one[2])
      assert torch.equal(ring, t["ring"])
      assert rel64(got, want) <= 4 * FLOOR and rel64(px, want0) <= 4 * FLOOR


# ---- 2. bit-exact equivalences ----------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["deis", "plms"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_constant_table_is_ldm_cfg_ms_update_bit_for_bit(dev, x_dtype, masked, table):
  m, t, _ = TD._kernel_inputs(dev)
  w32 = TD._kernel_weights(m) if table == "deis" else _plms_w32()
  for draws in (False, True):
    tt = TD._device_Q(dev, t) if draws else t
    for idx in (N - 1, 5, 1, 0):
      for j in range(4):
        ref = TD._run_ms(dev, m, tt, w32, idx, idx + j, masked, x_dtype, False, draws=draws)
        got = _run_sched(dev, m, tt, np.full(N, GS, np.float32), w32, idx, idx + j, True, masked, x_dtype, False,
                         draws=draws)
        for a, b_, what in zip(got, ref, ("x", "x0", "x_unet", "ring")):
          assert torch.equal(a, b_), (table, draws, idx, j, what)
        # unguided: eps_c arrives in the ring slot bit for bit, and the step is the table kernel's on eps_u := eps_c
        ung = _run_sched(dev, m, tt, np.full(N, GS, np.float32), w32, idx, idx + j, False, masked, x_dtype, False,
                         draws=draws)
        assert torch.equal(ung[3][idx & 3], tt["eps_all"][B:])
        cc = dict(tt, eps_all=torch.cat([tt["eps_all"][B:], tt["eps_all"][B:]]))
        ref = TD._run_ms(dev, m, cc, w32, idx, idx + j, masked, x_dtype, False, draws=draws)
        for a, b_, what in zip(ung, ref, ("x", "x0", "x_unet", "ring")):
          assert torch.equal(a, b_), (table, draws, idx, j, "unguided", what)


# ---- 3. what must not be read ------------------------------------------------------------------------------
def test_what_must_not_be_read(dev):
  m, t, _ = TD._kernel_inputs(dev)
  w32 = TD._kernel_weights(m)
  nan = float("nan")
  for draws in (False, True):
    for idx in (N - 1, 5, 0):
      for j in (0, 1, 2):
        for guided in (True, False):
          gtab = np.full(N, nan, np.float32)                        # entries other than *index
          gtab[idx] = GS
          ring = torch.full_like(t["ring"], nan)                    # slots beyond j
          for k in range(1, j + 1):
            ring[(idx + k) & 3] = t["ring"][(idx + k) & 3]
          eps = t["eps_all"].clone()
          if not guided:
            eps[:B] = nan                                           # the unconditional half
            gtab[idx] = nan                                         # ... and the scale itself
          a = _run_sched(dev, m, t, gtab, w32, idx, idx + j, guided, True, torch.float32, False, ring=ring,
                         draws=draws, eps_all=eps)
          z = _run_sched(dev, m, t, np.full(N, GS, np.float32), w32, idx, idx + j, guided, True, torch.float32, False,
                         draws=draws)
          assert all(bool(torch.isfinite(v).all()) for v in a[:3]), (draws, idx, j, guided)
          assert all(torch.equal(u, v) for u, v in zip(a[:3], z[:3])), (draws, idx, j, guided)


def test_rejects_what_it_cannot_vectorise(dev):
  from ldm_tf2_amd._lib import LdmHipError
  i = torch.zeros(1, dtype=torch.int32, device=dev)
  coef, g = torch.zeros(10, 4, device=dev), torch.ones(10, device=dev)
  x = torch.zeros(2, 3, 3, 3, device=dev)                           # n_per_sample = 27
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.cfg_sched_update(torch.zeros(4, 3, 3, 3, device=dev), x, x.clone(), coef, g, i, True)
  y = torch.zeros(2 * 16 + 1, device=dev)[1:].view(2, 4, 4, 1)      # 4-byte aligned only
  with pytest.raises(LdmHipError, match="aligned"):
    ops.cfg_sched_update(torch.zeros(4, 4, 4, 1, device=dev), y, torch.zeros(2, 4, 4, 1, device=dev), coef, g, i, False)
  z = torch.zeros(2, 4, 4, 1, device=dev)
  for name, bad in (("eps_all", dict(a=None)), ("gtab", dict(g=None))):
    args = dict(a=torch.zeros(4, 4, 4, 1, device=dev), g=g)
    args.update(bad)
    with pytest.raises(LdmHipError, match="null pointer"):
      ops.check(ops.lib.ldm_cfg_sched_update(
          args["a"].data_ptr() if args["a"] is not None else None, z.data_ptr(), None, z.data_ptr(), None, None, 0,
          coef.data_ptr(), args["g"].data_ptr() if args["g"] is not None else None, i.data_ptr(), None, None, 0, None,
          1, 0, 2, 16, None, None, None, 0, None, 1, None), "ldm_cfg_sched_update")


# ---- 4. the U-Net on the conditional half ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_unet_conditional_half(dev, dtype, unet_w, txt_w):
  from ldm_tf2_amd.unet import UNet
  unet = UNet(**T.UNET_CFG, weights=unet_w, dtype=dtype, device=dev, context_dim=T.CTX_DIM)
  context = O.text_encoder(T._ids(), txt_w, torch.float32)
  g = torch.Generator().manual_seed(12)
  x = torch.randn(B, HW, HW, 4, generator=g)
  x2 = torch.cat([x, x]).to(dev)
  t = torch.full((2 * B,), 401, dtype=torch.int32, device=dev)
  unet.set_context(context.to(dev).contiguous())
  full = unet.forward(x2, t_rows=t).clone()
  eps = torch.full((2 * B, HW, HW, 4), -77., device=dev)            # sentinel
  out = unet.forward(x2[B:], t_rows=t[B:].contiguous(), out=eps[B:], context_rows=(B, 2 * B))
  assert out.data_ptr() == eps[B:].data_ptr()
  assert bool((eps[:B] == -77.).all())                              # rows 0 .. B-1 untouched
  ref = O.unet_forward(x, np.full([B], 401, dtype=np.int32), context[B:], unet_w, torch.float32)
  T.check(eps[B:], full[B:].cpu(), dtype, "conditional half vs rows B.. of the 2B-row forward")
  T.check(eps[B:], ref, dtype, "conditional half vs the oracle U-Net")
  T.check(full[B:], ref, dtype, "2B-row forward vs the oracle U-Net")
  # the full evaluation afterwards is what it was (no buffer of one form is clobbered by the other)
  assert torch.equal(unet.forward(x2, t_rows=t), full)
  with pytest.raises(AssertionError):
    unet.forward(x2[B:], t_rows=t[B:].contiguous())                 # B rows against 2B context rows, undeclared
  with pytest.raises(AssertionError):
    unet.forward(x2[B:], t_rows=t[B:].contiguous(), context_rows=(B, 2 * B + 1))


# ---- 5. loops against the oracle composition ---------------------------------------------------------------
_CACHE = {}


def _oracle_steps(form, gtab, context, w_unet, x, start, blend=None):
  """`start + 1` scheduled steps of the specification in float32 torch on the restated tables: O.unet_forward on
  [x; x] (guided) or on x with the conditional context rows alone (unguided), then guidance_ref.sched_step."""
  name, spacing = FORMS[form]
  sched = TD._schedule(spacing, 0.)
  f = lambda key: np.asarray(sched[key]).astype(np.float32)
  c1, c2, a_prev = f("ddim_sqrt_recip_alphas_cumprod"), f("ddim_sqrt_recipm1_alphas_cumprod"), f("ddim_alphas_cumprod_prev")
  steps = sched["ddim_steps"]
  wtab = {"ddim": None, "plms": G.plms_weight_table(N).astype(np.float32),
          "deis": D.weight_table(AB, steps).astype(np.float32)}[name]
  x = torch.as_tensor(x, dtype=torch.float32)
  hist, rec = [], []
  for i in range(start, -1, -1):
    if float(gtab[i]) != 1.:
      eps_all = O.unet_forward(torch.cat([x, x], 0), np.full([2 * B], steps[i], dtype=np.int32), context, w_unet,
                               torch.float32)
      eu, ec = eps_all[:B], eps_all[B:]
    else:
      eu, ec = None, O.unet_forward(x, np.full([B], steps[i], dtype=np.int32), context[B:], w_unet, torch.float32)
    j = 0 if wtab is None else min(start - i, 3)
    w = np.array([1.], dtype=np.float32) if wtab is None else wtab[i, j]
    x, x0, e_i = G.sched_step(x, eu, ec, hist, gtab, i, j, w, c1, c2, a_prev)
    hist.insert(0, e_i)
    del hist[3:]
    assert x.dtype == torch.float32
    if blend is not None and i >= 1:
      mask, z0, Q = blend
      x = T.blend_ref(mask, T.q_sample_ref(AB, z0, [steps[i - 1]] * B, Q[i - 1]), x)
    rec.append((x.clone(), x0.clone()))
  return rec


def _oracle(form, sname, kind, w):
  key = (form, sname, kind)
  if key in _CACHE:
    return _CACHE[key]
  steps = D.step_table(AB, N, FORMS[form][1])
  gtab = _gtab(_schedules(steps)[sname], steps)
  context = O.text_encoder(T._ids(), w["cond_stage_model"], torch.float32)
  dec = lambda z: O.decoder_forward(z / LDM["scale_factor"], w["autoencoder"])
  if kind == "txt2img":
    rec = _oracle_steps(form, gtab, context, w["unet"], TD._x_T(), N - 1)
  else:
    k = kind
    img, E, Q, _, mask = T._inputs(0.)
    _, _, sample = O.diagonal_gaussian(O.encoder_forward(torch.from_numpy(img), w["autoencoder"]), E)
    z0 = np.float32(LDM["scale_factor"]) * sample
    x = T.q_sample_ref(AB, z0, [steps[k - 1]] * B, Q[k - 1])
    rec = _oracle_steps(form, gtab, context, w["unet"], x, k - 1, (mask, z0, Q))
  _CACHE[key] = dict(images=dec(rec[-1][0]), rec=rec)
  return _CACHE[key]


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_loops_against_oracle(dev, form, dtype, unet_w, txt_w, kl_w):
  name, spacing = FORMS[form]
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  base = TD._ddim_loop_error(dev, dtype, w)
  s = _sampler(dev, dtype, unet_w, txt_w, kl_w, sampler=name, spacing=spacing)
  steps = D.step_table(AB, N, spacing)
  assert s._ddim_steps.tolist() == steps.tolist()
  img, E, Q, _, mask = T._inputs(0.)
  outs = {}
  for sname, kw in _schedules(steps).items():
    gtab = _gtab(kw, steps)
    ref = _oracle(form, sname, "txt2img", w)
    got = s.ddim_p_sample_loop(T._ids(), SHAPE, x_T=TD._x_T(), **kw).clone()
    assert s._gtab.cpu().numpy().tobytes() == gtab.tobytes()
    assert set(G.guided(gtab)) <= set(s._sched_graphs)
    TD._loop_check(f"{form}/{spacing} {sname} txt2img latents", s._xt, ref["rec"][-1][0], dtype, base)
    TD._loop_check(f"{form}/{spacing} {sname} txt2img images", got, ref["images"], dtype, base)
    outs[sname] = got
    if sname == "middle":
      ref = _oracle(form, sname, 8, w)                               # img2img, half mask, under the interval
      got = s.ddim_p_sample_loop_img2img(T._ids(), img, strength=0.8, mask=mask, encode_noise=E, q_noises=Q, **kw)
      TD._loop_check(f"{form}/{spacing} {sname} inpainting latents", s._xt, ref["rec"][-1][0], dtype, base)
      TD._loop_check(f"{form}/{spacing} {sname} inpainting images", got, ref["images"], dtype, base)
      ref = _oracle(form, sname, "txt2img", w)
      freq = 5
      gi, gsm, gx = s.ddim_p_sample_loop_progressive(T._ids(), SHAPE, record_freq=freq, x_T=TD._x_T(), **kw)
      dec = lambda z: O.decoder_forward(z / LDM["scale_factor"], w["autoencoder"])
      TD._loop_check(f"{form}/{spacing} {sname} progressive images", gi, ref["images"], dtype, base)
      for r in range(N // freq):
        x, x0 = ref["rec"][N - 1 - r * freq]
        TD._loop_check(f"{form}/{spacing} {sname} progressive sample frame {r}", gsm[:, r], dec(x), dtype, base)
        TD._loop_check(f"{form}/{spacing} {sname} progressive pred_x0 frame {r}", gx[:, r], dec(x0), dtype, base)
  # the schedule matters: the three land in different places
  assert T.rel_err(outs["middle"], outs["nothing"].cpu())[0] > 10 * T.LOOP_REL[torch.float32]
  assert T.rel_err(outs["middle"], outs["ramp"].cpu())[0] > 10 * T.LOOP_REL[torch.float32]


# ---- 6. graphs and launches --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_graph_replay_is_the_eager_loop_and_tables_share_the_graphs(dev, form, unet_w, txt_w, kl_w):
  name, spacing = FORMS[form]
  ids, x_T = T._ids(), TD._x_T()
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing)
  e = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, use_graph=False)
  steps = s._ddim_steps
  sch = _schedules(steps)
  a = s.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch["middle"]).clone()
  graphs = dict(s._sched_graphs)
  assert sorted(graphs) == [False, True] and s._graph is None
  rec = []
  assert torch.equal(a, e.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch["middle"])) and not e._sched_graphs
  assert torch.equal(a, e.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, record=rec, **sch["middle"])) and len(rec) == N
  assert torch.equal(a, s.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch["middle"]))          # a second replay
  ms = s.last_form_ms_per_step()
  assert ms["guided"] > 0 and ms["unguided"] > 0 and s.last_loop_ms_per_step() > 0
  # another table: other values, another guided / unguided pattern -- the same two graph objects
  other = dict(guidance_scale=[3., 1., 1., 2., 1., 4., 4., 1., 6., 1.])
  b_ = s.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **other).clone()
  assert all(s._sched_graphs[k] is graphs[k] for k in (False, True)) and len(s._sched_graphs) == 2
  assert torch.equal(b_, e.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **other)) and not torch.equal(a, b_)
  c = s.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch["ramp"]).clone()
  assert all(s._sched_graphs[k] is graphs[k] for k in (False, True))
  assert torch.equal(c, e.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch["ramp"]))
  assert s.last_form_ms_per_step()["unguided"] is None
  # the float path next to it: its own graph, today's result, the scheduled graphs kept
  fresh = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing)
  assert torch.equal(s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T), fresh.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T))
  assert s._graph is not None and s._graph_key[0] == GS and not fresh._sched_graphs and fresh._gtab is None
  assert torch.equal(a, s.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch["middle"]))
  assert all(s._sched_graphs[k] is graphs[k] for k in (False, True))
  # skip_unguided=False: the same schedule on 2B rows every step (one U-Net plan for both forms)
  k2 = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, skip_unguided=False)
  d = k2.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch["middle"])
  r = T.rel_err(d, a.cpu())[0]
  print(f"{form}: skip_unguided False against True rel {r:.3e}, bit-equal {torch.equal(d, a)}")
  assert r <= 2 * T.LOOP_REL[torch.float32]       # (each lies within the loop gate of the one oracle composition)
  # only the forms a table uses are captured
  for sname, want in (("ramp", [True]), ("nothing", [False])):
    f = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing)
    f.ddim_p_sample_loop(ids, SHAPE, x_T=x_T, **sch[sname])
    assert sorted(f._sched_graphs) == want


def _count(monkeypatch, fn):
  proxy = T._CountingLib(ops.lib)
  monkeypatch.setattr(ops, "lib", proxy)
  try:
    fn()
  finally:
    monkeypatch.setattr(ops, "lib", proxy._lib)
  torch.cuda.synchronize()
  return proxy.calls


@pytest.mark.parametrize("noise_source", ["host", "device"])
@pytest.mark.parametrize("temb_table", [True, False])
@pytest.mark.parametrize("form", list(FORMS))
def test_the_calls_of_a_step(dev, form, temb_table, noise_source, unet_w, txt_w, kl_w, monkeypatch):
  name, spacing = FORMS[form]
  img, E, Q, _, mask = T._inputs(0.)
  rng = noise_source == "device"
  today = {"ddim": "ldm_cfg_ddim_update_masked", "plms": "ldm_cfg_plms_update", "deis": "ldm_cfg_ms_update"}[name]
  today = {"ddim": "ldm_cfg_ddim_update_rng"}.get(name, today + "_rng") if rng else today
  kw = dict(strength=0.5, mask=mask, encode_noise=E, **({} if rng else dict(q_noises=Q)))
  calls = {}
  for skip in (True, False):
    s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, use_graph=False,
                 temb_table=temb_table, noise_source=noise_source, skip_unguided=skip)
    s.ddim_p_sample_loop_img2img(T._ids(), img, GS, guidance_interval=(int(s._ddim_steps[1]), int(s._ddim_steps[2])),
                                 record=[], **kw)

    def one(fn):
      s._index_dev.fill_(s._loop_start_index(4))
      s._set_loop_start(3)
      return _count(monkeypatch, fn)
    calls[skip, "today"] = one(lambda: s._step(GS, False, None, dec_index=True, masked=True, rng=rng))
    calls[skip, "guided"] = one(lambda: s._step_sched(True, True, masked=True, rng=rng))
    calls[skip, "unguided"] = one(lambda: s._step_sched(False, True, masked=True, rng=rng))
    if skip:
      def forward_b():
        s._unet.forward(s._x2[B:], steps=s._steps_dev, index=s._index_dev, out=s._eps[B:], paired_rows=False,
                        context_rows=(B, 2 * B), **s._temb_kwargs(True))
      calls["forward_b"] = one(forward_b)
  swap = lambda cs: ["ldm_cfg_sched_update" if c == today else c for c in cs]
  for skip in (True, False):
    assert calls[skip, "today"].count(today) == 1 and "ldm_cfg_sched_update" not in calls[skip, "today"]
    assert calls[skip, "guided"] == swap(calls[skip, "today"]) and len(calls[skip, "guided"]) > 1
  assert calls[True, "unguided"] == calls["forward_b"] + ["ldm_cfg_sched_update"]
  assert calls[False, "unguided"] == swap(calls[False, "today"])     # skip_unguided=False: every step has today's launches
  print({str(k): len(v) for k, v in calls.items()})


@pytest.mark.parametrize("form", list(FORMS))
def test_a_float_scale_calls_what_the_parent_called(dev, form, unet_w, txt_w, kl_w, monkeypatch):
  """The whole eager loop with a float guidance_scale and no interval: the call sequence is N times today's step
  (U-Net evaluation on 2B rows + the sampler's own update) and no new symbol appears in it."""
  name, spacing = FORMS[form]
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, use_graph=False)
  ids, x_T = T._ids(), TD._x_T()
  s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T)
  s._index_dev.fill_(s._loop_start_index(N))
  s._set_loop_start(N - 1)
  step = _count(monkeypatch, lambda: s._step(GS, False, None, dec_index=True))
  context = s._cond_stage_model(ids)
  pre = _count(monkeypatch, lambda: s._set_context(context))
  loop = _count(monkeypatch, lambda: s.ddim_p_sample_loop(ids, SHAPE, GS, x_T=x_T))
  assert "ldm_cfg_sched_update" not in loop and s._gtab is None and not s._sched_graphs
  i = len(loop) - 1 - loop[::-1].index(step[-1])                    # the last step's last call
  assert loop[i + 1 - N * len(step):i + 1] == step * N
  head = loop[:i + 1 - N * len(step)]
  assert head[len(head) - len(pre):] == pre                         # (text encoder, then the context projections)


# ---- 7. device noise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_device_noise_under_an_interval(dev, form, unet_w, txt_w, kl_w):
  """Section 9's discipline: the fused draws against the same loop fed the table ldm_normal_fill produces, bit for
  bit (one kernel body draws or reads Q)."""
  from ldm_tf2_amd import model_runners as R
  name, spacing = FORMS[form]
  s = _sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, spacing=spacing, noise_source="device")
  img, E, _, _, mask = T._inputs(0.)
  rng = TD._rng(dev)
  q_tab = torch.stack([ops.normal_fill(torch.empty(B, HW, HW, 4, device=dev), rng, R.Q_STREAM + i) for i in range(N)])
  kw = dict(strength=0.8, mask=mask, encode_noise=E, seed=TD.SEED,
            guidance_interval=(int(s._ddim_steps[2]), int(s._ddim_steps[5])))
  fused = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, **kw).clone()
  tabled = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, q_noises=q_tab, **kw)
  assert bool(torch.isfinite(fused).all()) and torch.equal(fused, tabled)
  other = s.ddim_p_sample_loop_img2img(T._ids(), img, GS, **dict(kw, seed=TD.SEED + 1))
  assert not torch.equal(fused, other)
