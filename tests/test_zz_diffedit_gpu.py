"""DiffEdit on the GPU: the contrast accumulator as the kernels' own composition, the map and
the mask against the CPU oracle, the inversion that keeps its trajectory, the blend that reads it, the whole loop
against tests/diffedit_ref.py on the oracle's U-Net, the degenerate masks and the graph slots.

Gates.
  Accumulator: torch.equal against the float32 restatement applied to the product's own U-Net outputs.
  Map against the oracle (float32): |acc_got - acc_ref|_1 <= (1 + 1e-3) sum_r |eps_got_r - eps_ref_r|_1, which follows
    from ||a| - |b|| <= |a - b|; the right side is the existing U-Net's error measured in the same run and 1e-3 covers
    the float32 accumulation's own rounding.  Mask at tau = 1.5: equal to the oracle's on every cell outside a relative
    band of 1e-3 around the threshold, which may hold 1 % of the cells at most and none of the reference's.  Measured
    on the CPU on these inputs: the oracle's float32 and float64 maps differ by 7.4e-5 of the map's mean at most, 7.2 %
    of the cells are edited and the nearest cell is 2.3e-3 relative from the threshold.
  Loops: the error of ddim_p_sample_loop against O.ddim_p_sample_loop at the same scale, weights and dtype, measured
    in the same run, times LOOP_MARGIN (see test_whole_loop_against_reference).
Tiny models, fixtures and inputs are those of tests/test_img2img_gpu.py and tests/test_inversion_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diffedit_ref as DR  # noqa: E402
import inversion_ref as I  # noqa: E402
import test_img2img_gpu as T  # noqa: E402
import test_inversion_gpu as V  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)
from ldm_tf2_amd import ops  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

B, HW, N, LDM = T.B, T.HW, T.N, T.LDM
SHAPE = [B, HW, HW, 4]
LOOP_MARGIN = 8.
N_MAPS, K_M, TAU = 4, 5, 1.5
MAP_KW = dict(mask_strength=0.5, num_maps=N_MAPS, mask_threshold=0.5, mask_clamp_ratio=3.)
rel64 = V.rel64


def _map_noises():
  return np.random.default_rng(33).standard_normal((N_MAPS, B, HW, HW, 4)).astype(np.float32)


def _product_eps(s, dev, z0, M):
  """Each draw evaluated eagerly with the product's U-Net as the contrast step calls it (the context is the one the
  estimate left): eps [n,2B,h,w,c] on the host."""
  sa, sb, _ = s._device_q_tables()
  t = torch.full((B,), int(s._ddim_steps[K_M - 1]), dtype=torch.int32, device=dev)
  idx = torch.tensor([K_M - 1], dtype=torch.int32, device=dev)
  z = torch.from_numpy(z0).to(dev)
  out = []
  for r in range(len(M)):
    x, x2 = torch.empty(*SHAPE, device=dev), torch.empty(2 * B, HW, HW, 4, device=dev)
    ops.q_sample(z, torch.from_numpy(M[r]).to(dev), t, sa, sb, x, x_unet_out=x2)
    eps = torch.empty(2 * B, HW, HW, 4, device=dev)
    s._unet.forward(x2, steps=s._steps_dev, index=idx, out=eps, paired_rows=True, **s._temb_kwargs(False))
    out.append(eps.cpu().numpy())
  assert idx.item() == K_M - 1
  return np.stack(out)


def _restated_acc(eps):
  acc = np.zeros((B, HW, HW), np.float32)
  for e in eps:
    acc = DR.contrast_accum(acc, e[:B], e[B:])
  return acc


# ---- 1. the accumulator is the kernels' own composition --------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_accumulator_is_the_kernels_own_composition(dev, dtype, use_graph, unet_w, txt_w, kl_w):
  ids, other, z0, M = T._ids(), V._other_ids(), V._z0(), _map_noises()
  s = V._sampler(dev, dtype, unet_w, txt_w, kl_w, use_graph=use_graph)
  mask = s.diffedit_mask(ids, other, latents=z0, map_noises=M, **MAP_KW)
  acc = s._dm_acc.cpu()
  g = s._dm_graph
  assert (g is not None) == use_graph and s._graph is None and s._inv_graph is None
  assert s._dm_counters.tolist() == [K_M - 1, -1]                        # the time index stays, the draws are used up
  want = _restated_acc(_product_eps(s, dev, z0, M))
  assert torch.equal(acc, torch.from_numpy(want))
  # the mask is the mask kernel's on that accumulator: the restatement outside the band of a legal summation order
  ref, band = DR.contrast_mask(want, TAU), DR.band(want, TAU)
  assert tuple(mask.shape) == (B, HW, HW) and mask.dtype == torch.float32 and mask.data_ptr() != s._dm_out[0].data_ptr()
  assert np.array_equal(mask.cpu().numpy()[~band], ref["mask"][~band]) and band.mean() <= 0.01
  last = s.last_contrast_map()
  assert np.array_equal(last["mask"], mask.cpu().numpy()) and last["edited"].tolist() == (1 - last["mask"]).sum((1, 2)).tolist()
  assert np.array_equal(last["map"], (acc / float(4 * N_MAPS)).numpy())
  assert np.allclose(last["mean"], ref["mean64"], rtol=HW * HW * 2. ** -24, atol=0)
  assert np.array_equal(last["threshold"], (np.float32(TAU) * last["mean"]).astype(np.float32))
  # a second call replays the same captured graph and gives the same bits; the dilation grows the edit
  wide = s.diffedit_mask(ids, other, latents=z0, map_noises=M, mask_dilate=1, **MAP_KW)
  assert s._dm_graph is g and torch.equal(s._dm_acc.cpu(), acc)
  assert np.array_equal(wide.cpu().numpy() == 0, DR.dilate(mask.cpu().numpy() == 0, 1))


def test_map_noises_drawn_from_the_seed(dev, unet_w, txt_w, kl_w):
  """Without map_noises, draw r is stream MAP_STREAM + r per global sample index, on the host or on the device."""
  from ldm_tf2_amd.model_runners import MAP_STREAM, normal_latents
  ids, other, z0 = T._ids(), V._other_ids(), V._z0()
  s = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  s.diffedit_mask(ids, other, latents=z0, seed=5, first_sample_index=3, **MAP_KW)
  drawn, g = s._dm_acc.clone(), s._dm_graph
  M = np.stack([normal_latents(5, 3, B, (HW, HW, 4), stream=MAP_STREAM + r) for r in range(N_MAPS)])
  assert torch.equal(s._dm_noise.cpu(), torch.from_numpy(M).flip(0))
  s.diffedit_mask(ids, other, latents=z0, map_noises=M, **MAP_KW)
  assert torch.equal(s._dm_acc, drawn) and s._dm_graph is g
  s.diffedit_mask(ids, other, latents=z0, seed=6, **MAP_KW)
  assert not torch.equal(s._dm_acc, drawn) and s._dm_graph is g
  s._noise_source = "device"                   # (the table is then filled by ldm_normal_fill)
  s.diffedit_mask(ids, other, latents=z0, seed=5, first_sample_index=3, **MAP_KW)
  want = torch.empty(B, HW, HW, 4, device=dev)
  for r in range(N_MAPS):
    ops.normal_fill(want, s._set_rng(5, 3), MAP_STREAM + r)
    assert torch.equal(s._dm_noise[N_MAPS - 1 - r], want)
  assert s._dm_graph is g and torch.isfinite(s._dm_acc).all()


# ---- 2. against the oracle -------------------------------------------------------------------------------
def test_map_and_mask_against_the_oracle(dev, unet_w, txt_w, kl_w):
  ids, other, z0, M = T._ids(), V._other_ids(), V._z0(), _map_noises()
  s = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  mask = s.diffedit_mask(ids, other, latents=z0, map_noises=M, **MAP_KW).cpu().numpy()
  acc = s._dm_acc.cpu().numpy()
  eps_got = _product_eps(s, dev, z0, M)
  t_m = int(s._ddim_steps[K_M - 1])
  ctx = O.text_encoder(np.concatenate([ids[B:], other[B:]]), txt_w, torch.float32)
  acc_ref, eps_err = np.zeros((B, HW, HW), np.float32), 0.
  for r in range(N_MAPS):
    x = T.q_sample_ref(s._alphas_cumprod, z0, [t_m] * B, M[r])
    e = O.unet_forward(torch.cat([x, x]), np.full([2 * B], t_m, np.int32), ctx, unet_w, torch.float32).numpy()
    acc_ref = DR.contrast_accum(acc_ref, e[:B], e[B:])
    eps_err += float(np.abs(eps_got[r].astype(np.float64) - e.astype(np.float64)).sum())
  # (a)
  err = float(np.abs(acc.astype(np.float64) - acc_ref.astype(np.float64)).sum())
  print(f"|acc - ref|_1 = {err:.4e}; sum_r |eps - ref|_1 = {eps_err:.4e}; ratio {err / eps_err:.3f}")
  assert err <= (1 + 1e-3) * eps_err
  # (b)
  ref = DR.contrast_mask(acc_ref, TAU)
  thr, thr_got = ref["thr64"][:, None, None], s.last_contrast_map()["threshold"].astype(np.float64)[:, None, None]
  near_ref = np.abs(acc_ref - thr) <= 1e-3 * thr
  near = near_ref | (np.abs(acc - thr_got) <= 1e-3 * thr_got)
  edited = (ref["mask"] == 0).mean()
  nearest = float((np.abs(acc_ref - thr) / thr).min())
  print(f"edited {100 * edited:.2f} % of the cells; nearest cell {nearest:.3e} relative from the threshold; "
        f"the band excludes {near.sum()} cells")
  assert near_ref.sum() == 0 and near.mean() <= 0.01
  assert np.array_equal(mask[~near], ref["mask"][~near])
  assert 0.02 < edited < 0.5                                             # (a mask with both kinds of cells)


# ---- 3. the trajectory -----------------------------------------------------------------------------------
@pytest.mark.parametrize("temb_table", [True, False])
def test_trajectory_rows_are_the_inversion_steps_outputs(dev, unet_w, txt_w, kl_w, temb_table):
  ids, z0 = T._ids(), V._z0()
  s = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=True, temb_table=temb_table)
  e = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False, temb_table=temb_table)
  for strength, k in ((0.7, 7), (1.0, N), (0.3, 3)):
    rec = []
    want = e.ddim_invert_loop(ids, latents=z0, strength=strength, record=rec)          # as today, no trajectory
    got = s.ddim_invert_loop(ids, latents=z0, strength=strength, trajectory=True)
    traj = s.last_trajectory()
    assert tuple(traj.shape) == (k, B, HW, HW, 4) and traj.data_ptr() != s._traj.data_ptr()
    assert all(torch.equal(traj[j], rec[j]) for j in range(k)) and torch.equal(got, want)
    assert s._index_dev.item() == (N if temb_table else N - 1) - k
    rec2 = []
    e.ddim_invert_loop(ids, latents=z0, strength=strength, trajectory=True, record=rec2)   # eager, with the store
    assert torch.equal(e.last_trajectory(), traj) and all(torch.equal(a, b) for a, b in zip(rec, rec2))
  g = s._invt_graph
  assert g is not None and s._inv_graph is None and s._invt_graph_key[-1] == "trajectory"   # one capture, any depth
  # without the keyword: the graph slot and the key of today, beside the other
  a = s.ddim_invert_loop(ids, latents=z0)
  assert s._inv_graph is not None and s._invt_graph is g
  assert s._inv_graph_key == ("invert", None, s._ctx_shape, s._step_spacing)
  assert torch.equal(a, s.ddim_invert_loop(ids, latents=z0, trajectory=True)) and s._invt_graph is g


@pytest.mark.parametrize("temb_table", [True, False])
def test_trajectory_adds_one_launch_and_none_without_the_keyword(dev, unet_w, txt_w, kl_w, monkeypatch, temb_table):
  s = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False, temb_table=temb_table)
  ids, z0, k = T._ids(), V._z0(), 3
  s.ddim_invert_loop(ids, latents=z0, strength=0.3, trajectory=True, record=[])     # allocates everything
  calls = {}
  for what in ("step", "plain", "trajectory"):
    proxy = T._CountingLib(ops.lib)
    if what == "step":                         # one inversion step as tests/test_inversion_gpu.py counts it
      s._index_dev.fill_(s._invert_counter_start())
      monkeypatch.setattr(ops, "lib", proxy)
      s._step_invert(1., True)
    else:
      monkeypatch.setattr(ops, "lib", proxy)
      s.ddim_invert_loop(ids, latents=z0, strength=0.3, trajectory=what == "trajectory", record=[])
    monkeypatch.setattr(ops, "lib", proxy._lib)
    torch.cuda.synchronize()
    calls[what] = proxy.calls
  step = calls["step"]
  assert step[-1] == "ldm_cfg_ddim_invert_update" and "ldm_store_row" not in step
  tail = lambda cs, n: cs[len(cs) - n:]
  assert tail(calls["plain"], k * len(step)) == step * k                              # the loop's steps are today's
  assert tail(calls["trajectory"], k * (len(step) + 1)) == (step + ["ldm_store_row"]) * k
  assert calls["trajectory"][:len(calls["trajectory"]) - k * (len(step) + 1)] == calls["plain"][:len(calls["plain"]) - k * len(step)]


# ---- 4. the blend ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "plms"])
def test_blend_pins_the_kept_cells_to_the_trajectory(dev, name, unet_w, txt_w, kl_w):
  ids, other = T._ids(), V._other_ids()
  img, E, _, _, mask = T._inputs(0.)                                     # keep the left half
  k = 5
  e = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, use_graph=False)
  rec = []
  out = e.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask, encode_noise=E, record=rec)
  assert tuple(out.shape) == (B, 8 * HW, 8 * HW, 3) and len(rec) == k and e._dm_graph is None and e._dm_last is None
  traj = e.last_trajectory()
  assert traj.shape[0] == k
  keep = torch.from_numpy(mask).to(dev).bool()[..., None].expand(*SHAPE)
  for s_i, x in enumerate(rec):
    i = k - 1 - s_i                            # the DDIM index of the step that wrote x
    if i >= 1:
      assert torch.equal(x[keep], traj[i - 1][keep]), i
      assert not (x[~keep] == traj[i - 1][~keep]).any(), i
    else:                                      # index 0: decoded as it is
      assert not (x[keep] == traj[0][keep]).all() and torch.equal(x, e._xt)
  # graph replay: the same latents, a slot of its own, no other graph touched
  s = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name, use_graph=True)
  s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask, encode_noise=E)
  assert torch.equal(s._xt, rec[-1]) and s._de_graph is not None and s._graph is None and s._invt_graph is not None
  assert s._de_graph_key[-1] == ("traj_blend",) and not s._blend_traj
  # a one-mask [h,w] is tiled over the batch
  s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask[0], encode_noise=E)
  assert torch.equal(s._xt, rec[-1])
  with pytest.raises(ValueError, match="latent resolution"):
    s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask[:, :4], encode_noise=E)


def test_eta_noise_comes_from_the_table_for_both_noise_sources(dev, unet_w, txt_w, kl_w):
  """eta > 0: the loop always takes the table-reading update, whose eta noise is `noises` or the loop's own table (on
  the device: ldm_normal_fill's streams ETA_STREAM + i); the blend still pins the kept cells."""
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import ETA_STREAM, LatentDiffusionModelSampler, normal_latents
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  ids, other, k = T._ids(), V._other_ids(), 5
  img, E, _, noises, mask = T._inputs(1.)
  keep = torch.from_numpy(mask).to(dev).bool()[..., None].expand(*SHAPE)
  for source in ("host", "device"):
    s = LatentDiffusionModelSampler(UNet(**T.UNET_CFG, weights=unet_w, device=dev, context_dim=T.CTX_DIM),
                                    AutoencoderKL(**T.KL_CFG, weights=kl_w, device=dev),
                                    TransformerModel(**T.TXT_CFG, weights=txt_w, device=dev), verbose=False,
                                    noise_source=source, **dict(LDM, eta=1.))
    rec = []
    s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask, encode_noise=E, noises=noises,
                                  record=rec)
    traj = s.last_trajectory()
    assert all(torch.equal(rec[i][keep], traj[k - 2 - i][keep]) for i in range(k - 1))
    assert torch.equal(s._noise_buf.cpu(), torch.from_numpy(noises))
    given = s._xt.clone()
    s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask, encode_noise=E, noises=noises)
    assert torch.equal(s._xt, given) and s._de_graph is not None                   # graph replay, the same bits
    s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask, encode_noise=E, seed=3)
    assert torch.isfinite(s._xt).all() and not torch.equal(s._xt, given)
    want = torch.empty(*SHAPE, device=dev)
    for i in range(N):                         # the loop's own table
      if source == "device":
        ops.normal_fill(want, s._set_rng(3, 0), ETA_STREAM + i)
      else:
        want.copy_(torch.from_numpy(normal_latents(3 + 1 + i, 0, B, (HW, HW, 4))))
      assert torch.equal(s._noise_buf[i], want), (source, i)


# ---- 5. the whole loop against the reference composition -------------------------------------------------
@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_whole_loop_against_reference(dev, dtype, unet_w, txt_w, kl_w):
  """DR.diffedit_loop in float32 on the oracle's U-Net, given the device's own mask and z0 (a threshold flip cannot
  enter).  Gate as test_inversion_gpu.test_edit_loop: LOOP_MARGIN * max(base_1, base_5).
  Margin 8: between a float32 and a float64 run of the restatements on the oracle's U-Net at these shapes (on the CPU)
  this composition drifts 2.06e-6, the sampling loops 3.64e-6 (g = 5) and 6.29e-7 (g = 1): 0.56 times the larger, the
  one the gate takes, and 3.27 times the smaller.  8 covers both, so it stays."""
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  ids, other = T._ids(), V._other_ids()
  img, E, _, _, _ = T._inputs(0.)
  k = 5
  base, base5 = V._sampling_error(dev, dtype, w, 1.), V._sampling_error(dev, dtype, w, 5.)
  s = V._sampler(dev, dtype, unet_w, txt_w, kl_w)
  out = s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, encode_noise=E, map_noises=_map_noises(),
                                      **MAP_KW)
  assert tuple(out.shape) == (B, 8 * HW, 8 * HW, 3) and s._index_dev.item() == 0
  z0, mask = s._z0_buf.cpu().numpy(), s._mask_buf.cpu().numpy()
  assert np.array_equal(mask, s.last_contrast_map()["mask"]) and 0 < (mask == 0).sum() < mask.size
  tab = I.make_tables(s._alphas_cumprod, s._ddim_steps, np.float32)
  ref, traj = DR.diffedit_loop(V._eps_fn(w, ids, 1.), V._eps_fn(w, other, 5.), z0, mask, 1., 5., k, s._ddim_steps, tab,
                               dtype=np.float32)
  r, gate = rel64(s._xt, ref), LOOP_MARGIN * max(base, base5)
  rt = rel64(s.last_trajectory(), traj)
  print(f"diffedit [{dtype}]: {r:.3e}; trajectory {rt:.3e}; sampling loops {base:.3e} (g = 1), {base5:.3e} (g = 5); "
        f"gate {gate:.3e}")
  assert r <= gate, (r, gate)


# ---- 6. degenerate masks ---------------------------------------------------------------------------------
def test_all_zeros_mask_is_the_edit_loop_bit_for_bit(dev, unet_w, txt_w, kl_w):
  ids, other = T._ids(), V._other_ids()
  img, E, _, _, _ = T._inputs(0.)
  for name in ("ddim", "plms"):
    s = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w, sampler=name)
    img_e = s.ddim_p_sample_loop_edit(ids, other, img, guidance_scale=5., strength=0.5, encode_noise=E)
    want = s._xt.clone()
    img_d = s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=np.zeros((HW, HW), np.float32),
                                          encode_noise=E)
    assert torch.equal(s._xt, want) and torch.equal(img_d, img_e)


@pytest.mark.parametrize("dtype", T.DT, ids=["f32", "bf16"])
def test_all_ones_mask_reconstructs(dev, dtype, unet_w, txt_w, kl_w):
  """Both scales 1, the same ids, every cell kept: each step but the last lands on the trajectory, the last is one
  sampling step from traj[0].  That is a reconstruction of the image, and a much closer one than
  ddim_p_sample_loop_edit's, whose k free steps collect the inversion's truncation error: in float64 on the oracle's
  U-Net (CPU, these inputs) the all-ones loop ends 6.26e-4 relative from z0 and the edit loop 0.311, 0.299 from one
  another.  So the two are NOT equal within a rounding gate, whatever the precision, and the check is the one
  test_edit_loop makes for its reconstruction, against this loop's own reference: the latents against
  DR.diffedit_loop with the all-ones mask within LOOP_MARGIN * base_1 (float32 against float64 that reference drifts
  7.0e-8, the g = 1 sampling loop 6.29e-7), and no farther from z0 than the edit loop's reconstruction."""
  w = dict(unet=unet_w, autoencoder=kl_w, cond_stage_model=txt_w)
  ids, k = T._ids(), 5
  img, E, _, _, _ = T._inputs(0.)
  base = V._sampling_error(dev, dtype, w, 1.)
  s = V._sampler(dev, dtype, unet_w, txt_w, kl_w, use_graph=False)
  s.ddim_p_sample_loop_edit(ids, ids, img, guidance_scale=1., strength=0.5, encode_noise=E)
  edit = s._xt.clone()
  ones = np.ones((B, HW, HW), np.float32)
  rec = []
  s.ddim_p_sample_loop_diffedit(ids, ids, img, 1., strength=0.5, mask=ones, encode_noise=E, record=rec)
  traj = s.last_trajectory()
  assert all(torch.equal(rec[i], traj[k - 2 - i]) for i in range(k - 1))                 # on the trajectory, all of x
  z0 = s._z0_buf.cpu().numpy()
  tab = I.make_tables(s._alphas_cumprod, s._ddim_steps, np.float32)
  fn = V._eps_fn(w, ids, 1.)
  ref, _ = DR.diffedit_loop(fn, fn, z0, ones, 1., 1., k, s._ddim_steps, tab, dtype=np.float32)
  r, gate = rel64(s._xt, ref), LOOP_MARGIN * base
  d_got, d_ref, d_edit = rel64(s._xt, z0), rel64(ref, z0), rel64(edit, z0)
  print(f"all-ones mask [{dtype}]: against the reference {r:.3e} (gate {gate:.3e}); distance to z0 {d_got:.4e}, "
        f"reference {d_ref:.4e}, the edit loop's {d_edit:.4e}; against the edit loop's latents {rel64(s._xt, edit):.3e}")
  assert r <= gate, (r, gate)
  assert d_got <= d_edit


# ---- 7. the graph slots ----------------------------------------------------------------------------------
def test_graph_slots_live_side_by_side(dev, unet_w, txt_w, kl_w):
  """The new slots beside the existing ones.  (The masked img2img loop and the plain sampling loop share the slot
  _graph under different keys, today as before, so each is alternated with the inversion and the new loop in turn.)"""
  ids, other, M = T._ids(), V._other_ids(), _map_noises()
  img, E, Q, _, mask = T._inputs(0.)
  s = V._sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  run = dict(
      inpaint=lambda: s.ddim_p_sample_loop_img2img(ids, img, 5., strength=0.5, mask=mask, encode_noise=E, q_noises=Q),
      sample=lambda: s.ddim_p_sample_loop(ids, SHAPE, 5., x_T=V._x_T()),
      invert=lambda: s.ddim_invert_loop(ids, init_images=img, encode_noise=E),
      diffedit=lambda: s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, encode_noise=E, map_noises=M,
                                                     **MAP_KW))
  slots = ("_graph", "_inv_graph", "_dm_graph", "_invt_graph", "_de_graph")
  for legacy in ("inpaint", "sample"):
    names = (legacy, "invert", "diffedit")
    first = {}
    for name in names:                         # (the first calls allocate owned buffers, which drops graphs)
      run[name]()
      first[name] = s._xt.clone()
    for name in names:
      run[name]()
    graphs = {n: getattr(s, n) for n in slots}
    assert all(g is not None for g in graphs.values()) and len({id(g) for g in graphs.values()}) == len(slots)
    assert s._graph_key[3] == (legacy == "inpaint") and s._de_graph_key[3] and s._graph_key != s._de_graph_key
    for _ in range(2):
      for name in names:
        run[name]()
        assert torch.equal(s._xt, first[name]), name
        assert all(getattr(s, n) is g for n, g in graphs.items()), name
  # the masked img2img loop never replays the trajectory's step, nor the other way round
  run["inpaint"]()
  inpaint, g7 = s._xt.clone(), s._graph
  de = s._de_graph
  s.ddim_p_sample_loop_diffedit(ids, other, img, 5., strength=0.5, mask=mask, encode_noise=E)
  assert not torch.equal(s._xt, inpaint) and s._graph is g7 and s._de_graph is de
  run["inpaint"]()
  assert torch.equal(s._xt, inpaint) and s._graph is g7 and s._de_graph is de
