"""Round-4 launch forms against the CPU oracle and against the forms they replace (all through the C ABI).

  * launch-plan robustness: a table entry whose tile cannot run a launch (persistent tile, epilogue not
    instantiated / deferred split-K product) falls back to the cost model instead of raising or recursing.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ldm_tf2_amd import ops, weights as Wt  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402

from test_models_gpu import CTX_DIM, KL_CFG, LDM, TXT_CFG, UNET_CFG, check  # noqa: E402

DT = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def unet_w():
  return Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **UNET_CFG), seed=2, mode="random", scope="unet")


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("mc", [64, 320], ids=["per-layer", "st_block"])
def test_paired_rows_share_the_prefix(dev, dtype, mc):
  """forward(paired_rows=True): rows r and r + R/2 carry the same x and t (the DDIM loop's concat([xt, xt]),
  model_runners.py:449-452) and differ in their context only, so the first ResBlock and the first transformer
  block up to its self-attention run ONCE on R/2 rows.  Same result as the plain evaluation up to summation order
  (the half-row launches may take other tiles), both inside the U-Net gate against the oracle.  mc = 320 takes
  ldm_st_block's in_rows form (bf16), mc = 64 the per-layer path that duplicates the rows after the self-attention."""
  from ldm_tf2_amd.unet import UNet
  cfg = dict(model_channels=mc, out_channels=4, num_blocks=1, channel_mult=(1, 2), num_heads=8) if mc == 320 else UNET_CFG
  w = Wt.init_weights(Wt.unet_manifest(context_dim=CTX_DIM, **cfg), seed=4, mode="random", scope="unet")
  R, hw = 4, 16
  g = np.random.default_rng(5)
  xh = g.standard_normal((R // 2, hw, hw, 4)).astype(np.float32)
  x = np.concatenate([xh, xh], 0)
  ctx = g.standard_normal((R, 77, CTX_DIM)).astype(np.float32)
  t = np.full((R,), 481, dtype=np.int32)
  xd, cd, td = (torch.from_numpy(a).to(dev) for a in (x, ctx, t))
  kw = dict(ffn_min_rows=1, fold_min_rows=1) if mc == 320 else {}
  u = UNet(**cfg, context_dim=CTX_DIM, weights=w, dtype=dtype, device=dev, **kw)
  u.set_context(cd)
  calls = {"st_block": 0, "in_rows": []}
  orig = ops.st_block

  def counted(att, *a, **k):
    calls["st_block"] += 1
    calls["in_rows"].append((att.shape[0], a[6].shape[0]))      # rows of att, samples of ctx_k
    return orig(att, *a, **k)

  ops.st_block = counted
  try:
    plain = u.forward(xd, t_rows=td, shared_t=True).clone()
    paired = u.forward(xd, t_rows=td, shared_t=True, paired_rows=True).clone()
  finally:
    ops.st_block = orig
  torch.cuda.synchronize()
  if mc == 320 and dtype == torch.bfloat16:
    assert (R // 2, R) in calls["in_rows"], f"ldm_st_block never ran in its in_rows form: {calls}"
  with torch.no_grad():
    want = O.unet_forward(x, t, ctx, w)
  check(plain, want, dtype, f"unet mc={mc} plain")
  check(paired, want, dtype, f"unet mc={mc} paired rows")
  r = ((paired.double() - plain.double()).norm() / plain.double().norm()).item()
  print(f"paired vs plain [{dtype}] mc={mc}: rel {r:.3e}")
  assert r < (2e-5 if dtype == torch.float32 else 2e-2)
  # rows that do NOT pair up must not be declared so: the flag is a promise, not a detection -- but an unpaired
  # evaluation through the default path is untouched by it
  assert torch.equal(u.forward(xd, t_rows=td, shared_t=True), plain)


def test_select_row_and_pre_decrement(dev):
  """ldm_select_row: out = table[*index] bit for bit; pre_decrement moves the device-side counter first; an index
  outside the table reads its nearest row instead of memory behind it."""
  g = torch.Generator().manual_seed(1)
  table = torch.randn(7, 20160, generator=g).to(dev)
  idx = torch.tensor([5], dtype=torch.int32, device=dev)
  out = torch.empty(1, 20160, device=dev)
  ops.select_row(table, idx, out)
  assert torch.equal(out[0], table[5]) and int(idx.item()) == 5
  ops.select_row(table, idx, out, pre_decrement=True)
  assert torch.equal(out[0], table[4]) and int(idx.item()) == 4
  idx.fill_(7)
  ops.select_row(table, idx, out)
  assert torch.equal(out[0], table[6])
  wide = torch.randn(3, 64, generator=g).to(dev)[:, :32]          # a strided table
  idx.fill_(2)
  o2 = torch.empty(32, device=dev)
  ops.select_row(wide, idx, o2)
  assert torch.equal(o2, wide[2])


def test_temb_table_loop_equals_the_per_step_launches(dev, unet_w):
  """The DDIM loop with the steps' temb projections taken from the per-loop table (one row-select per step, which
  also moves the loop counter) == the loop that runs the timestep MLP and a decrement launch in every step: same
  bits (float32 and bf16; graph replay and eager), and the table's rows are the per-step values."""
  from ldm_tf2_amd.autoencoder import AutoencoderKL
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  from ldm_tf2_amd.transformer import TransformerModel
  from ldm_tf2_amd.unet import UNet
  txt_w = Wt.init_weights(Wt.transformer_manifest(**TXT_CFG), seed=2, mode="random", scope="cond_stage_model")
  kl_w = Wt.init_weights(Wt.decoder_manifest(**KL_CFG), seed=2, mode="random", scope="autoencoder")
  B = 2
  g = np.random.default_rng(9)
  ids = np.concatenate([np.tile(np.array([[101, 102] + [0] * 75]), (B, 1)), g.integers(0, 1000, size=(B, 77))], 0).astype(np.int64)
  x_T = g.standard_normal((B, 16, 16, 4)).astype(np.float32)
  ldm = dict(LDM, eta=1.0)
  noises = g.standard_normal((ldm["num_ddim_steps"], B, 16, 16, 4)).astype(np.float32)
  for dtype in DT:
    res = {}
    for table in (True, False):
      for graph in (True, False):
        unet = UNet(**UNET_CFG, context_dim=CTX_DIM, weights=unet_w, dtype=dtype, device=dev)
        txt = TransformerModel(**TXT_CFG, weights=txt_w, dtype=dtype, device=dev)
        ae = AutoencoderKL(**KL_CFG, weights=kl_w, dtype=dtype, device=dev)
        s = LatentDiffusionModelSampler(unet, ae, txt, verbose=False, use_graph=graph, temb_table=table, **ldm)
        img = s.ddim_p_sample_loop(ids, [B, 16, 16, 4], guidance_scale=5., x_T=x_T, noises=noises)
        torch.cuda.synchronize()
        assert (s._temb_tbl is not None) == table
        assert int(s._index_dev.item()) == (0 if table else -1)
        res[(table, graph)] = (img.clone(), s._xt.clone())
        if table and graph:
          # a second loop on the same sampler (same graph) reproduces the first
          img2 = s.ddim_p_sample_loop(ids, [B, 16, 16, 4], guidance_scale=5., x_T=x_T, noises=noises)
          assert torch.equal(img2, img)
          # row i of the table = what one evaluation computes for t = steps[i]
          t_i = s._steps_dev[3:4].clone()
          assert torch.equal(unet._temb(1, t_i, None, None, True)[0], s._temb_tbl[3])
    ref = res[(False, False)]
    for k, v in res.items():
      assert torch.equal(v[1], ref[1]) and torch.equal(v[0], ref[0]), f"{dtype} temb_table={k[0]} graph={k[1]} differs"


@pytest.mark.parametrize("R,T,C,H,S", [(4, 256, 640, 8, 80), (4, 64, 1280, 8, 160), (2, 128, 640, 8, 80), (3, 96, 320, 8, 40),
                                       (32, 1024, 320, 8, 40)])    # 128 panels x 2 workgroups: ranges straddle n_split
def test_merged_qkv_launch_equals_the_two_launches(dev, R, T, C, H, S):
  """LayerNorm -> q | k (row-major) and -> V^T (transposed per sample) as ONE launch of the persistent kernel
  (ldm_gemm out2 with n_split = 2 heads Sp and ln_cs; unet.py:270-276, :309): the same bits as the two launches it
  replaces (every output is the same sequence of MFMAs over k), and the oracle's LayerNorm + Dense within the bf16
  gate.  The 40-wide heads are padded to 48 (n_split = 768: six 128-column n-tiles); the last case is the 32x32 level of
  BASELINE configs[2], where a workgroup's range of n-tiles straddles n_split (both instances of the body in one
  workgroup)."""
  from ldm_tf2_amd import layout as L
  BF = torch.bfloat16
  g = torch.Generator().manual_seed(11)
  sp = L.padded_head(S)
  hs = H * sp
  M = R * T
  x = (torch.randn(M, C, generator=g) * 1.5 + 0.5 * torch.randn(M, 1, generator=g)).to(BF)
  gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
  kq, kk, kv = (torch.randn(C, H, S, generator=g).numpy() * C ** -0.5 for _ in range(3))
  f32, cpu = torch.float32, "cpu"
  wq, wk, wv = (L.split_kernel(k_, sp, f32, cpu) for k_ in (kq, kk, kv))
  qk_w, qk_cs, qk_b = L.ln_fold(torch.cat([wq, wk], 0), gamma.numpy(), beta.numpy(), None, BF, dev)
  v_w, v_cs, v_b = L.ln_fold(wv, gamma.numpy(), beta.numpy(), None, BF, dev)
  a_w, a_cs, a_b = L.ln_fold(torch.cat([wq, wk, wv], 0), gamma.numpy(), beta.numpy(), None, BF, dev)
  xd = x.to(dev).view(R, T, C)
  tp = (T + 7) // 8 * 8
  qk0 = torch.empty(R, T, 2 * hs, dtype=BF, device=dev)
  vt0 = torch.zeros(R, hs, tp, dtype=BF, device=dev)
  ops.linear(xd, qk_w, qk0, bias=qk_b, ln_fold=(qk_cs, 1e-5))
  ops.linear_t(xd, v_w, vt0, bias=v_b, ln_fold=(v_cs, 1e-5))
  qk1 = torch.full((R, T, 2 * hs), float("nan"), dtype=BF, device=dev)
  vt1 = torch.zeros(R, hs, tp, dtype=BF, device=dev)
  ops.linear(xd, a_w, qk1, bias=a_b, ln_fold=(a_cs, 1e-5), out2=vt1)
  torch.cuda.synchronize()
  # (bit for bit at 25 M outputs too: round 4 first saw 10 outputs on the other side of a bf16 rounding tie here -- the
  # LayerNorm fold's variance was contracted differently in the inlined copies of the epilogue, so a row's rstd
  # depended on whether its n-tile was a workgroup's last; the contraction is pinned in gemm3_kernel.h now)
  assert torch.equal(qk1, qk0) and torch.equal(vt1, vt0)
  ln = O.layer_norm(x.float(), gamma, beta, eps=1e-5)
  want_qk = ln @ torch.cat([wq, wk], 0).t()
  want_v = (ln @ wv.t()).view(R, T, hs).permute(0, 2, 1)
  r1 = ((qk1.float().cpu().view(M, -1) - want_qk).norm() / want_qk.norm()).item()
  r2 = ((vt1.float().cpu()[:, :, :T] - want_v).norm() / want_v.norm()).item()
  print(f"merged q|k|V^T R={R} T={T} C={C}: rel {r1:.3e} / {r2:.3e}")
  assert r1 < 6e-3 and r2 < 6e-3


@pytest.mark.parametrize("case", ["shift32", "shift64", "outliers"])
@pytest.mark.parametrize("M,K,N", [(1024, 320, 768), (512, 1280, 1280)])
def test_layernorm_fold_on_rows_with_a_large_mean(dev, case, M, K, N):
  """the LayerNorm fold takes its row statistics in ONE pass (f32 sums of x and x^2, var = E[x^2] -
  mean^2) and subtracts mean * colsum from the accumulated product; rows whose |mean| is far above their spread
  are the hard case.  bf16 rows cannot carry more than 2^8 of mean / spread (the values' own rounding step), so
  the cases are: a common offset of 32 and 64 sigma, and 1 % outlier channels at 60 sigma (what trained
  checkpoints' residual streams show).  Gate: no worse than 1.5x the two-launch form (two-pass LayerNorm kernel ->
  bf16 rows -> GEMM) on the same bf16 inputs, against the float64 oracle of those inputs."""
  from ldm_tf2_amd import layout as L
  BF = torch.bfloat16
  g = torch.Generator().manual_seed(21)
  x = torch.randn(M, K, generator=g)
  if case == "outliers":
    idx = torch.randperm(K, generator=g)[:max(1, K // 100)]
    x[:, idx] += 60.0 * torch.sign(torch.randn(len(idx), generator=g))
  else:
    x = x + float(case[5:]) * torch.sign(torch.randn(M, 1, generator=g))
  x = x.to(BF)
  gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
  w = torch.randn(N, K, generator=g) * K ** -0.5
  bias = torch.randn(N, generator=g)
  xd = x.double()
  mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
  ref = ((xd - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()) @ w.double().t() + bias.double()
  wq, cs, bb = L.ln_fold(w, gamma.numpy(), beta.numpy(), bias.numpy(), BF, dev)
  out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
  ops.linear(x.to(dev), wq, out, bias=bb, ln_fold=(cs, 1e-5))
  ln = torch.empty(M, K, dtype=BF, device=dev)
  ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), ln, 1e-5)
  out2 = torch.empty(M, N, dtype=BF, device=dev)
  ops.linear(ln, w.to(BF).to(dev), out2, bias=bias.to(dev))
  rel = lambda a: ((a.double().cpu() - ref).norm() / ref.norm()).item()
  r, r2 = rel(out), rel(out2)
  print(f"LN fold, {case}, M={M} K={K} N={N}: rel {r:.3e} (LayerNorm kernel + GEMM: {r2:.3e})")
  assert torch.isfinite(out.float()).all()
  assert r <= max(4e-3, 1.5 * r2)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,Cin,Cin2,Cout,tile,split", [
    (2, 16, 128, 192, 320, 0, 0),        # cost model
    (3, 8, 256, 128, 640, 9, 2),         # ping-pong tile, split-K: the shortcut's K-tiles fall into the last slab
    (2, 32, 64, 64, 320, 10, 1),
    (1, 16, 320, 960, 320, 2, 3),        # an output block's shape: the shortcut is wider than the convolution
    (5, 4, 128, 256, 1280, 18, 4),       # 4x4 level, deep-ring small tile
])
def test_conv3x3_with_the_shortcut_as_a_second_operand(dev, dtype, B, H, Cin, Cin2, Cout, tile, split):
  """ldm_gemm a2: out = conv3x3(x) W[:, :9 Cin]^T + x2 W[:, 9 Cin:]^T + bias (+ residual ...) -- the ResidualBlock's
  1x1 shortcut over the block input (unet.py:379-380, :393-397) accumulated inside its second convolution's K loop.
  Against the oracle's conv2d + dense; plain, with a deferred split-K reduce completed by the GroupNorm that
  follows (ldm_groupnorm_splitk), and against the two-launch form on the same operands."""
  from ldm_tf2_amd import layout as L
  if dtype == torch.float32 and tile in (9, 10):
    pytest.skip("bf16-only tile")
  g = torch.Generator().manual_seed(31)
  x = torch.randn(B, H, H, Cin, generator=g).to(dtype)
  x2 = torch.randn(B, H, H, Cin2, generator=g).to(dtype)
  k = torch.randn(3, 3, Cin, Cout, generator=g) * (9 * Cin) ** -0.5
  ks = torch.randn(Cin2, Cout, generator=g) * Cin2 ** -0.5
  b1, b2 = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
  want = O.conv2d(x.float(), k, b1) + O.dense(x2.float(), ks, b2)
  wt = L.conv_shortcut_kernel(k.numpy(), ks.numpy(), dtype, dev)
  bias = (b1 + b2).to(dev)
  xd, x2d = x.to(dev), x2.to(dev)
  out = torch.full((B, H, H, Cout), float("nan"), dtype=dtype, device=dev)
  ops.conv3x3(xd, wt, out, bias=bias, x2=x2d, tile=tile, split_k=split)
  gate = 2e-5 if dtype == torch.float32 else 6e-3
  r = ((out.float().cpu().double() - want.double()).norm() / want.double().norm()).item()
  # two-launch form: shortcut GEMM, then the convolution with it as the residual
  res = torch.empty_like(out)
  ops.linear(x2d, L.dense_kernel(ks.numpy(), dtype, dev), res, bias=b2.to(dev))
  out2 = torch.empty_like(out)
  ops.conv3x3(xd, L.conv_kernel(k.numpy(), dtype, dev), out2, bias=b1.to(dev), residual=res)
  r2 = ((out2.float().cpu().double() - want.double()).norm() / want.double().norm()).item()
  print(f"conv + shortcut as one product [{dtype}] B={B} H={H} {Cin}+{Cin2}->{Cout} tile {tile} split {split}: rel {r:.3e} (two launches {r2:.3e})")
  assert r < gate and r <= r2 * 1.2 + 1e-6          # (no rounding of the shortcut's output to the storage type)
  # a channel slice of a wider buffer as the second operand (the U-Net's concat buffers)
  wide = torch.randn(B, H, H, Cin2 + 64, generator=g).to(dtype).to(dev)
  wide[..., 32:32 + Cin2] = x2d
  out3 = torch.empty_like(out)
  ops.conv3x3(xd, wt, out3, bias=bias, x2=wide[..., 32:32 + Cin2], tile=tile, split_k=split)
  assert torch.equal(out3, out)
  # deferred reduce + GroupNorm in one launch
  gamma, beta = (1.0 + 0.3 * torch.randn(Cout, generator=g)).to(dev), (0.2 * torch.randn(Cout, generator=g)).to(dev)
  y = torch.empty_like(out)
  pend = ops.conv3x3(xd, wt, y, bias=bias, x2=x2d, tile=tile, split_k=split, defer_reduce=True)
  gn = torch.empty_like(out)
  ops.groupnorm(y, gamma, beta, gn, 1e-5, silu=True, pending=pend)
  gn0 = torch.empty_like(out)
  ops.groupnorm(out, gamma, beta, gn0, 1e-5, silu=True)
  assert torch.equal(y, out) and torch.equal(gn, gn0)


def test_conv3x3_second_operand_is_rejected_where_it_cannot_run(dev):
  BF = torch.bfloat16
  x = torch.zeros(1, 16, 16, 64, dtype=BF, device=dev)
  x2 = torch.zeros(1, 16, 16, 64, dtype=BF, device=dev)
  w = torch.zeros(320, 9 * 64 + 64, dtype=BF, device=dev)
  out = torch.empty(1, 16, 16, 320, dtype=BF, device=dev)
  for tile in (13, 15):                       # persistent / halo-staged tiles
    with pytest.raises(RuntimeError, match="a2"):
      ops.conv3x3(x, w, out, x2=x2, tile=tile)
  with pytest.raises(AssertionError):
    ops.conv3x3(x, w, torch.empty(1, 8, 8, 320, dtype=BF, device=dev), x2=x2, stride=2)


@pytest.mark.parametrize("M,C,tile,split", [(2048, 640, 0, 0), (1024, 1280, 9, 2), (512, 1280, 1, 3), (300, 320, 11, 1)])
def test_ffout_and_proj_out_as_one_folded_product(dev, M, C, tile, split):
  """out = x + Wp (h + W2 g + b2) + bp as ONE launch over (g | h) with the folded weights (Wp W2 | Wp)
  (layout.ff_proj_fold; ldm_gemm a2 on plain rows; unet.py:313, :338, :363-365): against the float64 oracle of the
  two Dense layers on the same bf16 inputs, and no worse than the two launches it replaces (whose intermediate y is
  rounded to bf16)."""
  from ldm_tf2_amd import layout as L
  BF = torch.bfloat16
  g = torch.Generator().manual_seed(41)
  gg = torch.randn(M, 4 * C, generator=g).to(BF)
  h = torch.randn(M, C, generator=g).to(BF)
  x = torch.randn(M, C, generator=g).to(BF)
  k2 = (torch.randn(4 * C, C, generator=g) * (4 * C) ** -0.5).numpy()
  kp = (torch.randn(C, C, generator=g) * C ** -0.5).numpy()
  b2, bp = torch.randn(C, generator=g).numpy(), torch.randn(C, generator=g).numpy()
  y = h.double() + gg.double() @ torch.from_numpy(k2).double() + torch.from_numpy(b2).double()
  want = x.double() + y @ torch.from_numpy(kp).double() + torch.from_numpy(bp).double()
  w, b = L.ff_proj_fold(k2, b2, kp, bp, BF, dev)
  assert tuple(w.shape) == (C, 5 * C)
  out = torch.full((M, C), float("nan"), dtype=BF, device=dev)
  ops.linear(gg.to(dev), w, out, bias=b, residual=x.to(dev), x2=h.to(dev), tile=tile, split_k=split)
  yd = torch.empty(M, C, dtype=BF, device=dev)
  ops.linear(gg.to(dev), L.dense_kernel(k2, BF, dev), yd, bias=torch.from_numpy(b2).to(dev), residual=h.to(dev))
  out2 = torch.empty(M, C, dtype=BF, device=dev)
  ops.linear(yd, L.dense_kernel(kp, BF, dev), out2, bias=torch.from_numpy(bp).to(dev), residual=x.to(dev))
  rel = lambda a: ((a.double().cpu() - want).norm() / want.norm()).item()
  r, r2 = rel(out), rel(out2)
  print(f"FF-out + proj_out folded M={M} C={C} tile {tile} split {split}: rel {r:.3e} (two launches {r2:.3e})")
  assert torch.isfinite(out.float()).all() and r < 5e-3 and r <= r2 * 1.2


def test_layernorm_fold_does_not_depend_on_the_deal_of_n_tiles(dev):
  """The LayerNorm-folded persistent launch gives the same bits however its n-tiles are dealt to workgroups (1, 2, 3
  or 6 per 256-row panel; split_k < 0 = workgroups per panel).  Round 4 found 8 - 46 of 25 M outputs differing by one
  bf16 ulp between deals: `q ik - mu mu` was fused differently in the epilogue's inlined copies (-ffp-contract=fast),
  so a row's variance depended on whether the n-tile was the workgroup's last."""
  from ldm_tf2_amd import layout as L
  BF = torch.bfloat16
  M, C, N = 32768, 320, 768
  g = torch.Generator().manual_seed(11)
  x = (torch.randn(M, C, generator=g) * 1.5 + 0.5 * torch.randn(M, 1, generator=g)).to(BF).to(dev)
  w = torch.randn(N, C, generator=g) * C ** -0.5
  gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
  wq, cs, bb = L.ln_fold(w, gamma.numpy(), beta.numpy(), torch.randn(N, generator=g).numpy(), BF, dev)
  outs = []
  for wg in (1, 2, 3, 6):
    out = torch.empty(M, N, dtype=BF, device=dev)
    ops.linear(x, wq, out, bias=bb, ln_fold=(cs, 1e-5), tile=14, split_k=-wg)
    outs.append(out)
  torch.cuda.synchronize()
  for o_ in outs[1:]:
    assert torch.equal(o_, outs[0])


def test_plan_entry_that_cannot_run_falls_back(dev, tmp_path):
  """ADVICE r3 (medium) / VERDICT r3 item 8: a table entry naming the persistent tile 13 for a convolution key
  whose epilogue (bias + addend + residual together) is not instantiated there, reached through BOTH launch
  paths -- the plain one and the deferred-reduce one every ResBlock convolution takes."""
  B, H, Cin, Cout = 2, 16, 64, 320
  g = torch.Generator(device="cpu").manual_seed(0)
  x = torch.randn(B, H, H, Cin, generator=g).to(dev).to(torch.bfloat16)
  w = (torch.randn(Cout, 9 * Cin, generator=g) * 0.05).to(dev).to(torch.bfloat16)
  bias = torch.randn(Cout, generator=g).to(dev)
  add = torch.randn(B, Cout, generator=g).to(dev)
  res = torch.randn(B, H, H, Cout, generator=g).to(dev).to(torch.bfloat16)
  p = ops._conv_params(x, w, torch.empty(B, H, H, Cout, dtype=torch.bfloat16, device=dev), bias, 1, False, add, res,
                       0, 0)
  key = ops.plan_key(p)
  before = ops.plan_tables()
  f = tmp_path / "bad.json"
  f.write_text(json.dumps({"config": {"rows": B, "latent": 1234, "dtype": "bf16"}, "plans": {key: [13, 1]}}))
  try:
    ops.load_plans(str(f))
    want = torch.empty(B, H, H, Cout, dtype=torch.bfloat16, device=dev)
    ops.conv3x3(x, w, want, bias=bias, addend=add, residual=res)          # no table: the cost model's plan
    with ops.plan_scope(B, 1234, torch.bfloat16):
      q = ops._conv_params(x, w, want, bias, 1, False, add, res, 0, 0)
      assert ops.resolve_plan(q) and q.tile == 13                          # the entry is live in this scope
      got = torch.empty_like(want)
      ops.conv3x3(x, w, got, bias=bias, addend=add, residual=res)
      got_d = torch.empty_like(want)
      pend = ops.conv3x3(x, w, got_d, bias=bias, addend=add, residual=res, defer_reduce=True)
      ops.finish(pend)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got_d, want)
  finally:
    ops.clear_plans()
    ops._load_default_plans()
  assert ops.plan_tables() == before
