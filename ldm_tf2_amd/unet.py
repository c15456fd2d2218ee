"""Conditioning U-Net on the HIP path -- host side.

Mirrors the reference's `UNet` operator (unet.py:51-138): same constructor
kwargs (= the YAML `unet` section), same call contract
`unet(x f32[R,h,w,4], t int32[R], context [R,77,D]) -> f32[R,h,w,4]`, NHWC.
The arithmetic runs in hand-written HIP kernels through the C ABI
(include/ldm_hip.h); this file only walks the block structure and hands out
buffers.  There is no CPU path.

What the host does differently from a line-by-line transcription (none of it
changes results beyond float rounding order):
  * the skip concatenation (unet.py:135) is free: every skip tensor and every
    block output is written straight into its channel slice of the buffer the
    consuming output block reads;
  * the timestep MLP (unet.py:126-127) and the 22 ResBlock temb projections
    (unet.py:386) depend only on t: they run once per call as four skinny-Dense
    launches; when all rows share one t (the DDIM loop, model_runners.py:449)
    they run for a single row;
  * cross-attention K and V of the text context (unet.py:274-275 with
    context != None) are step-invariant: `set_context` computes them once;
  * nearest-2x upsample (unet.py:44) is fused into the following conv, which runs as four 2x2 phase
    convolutions over the low-resolution image with pre-summed weights (ops.conv3x3_up2).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import layout as L
from . import ops
from .st_form import StFlags, StForm, st_form
from .weights import init_weights, unet_manifest

GN_EPS_RES = 1e-5   # unet.py:374,377,115
GN_EPS_ST = 1e-6    # unet.py:354
LN_EPS = 1e-5       # unet.py:304-306


class _Res:
  """ResidualBlock weights (unet.py:368-380).  The second convolution and the shortcut are kept in the one form
  the block launches: `conv2_sc` (a block with a shortcut, `merge_shortcut`), else `conv2` and, where the block has
  one, `shortcut`; the operands of the other form are None."""

  def __init__(self, w, p, dtype, dev, merge_shortcut=True):
    g = lambda n: w[p + "/" + n]
    self.cin, self.cout = g("conv2d_1/kernel").shape[2], g("conv2d_1/kernel").shape[3]
    self.gn1 = (L.vec(g("group_norm_1/gamma"), dev), L.vec(g("group_norm_1/beta"), dev))
    self.conv1 = (L.conv_kernel(g("conv2d_1/kernel"), dtype, dev), L.vec(g("conv2d_1/bias"), dev))
    self.temb_k, self.temb_b = g("dense/kernel"), g("dense/bias")   # gathered by the U-Net
    self.gn2 = (L.vec(g("group_norm_2/gamma"), dev), L.vec(g("group_norm_2/beta"), dev))
    self.conv2 = self.shortcut = self.conv2_sc = None
    if (p + "/shortcut/kernel") in w and merge_shortcut:
      # the shortcut as extra K columns of the second convolution (ldm_gemm a2): [Cout, 9 Cout + Cin], bias sum
      self.conv2_sc = (L.conv_shortcut_kernel(g("conv2d_2/kernel"), g("shortcut/kernel"), dtype, dev),
                       L.vec(np.asarray(g("conv2d_2/bias"), dtype=np.float32) + np.asarray(g("shortcut/bias"), dtype=np.float32), dev))
    else:
      self.conv2 = (L.conv_kernel(g("conv2d_2/kernel"), dtype, dev), L.vec(g("conv2d_2/bias"), dev))
      if (p + "/shortcut/kernel") in w:
        self.shortcut = (L.dense_kernel(g("shortcut/kernel"), dtype, dev), L.vec(g("shortcut/bias"), dev))
    self.temb_off = 0


class _ST:
  """SpatialTransformer weights (unet.py:341-354, :295-306, :248-265, :317-338)."""

  def __init__(self, w, p, heads, dtype, dev, fold_ln=False, matrix_softmax=True):
    g = lambda n: w[p + "/" + n]
    c = g("dense1/kernel").shape[0]
    self.c, self.heads = c, heads
    self.s = c // heads
    self.sp = L.padded_head(self.s)
    sp = self.sp
    self.gn = (L.vec(g("groupnorm/gamma"), dev), L.vec(g("groupnorm/beta"), dev))
    self.proj_in = (L.dense_kernel(g("dense1/kernel"), dtype, dev), L.vec(g("dense1/bias"), dev))
    self.proj_out = (L.dense_kernel(g("dense2/kernel"), dtype, dev), L.vec(g("dense2/bias"), dev))
    a1, a2 = p + "/block/att_layer1", p + "/block/att_layer2"
    self.qk1 = torch.cat([L.split_kernel(w[a1 + "/query/kernel"], sp, dtype, dev),
                          L.split_kernel(w[a1 + "/key/kernel"], sp, dtype, dev)], 0).contiguous()
    self.v1 = L.split_kernel(w[a1 + "/value/kernel"], sp, dtype, dev)
    self.qkv1 = torch.cat([self.qk1, self.v1], 0).contiguous()      # one launch: q | k | v (v stored as V^T)
    self.o1 = (L.merge_kernel(w[a1 + "/output/kernel"], sp, dtype, dev), L.vec(w[a1 + "/output/bias"], dev))
    self.q2 = L.split_kernel(w[a2 + "/query/kernel"], sp, dtype, dev)
    self.k2 = L.split_kernel(w[a2 + "/key/kernel"], sp, dtype, dev)
    self.v2 = L.split_kernel(w[a2 + "/value/kernel"], sp, dtype, dev)
    self.o2 = (L.merge_kernel(w[a2 + "/output/kernel"], sp, dtype, dev), L.vec(w[a2 + "/output/bias"], dev))
    self.geglu = L.geglu_kernel(g("block/ffn/geglu/kernel"), g("block/ffn/geglu/bias"), dtype, dev)
    self.ff_out = (L.dense_kernel(g("block/ffn/dense/kernel"), dtype, dev), L.vec(g("block/ffn/dense/bias"), dev))
    self.ln = [(L.vec(g(f"block/layernorm{i}/gamma"), dev), L.vec(g(f"block/layernorm{i}/beta"), dev))
               for i in (1, 2, 3)]
    # bf16: FF-out and proj_out as one product over (hidden | residual stream) (layout.ff_proj_fold; per-layer path)
    self.ffp = None
    if fold_ln:
      self.ffp = L.ff_proj_fold(g("block/ffn/dense/kernel"), g("block/ffn/dense/bias"), g("dense2/kernel"),
                                g("dense2/bias"), dtype, dev)
    # bf16: the three LayerNorms folded into the projections they feed (ldm_gemm ln_cs): (w', cs, b')
    self.fold = None
    # matrix-side softmax (ldm_attention_ms): 40-wide heads padded to 48, together with the fold (the
    # folded projections' biases carry the ones of the padded rows, their weights the exp2-domain scale)
    self.ms = bool(fold_ln and matrix_softmax and self.s == L.MS_DIM and sp == 48)
    self.ms_kbias = self.ms_vbias = None
    if fold_ln:
      lnp = [(g(f"block/layernorm{i}/gamma"), g(f"block/layernorm{i}/beta")) for i in (1, 2, 3)]
      f32, cpu = torch.float32, "cpu"
      hs = heads * sp
      qk_f = torch.cat([L.split_kernel(w[a1 + "/query/kernel"], sp, f32, cpu),
                        L.split_kernel(w[a1 + "/key/kernel"], sp, f32, cpu)], 0)
      gw, gb = L.geglu_kernel(g("block/ffn/geglu/kernel"), g("block/ffn/geglu/bias"), f32, cpu)
      qk_scale = qk_ones = v_ones = q_scale = None
      if self.ms:
        c2 = float(self.s) ** -0.5 * L.MS_LOG2E                  # unet.py:281 scale, in the exp2 domain
        qk_scale = torch.cat([torch.full((hs,), c2), torch.ones(hs)])
        qk_ones = L.ms_ones(heads, sp, offset=hs)                 # K[..., 40] = 1
        v_ones = L.ms_ones(heads, sp)                             # V^T row 40 = 1
        q_scale = torch.full((hs,), c2)
        self.ms_kbias, self.ms_vbias = v_ones.to(dev), v_ones.clone().to(dev)     # cross-attention K / V of the context
      v_f = L.split_kernel(w[a1 + "/value/kernel"], sp, f32, cpu)
      self.fold = dict(
          # q | k | v as ONE launch (row-major q | k, V^T transposed: ldm_gemm out2 with n_split = 2 heads Sp)
          qkv1=L.ln_fold(torch.cat([qk_f, v_f], 0), lnp[0][0], lnp[0][1], None, dtype, dev,
                         row_scale=None if qk_scale is None else torch.cat([qk_scale, torch.ones(hs)]),
                         bias_extra=None if qk_ones is None else torch.cat([qk_ones, v_ones])),
          qk1=L.ln_fold(qk_f, lnp[0][0], lnp[0][1], None, dtype, dev, row_scale=qk_scale, bias_extra=qk_ones),
          v1=L.ln_fold(v_f, lnp[0][0], lnp[0][1], None, dtype, dev, bias_extra=v_ones),
          q2=L.ln_fold(L.split_kernel(w[a2 + "/query/kernel"], sp, f32, cpu), lnp[1][0], lnp[1][1], None, dtype, dev,
                       row_scale=q_scale),
          geglu=L.ln_fold(gw, lnp[2][0], lnp[2][1], gb.numpy(), dtype, dev))
    # the whole feed-forward as one row-panel launch (ldm_ffn_geglu): C = 320 blocks, with the fold
    self.ffn_aux = None
    if self.fold is not None and c == 320:
      self.ffn_aux = L.ffn_aux(self.fold["geglu"][1], self.fold["geglu"][2])
    self.ctx_k = self.ctx_vt = None     # filled by UNet.set_context
    self.form = None                    # the StForm of the last evaluation (UNet._st)


class _StRun(NamedTuple):
  """What the launches after a block's self-attention read: the block, its form, the self-attention's output, the
  residual stream and the block input (all of out's rows, or half of them for ldm_st_block's in_rows), the block
  output, the context's projections, the heat-map setting or None."""
  st: _ST
  form: StForm
  att: torch.Tensor
  ha: torch.Tensor
  x: torch.Tensor
  out: torch.Tensor
  ctx_k: torch.Tensor
  ctx_vt: torch.Tensor
  cap: Optional[dict]


class UNet:
  """Same kwargs as the reference constructor (unet.py:52-61).  Extra, build-only
  kwargs: `weights` (reference-layout float32 dict, weights.unet_manifest names;
  None = random init, the reference's behaviour when no checkpoint restores),
  `dtype` (torch.float32 | torch.bfloat16 storage), `device`, `context_dim`."""

  def __init__(self, model_channels=320, out_channels=4, num_blocks=2,
               attention_resolutions=(4, 2, 1), dropout_rate=0.1, channel_mult=(1, 2, 4, 4),
               num_heads=8, *, weights=None, dtype=torch.float32, device="cuda:0",
               context_dim=1280, init="keras", seed=2, fuse_layernorm=False, fuse_qkv=True,
               split_qkv=True, small_conv_out=False, fold_layernorm=True, fold_min_rows=2048,
               defer_reduce=True, matrix_softmax=True, gn_single_launch=True, fused_ffn=True,
               ffn_min_rows=24576, fused_tail=True, fused_xattn=True, fused_block=True,
               shared_prefix=True, merge_qkv=True, merge_qkv_max_rows=1 << 30,
               merge_shortcut=True, merge_ffproj=True, block_min_rows=12288, phase_upsample=True):
    # the transformer blocks' launch-form switches and thresholds (st_form.StFlags holds what each one selects)
    self._st_flags = StFlags.of(dtype, fuse_layernorm=fuse_layernorm, fuse_qkv=fuse_qkv, split_qkv=split_qkv,
                                fold_layernorm=fold_layernorm, matrix_softmax=matrix_softmax, fused_ffn=fused_ffn,
                                fused_tail=fused_tail, fused_xattn=fused_xattn, fused_block=fused_block,
                                merge_qkv=merge_qkv, merge_qkv_max_rows=merge_qkv_max_rows, merge_ffproj=merge_ffproj,
                                fold_min_rows=fold_min_rows, ffn_min_rows=ffn_min_rows, block_min_rows=block_min_rows)
    self._fuse_ln = self._st_flags.fuse_ln
    self._small_conv_out = bool(small_conv_out)
    self._gn_single = bool(gn_single_launch)      # False: partial-sums + apply launches everywhere (A/B)
    self._defer_reduce = bool(defer_reduce)   # split-K reduces fused into the consuming GroupNorm (A/B: False)
    self._merge_shortcut = bool(merge_shortcut)   # ResBlock shortcut inside its second convolution's K loop (A/B: False)
    # the upsample convolutions as four 2x2 phase convolutions over the image itself (ops.conv3x3_up2: 4/9 of the
    # multiply-adds; only that weight form is built).  A/B: False = the nine-tap gather over the upsampled image
    self._phase_upsample = bool(phase_upsample)
    self._shared_prefix = bool(shared_prefix)     # forward(paired_rows=True): the CFG pair's common prefix once (A/B: False)
    self._ctx_sel = None                  # the context rows an evaluation attends to (forward(context_rows=)); None = all
    self._attn_cap = None                 # capture_attention: rows, layers and weight table of the heat maps; None = off
    self._attn_acc = {}                   # st index -> (h, w, accumulator) of the evaluations made with capture on
    self._attn_all = {}                   # every accumulator this model has handed out, by (st index, shape)
    self._fwd_index = None                # the device step counter of the evaluation in flight (forward(index=))
    self._pend = None
    self._taps = None                     # forward(taps=): the dict this evaluation stores its stage outputs in
    self._tapq = []                       # ... stage outputs that a deferred split-K product has yet to complete
    self._model_channels = model_channels
    self._out_channels = out_channels
    self._num_blocks = num_blocks
    self._attention_resolutions = attention_resolutions   # stored, never read (unet.py:66)
    self._dropout_rate = dropout_rate                     # inference: dropout inactive
    self._channel_mult = tuple(channel_mult)
    self._num_heads = num_heads
    self.dtype, self.device = dtype, torch.device(device)
    self.manifest = unet_manifest(model_channels, out_channels, num_blocks, self._channel_mult,
                                  num_heads, context_dim=context_dim)
    if weights is None:
      weights = init_weights(self.manifest, seed=seed, mode=init, scope="unet")
    missing = [k for k in self.manifest if k not in weights]
    if missing:
      raise KeyError(f"UNet weights missing {len(missing)} tensors, e.g. {missing[:3]}")
    self.buf = L.Buffers(self.device)
    self._ws = ops.new_workspace(self.device)   # this model's split-K workspace (ops.workspace_scope)
    self._compile(weights)

  # ---- build ---------------------------------------------------------------------
  def _compile(self, w):
    dt, dev, H = self.dtype, self.device, self._num_heads
    mc = self._model_channels
    self.conv_in = (L.vec(w["conv_in/kernel"], dev), L.vec(w["conv_in/bias"], dev))
    self.time1 = (L.dense_kernel(w["time_dense1/kernel"], dt, dev), L.vec(w["time_dense1/bias"], dev))
    self.time2 = (L.dense_kernel(w["time_dense2/kernel"], dt, dev), L.vec(w["time_dense2/bias"], dev))
    res_all = []

    def mk_res(p):
      r = _Res(w, p, dt, dev, merge_shortcut=self._merge_shortcut)
      res_all.append(r)
      return r

    def mk_st(p):
      return (_ST(w, p, H, dt, dev, fold_ln=self._st_flags.fold_ln, matrix_softmax=self._st_flags.matrix_softmax)
              if (p + "/dense1/kernel") in w else None)

    self.in_blocks, self.skip_ch, self.skip_lvl = [], [mc], [0]
    lvl, i = 0, 0
    while any(k.startswith(f"input_blocks/{i}/") for k in w):
      p = f"input_blocks/{i}"
      if (p + "/downsample/conv/kernel") in w:
        k = w[p + "/downsample/conv/kernel"]
        self.in_blocks.append(("down", L.conv_kernel(k, dt, dev), L.vec(w[p + "/downsample/conv/bias"], dev)))
        lvl += 1
        self.skip_ch.append(k.shape[3])
      else:
        r = mk_res(p + "/residual")
        self.in_blocks.append(("res", r, mk_st(p + "/spatial_transformer")))
        self.skip_ch.append(r.cout)
      self.skip_lvl.append(lvl)
      i += 1
    self.mid = (mk_res("middle_block/residual1"), mk_st("middle_block/spatial_transformer"),
                mk_res("middle_block/residual2"))
    self.out_blocks = []
    i = 0
    while any(k.startswith(f"output_blocks/{i}/") for k in w):
      p = f"output_blocks/{i}"
      up = None
      if (p + "/upsample/conv/kernel") in w:
        mk = L.upsample_phase_kernel if self._phase_upsample else L.conv_kernel
        up = (mk(w[p + "/upsample/conv/kernel"], dt, dev), L.vec(w[p + "/upsample/conv/bias"], dev))
      self.out_blocks.append((mk_res(p + "/residual"), mk_st(p + "/spatial_transformer"), up))
      i += 1
    assert len(self.out_blocks) == len(self.skip_ch), "U-Net skip structure mismatch"
    self.gn_out = (L.vec(w["groupnorm/gamma"], dev), L.vec(w["groupnorm/beta"], dev))
    self.conv_out = (L.vec(w["conv_out/kernel"], dev), L.vec(w["conv_out/bias"], dev))
    # bf16: the 320 -> 4 output conv as an implicit-GEMM launch too (N = 4 of a 64-column tile is
    # wasted MFMA work, but 3 GFLOP on the matrix cores beat the 8-threads-per-pixel FMA kernel 4x);
    # small_conv_out=True: the scalar kernel (A/B)
    self.conv_out_mm = (L.conv_kernel(w["conv_out/kernel"], dt, dev)
                        if dt == torch.bfloat16 and not self._small_conv_out else None)
    # all ResBlock temb projections as ONE skinny Dense [sum(Cout), 4*mc]
    off, ks, bs = 0, [], []
    for r in res_all:
      r.temb_off = off
      off += r.cout
      ks.append(L.dense_kernel(r.temb_k, dt, dev))
      bs.append(L.vec(r.temb_b, dev))
      r.temb_k = r.temb_b = None
    self.temb_all = (torch.cat(ks, 0).contiguous(), torch.cat(bs, 0).contiguous())
    self.temb_total = off
    self.sts = [b[2] for b in self.in_blocks if b[0] == "res" and b[2] is not None]
    self.sts += [self.mid[1]] + [b[1] for b in self.out_blocks if b[1] is not None]
    for n, st in enumerate(self.sts):
      st.index = n

  # ---- step-invariant cross-attention K / V ------------------------------------------
  def set_context(self, context):
    """Projects the text context through every cross-attention key/value layer once
    (unet.py:274-275).  The projections land in buffers owned by this model (one set per
    context shape), so a captured step graph stays valid across calls; callers invoke this
    EVERY time they are handed a context (32 small GEMMs) -- nothing is cached on tensor
    identity, because a freed context's address is routinely reused by the next one."""
    if context.dtype != self.dtype:
      c2 = self.buf.get("ctx_cast", context.shape, self.dtype)
      ops.cast(context, c2)
      context = c2
    R, Tk, _ = context.shape
    if self._attn_cap is not None:
      self._check_attention(self._attn_cap["layers"], Tk)
    tkp = (Tk + 7) // 8 * 8
    with ops.workspace_scope(self._ws):
      for n, st in enumerate(self.sts):
        hs = st.heads * st.sp
        st.ctx_k = self.buf.get(f"ctxk{n}", (R, Tk, hs), self.dtype)
        st.ctx_vt = self.buf.get(f"ctxv{n}", (R, hs, tkp), self.dtype, zero=True)
        # (matrix-side softmax blocks: 1.0 in the padded dim 40 of every head of K and V^T; inert for
        # the plain attention kernel, whose Q is zero there)
        ops.linear(context, st.k2, st.ctx_k, bias=st.ms_kbias)
        ops.bmm_nt(context, st.v2, st.ctx_vt, transposed_out=True, bias=st.ms_vbias)
    self._ctx_rows = R

  # ---- cross-attention heat maps ------------------------------------------
  def _check_attention(self, layers, Tk):
    for n in layers:
      st = self.sts[n]
      if not ops.xattn_map_supported(st.heads, Tk, st.s, st.sp, self.dtype):
        raise ValueError(f"capture_attention: layer {n} (heads={st.heads}, head size {st.s} padded to {st.sp}) with "
                         f"{Tk} context tokens is outside ldm_xattn_map's range (at most 80 tokens)")

  def capture_attention(self, rows=None, layers=None, step_w=None, index_bias=0):
    """Turns the cross-attention heat maps on or off (off: `rows` None, the default).  On, every forward adds, for
    each transformer block n in `layers` (indices into self.sts; None = all), the head-averaged cross-attention
    probabilities of the batch rows `rows` = (r0, r1) into a float32 accumulator [r1-r0, h, w, Tk] of this model
    (attention_layers; one ldm_xattn_map launch per layer in front of its cross-attention, the block without the
    ldm_st_block form, which never materialises the queries).  `step_w` (device float32 [N]) weights an evaluation
    by step_w[index[0] + index_bias] with forward's device `index`, a zero or an index outside the table adding
    nothing; None: every evaluation counts once.  The accumulators keep their addresses, so a captured graph of the
    forward stays valid; a graph captured with another setting does not see a change made here."""
    if rows is None:
      self._attn_cap = None
      return
    r0, r1 = (int(v) for v in rows)
    if not 0 <= r0 < r1:
      raise ValueError(f"capture_attention: rows must be (r0, r1) with 0 <= r0 < r1, got {rows!r}")
    layers = list(range(len(self.sts))) if layers is None else [int(n) for n in layers]
    if not layers or sorted(set(layers)) != sorted(layers) or not all(0 <= n < len(self.sts) for n in layers):
      raise ValueError(f"capture_attention: layers must be distinct indices below {len(self.sts)}, got {layers!r}")
    if step_w is not None and (step_w.dtype != torch.float32 or step_w.dim() != 1 or not step_w.is_cuda):
      raise ValueError("capture_attention: step_w must be a device float32 vector")
    self._check_attention(layers, 1 if self.sts[0].ctx_k is None else self.sts[0].ctx_k.shape[1])
    self._attn_cap = dict(rows=(r0, r1), layers=frozenset(layers), step_w=step_w, index_bias=int(index_bias))
    self._attn_acc = {}                   # (attention_layers lists what THIS setting's evaluations reach)

  def attention_layers(self):
    """[(st index, h, w, acc)]: the accumulators float32 [r1-r0, h, w, Tk] (device) of the captured layers that an
    evaluation has reached, in layer order."""
    if self._attn_cap is None:
      return []
    return [(n,) + self._attn_acc[n] for n in sorted(self._attn_cap["layers"]) if n in self._attn_acc]

  def reset_attention_maps(self):
    """Zeroes every accumulator of this model (all layers and shapes; their addresses stay)."""
    for acc in self._attn_all.values():
      acc.zero_()

  def _attn_map(self, st, cap, q, ctx_k, h, w, scale, ms):
    r0, r1 = cap["rows"]
    if r1 > q.shape[0]:
      raise ValueError(f"capture_attention: rows {cap['rows']} exceed the evaluation's {q.shape[0]} rows")
    Tk = ctx_k.shape[1]
    acc = self.buf.get(f"xmap{st.index}", (r1 - r0, h, w, Tk), torch.float32, zero=True)
    self._attn_acc[st.index] = (h, w, acc)
    self._attn_all[st.index, tuple(acc.shape)] = acc
    # (matrix-softmax blocks: the folded query projection carries s^-1/2 log2(e) already)
    ops.xattn_map(q[r0:r1], ctx_k[r0:r1], acc, st.heads, st.s, st.sp, 1.0 if ms else scale * L.MS_LOG2E,
                  step_w=cap["step_w"], index=self._fwd_index if cap["step_w"] is not None else None,
                  index_bias=cap["index_bias"])

  # ---- blocks ------------------------------------------------------------------------------
  # ---- split-K products whose reduce is fused into the GroupNorm that consumes them ---------------
  # A split-K convolution leaves float32 slabs; its reduce + epilogue launch is followed, almost
  # everywhere in the U-Net, by the GroupNorm of exactly that tensor.  `_conv_deferred` launches only the
  # main kernel and parks the slabs (self._pend); `_gn` completes them inside the GroupNorm launch
  # (ldm_groupnorm_splitk: same value, bit for bit, one launch and one bf16 round trip less).  Whatever
  # else is about to read the tensor or use the workspace calls `_flush` first (plain reduce).
  def _flush(self):
    if self._pend is not None:
      ops.finish(self._pend)
      self._pend = None
    self._tap_drain()

  # ---- stage taps (forward(taps=)): copies only, no launch of the evaluation moves ---------------------------
  def _tap(self, name, t):
    """Stores a clone of stage output `t`.  While a deferred split-K product is outstanding `t` may be the tensor
    its slabs still have to be summed into: the clone is queued and made by the GroupNorm or flush that completes
    the product (never by an early flush, which would replace ldm_groupnorm_splitk with the plain reduce) -- that
    is before the next writer of the reused scratch tags (blk_r, blk_s), whose producer flushes first."""
    if self._taps is None:
      return
    if self._pend is not None:
      self._tapq.append((name, t))
    else:
      self._taps[name] = t.clone()

  def _tap_drain(self):
    if self._tapq:
      for name, t in self._tapq:
        self._taps[name] = t.clone()
      self._tapq = []

  def _conv_deferred(self, x, wt, out, **kw):
    self._flush()
    self._park(ops.conv3x3(x, wt, out, defer_reduce=self._defer_reduce, **kw))
    return out

  def _park(self, r):
    """`r`: what a launch with defer_reduce returned -- its slabs if the plan split K, for `_gn` or `_flush`."""
    self._pend = r if isinstance(r, ops.PendingReduce) else None

  def _gn(self, x, gn, eps, silu, out, store_x=True):
    pend, self._pend = self._pend, None
    ops.groupnorm(x, gn[0], gn[1], out, eps, silu=silu, partial=self._gnp, pending=pend, store_x=store_x,
                  fused=None if self._gn_single else False)
    self._tap_drain()                     # (x is complete now: store_x is False only for a tensor no stage ends in)
    return out

  def _res(self, r, x, tall, out):
    B_, dt = self.buf, self.dtype
    R, h, w, _ = x.shape
    # GN1 first: it completes a deferred product that produced x (x is materialised by that launch)
    t0 = B_.get("gn", tuple(x.shape), dt)
    self._gn(x, r.gn1, GN_EPS_RES, True, t0)
    res = x
    if r.shortcut is not None:                  # before conv1: the slabs of conv1 must survive until GN2
      res = B_.get("sc", (R, h, w, r.cout), dt)
      ops.linear(x, r.shortcut[0], res, bias=r.shortcut[1])
    h1 = B_.get("h1", (R, h, w, r.cout), dt)
    self._conv_deferred(t0, r.conv1[0], h1, bias=r.conv1[1], addend=tall[:, r.temb_off:r.temb_off + r.cout])
    t1 = B_.get("gn", (R, h, w, r.cout), dt)
    self._gn(h1, r.gn2, GN_EPS_RES, True, t1, store_x=False)      # h1 has no other reader (unet.py:388-390)
    # conv2's reduce is left to the next GroupNorm (the following block's first op) when that reads `out`
    if r.conv2_sc is not None:
      # unet.py:393-397: shortcut(x) + conv2(...) as ONE product -- the shortcut's channels are extra K columns of
      # the convolution (ldm_gemm a2): no launch and no [M, Cout] tensor of its own
      self._conv_deferred(t1, r.conv2_sc[0], out, bias=r.conv2_sc[1], x2=x)
    else:
      self._conv_deferred(t1, r.conv2[0], out, bias=r.conv2[1], residual=res)
    return out

  def _pair_buf(self, tag, shape, dt, pair):
    """(view, full): scratch for a tensor of `shape`; for a CFG pair the buffer has twice the rows and `view` is
    its first half, so that leaving the common prefix is ONE copy of the first half onto the second (_dup_rows)."""
    if not pair:
      t = self.buf.get(tag, shape, dt)
      return t, t
    full = self.buf.get(tag + "_pair", (2 * shape[0],) + tuple(shape[1:]), dt)
    return full[:shape[0]], full

  def _dup_rows(self, full):
    """full[n:] = full[:n] (a CFG pair leaving its common prefix on a path without ldm_st_block's in_rows)."""
    n = full.shape[0] // 2
    ops.cast(full[:n], full[n:])
    return full

  def _st(self, st, x, out, pair=False, x_full=None):
    """One transformer block (unet.py:341-365): pick its form (st_form), run the head up to the self-attention, then
    the form's way to the block's output.  `pair`: x holds the first half of out's rows and the second half is
    identical up to the first cross-attention (forward(paired_rows=True)); out and the context cover all rows, and
    `x_full` is x's buffer with room for them."""
    R, h, w, c = x.shape
    ctx_k, ctx_vt = (st.ctx_k, st.ctx_vt) if self._ctx_sel is None else (st.ctx_k[self._ctx_sel], st.ctx_vt[self._ctx_sel])
    assert ctx_k.shape[0] == (2 * R if pair else R) and out.shape[0] == ctx_k.shape[0]
    cap = self._attn_cap if self._attn_cap is not None and st.index in self._attn_cap["layers"] else None
    form = st.form = st_form(self._st_flags, self.dtype, c, st.heads, st.s, st.sp, st.fold is not None,
                             st.ffn_aux is not None, st.ffp is not None, st.ms, R, pair, h * w, ctx_k.shape[1],
                             ctx_vt.shape[2], cap is not None)
    (att, att_full), (ha, ha_full) = self._st_head(st, form, x, pair)
    if form.leave_prefix:
      # per-layer path: the pair leaves its common prefix here -- both halves get their copy of the self-attention's
      # output, the residual stream and the block input, and everything below covers all rows
      ins = self._dup_rows(att_full), self._dup_rows(ha_full), self._dup_rows(x_full)
    else:
      ins = att, ha, x                    # ("block" with a pair: half of out's rows -> ldm_st_block's in_rows)
    self._ST_REST[form.rest](self, _StRun(st, form, *ins, out, ctx_k, ctx_vt, cap))
    return out

  def _ln_buf(self, like):
    return self.buf.get("st_ln", tuple(like.shape), self.dtype)

  def _lnp(self, st, form, i, hn):
    """`ln=` of the GEMM that produces the residual stream `hn`: each LayerNorm of the block normalises a row the
    preceding projection has just produced, so where the GEMM tile holds whole rows it is emitted by that GEMM's
    epilogue (the "epilogue" form); else None."""
    return (st.ln[i][0], st.ln[i][1], self._ln_buf(hn), LN_EPS) if form.norm == "epilogue" else None

  def _normed(self, st, form, i, hn):
    """LayerNorm i of the residual stream `hn` for a consumer without the fold: its own launch ("separate") unless
    the GEMM that produced `hn` has emitted it."""
    ln = self._ln_buf(hn)
    if form.norm == "separate":
      ops.layernorm(hn, st.ln[i][0], st.ln[i][1], ln, LN_EPS)
    return ln

  def _st_head(self, st, form, x, pair):
    """GroupNorm, proj_in, the self-attention's projections in the form's norm / qkv arm and the self-attention
    (unet.py:355-357, :309-310): (attention output, residual stream), each as _pair_buf's (view, full)."""
    B_, dt, fold = self.buf, self.dtype, st.fold
    R, h, w, c = x.shape
    T, hs = h * w, st.heads * st.sp
    t0 = B_.get("gn", (R, h, w, c), dt)
    self._gn(x, st.gn, GN_EPS_ST, False, t0)
    ha, ha_full = self._pair_buf("st_a", (R, T, c), dt, pair)
    ops.linear(t0, st.proj_in[0], ha, bias=st.proj_in[1], ln=self._lnp(st, form, 0, ha))
    qk = B_.get("st_qk", (R, T, 2 * hs), dt)
    vt = B_.get("st_vt", (R, hs, (T + 7) // 8 * 8), dt, zero=True)
    if form.qkv == "qkv_fold":
      # q | k | V^T: one pass of the persistent kernel over the LayerNorm'ed rows (gemm3_kernel EPI bit 7)
      ops.linear(ha, fold["qkv1"][0], qk, bias=fold["qkv1"][2], ln_fold=(fold["qkv1"][1], LN_EPS), out2=vt)
    elif form.qkv == "qk_v_fold":
      ops.linear(ha, fold["qk1"][0], qk, bias=fold["qk1"][2], ln_fold=(fold["qk1"][1], LN_EPS))
      ops.linear_t(ha, fold["v1"][0], vt, bias=fold["v1"][2], ln_fold=(fold["v1"][1], LN_EPS))
    else:
      ln = self._normed(st, form, 0, ha)
      if form.qkv == "qk_vt":
        # bf16: q|k row-major and v TRANSPOSED (straight into the attention kernel's V^T layout) as two
        # launches that can both take the persistent kernel (ops.linear_t)
        ops.linear(ln, st.qk1, qk)
        ops.linear_t(ln, st.v1, vt)
      elif form.qkv == "qkv_out2":
        # q | k | v in ONE launch: q|k row-major, v straight into the attention kernel's V^T layout
        ops.linear(ln, st.qkv1, qk, out2=vt)
      else:
        ops.linear(ln, st.qk1, qk)
        ops.bmm_nt(ln, st.v1, vt, transposed_out=True)
    att, att_full = self._pair_buf("st_att", (R, T, hs), dt, pair)
    ops.attention(qk[..., :hs], qk[..., hs:], vt, att, st.heads, st.sp, st.s ** -0.5, matrix_softmax=form.ms)
    return (att, att_full), (ha, ha_full)

  # ---- the six ways from the self-attention's output to the block's output (StForm.rest), each a prefix of launches
  # shared with the next one down plus its own: b = _StRun
  def _st_block(self, b):
    """Everything as ONE row-panel launch (ldm_st_block)."""
    st, q2 = b.st, b.st.fold["q2"]
    ops.st_block(b.att, st.o1[0], st.o1[1], b.ha, q2[0], q2[1], q2[2], b.ctx_k, b.ctx_vt, st.o2[0], st.o2[1],
                 st.fold["geglu"][0], st.ffn_aux, st.ff_out[0], st.ff_out[1], st.proj_out[0], st.proj_out[1], b.x, b.out,
                 LN_EPS)

  def _st_query(self, b):
    """o1-projection + residual, the cross-attention's queries (unet.py:310-311) and, captured, their heat map:
    (residual stream, queries)."""
    st = b.st
    hb = self.buf.get("st_b", tuple(b.ha.shape), self.dtype)
    q = self.buf.get("st_q", tuple(b.att.shape), self.dtype)
    ops.linear(b.att, st.o1[0], hb, bias=st.o1[1], residual=b.ha, ln=self._lnp(st, b.form, 1, hb))
    if b.form.norm == "fold":
      q2 = st.fold["q2"]
      ops.linear(hb, q2[0], q, bias=q2[2], ln_fold=(q2[1], LN_EPS))
    else:
      ops.linear(self._normed(st, b.form, 1, hb), st.q2, q)
    if b.cap is not None:
      self._attn_map(st, b.cap, q, b.ctx_k, b.x.shape[1], b.x.shape[2], st.s ** -0.5, b.form.ms)
    return hb, q

  def _st_xtail(self, b):
    """... with the cross-attention itself in front of the tail, in place in the LDS panel (ldm_st_xtail)."""
    st = b.st
    hb, q = self._st_query(b)
    ops.st_xtail(q, b.ctx_k, b.ctx_vt, st.o2[0], st.o2[1], hb, st.fold["geglu"][0], st.ffn_aux, st.ff_out[0],
                 st.ff_out[1], st.proj_out[0], st.proj_out[1], b.x, b.out, LN_EPS)

  def _st_cross(self, b):
    """... the cross-attention as its own launch, into b.att (unet.py:311-312): the residual stream."""
    hb, q = self._st_query(b)
    ops.attention(q, b.ctx_k, b.ctx_vt, b.att, b.st.heads, b.st.sp, b.st.s ** -0.5, matrix_softmax=b.form.ms)
    return hb

  def _st_tail(self, b):
    """o-projection + residual, LayerNorm -> GEGLU -> FF-out + residual, proj_out + residual: ONE row-panel launch;
    the two intermediate residual-stream tensors live only in LDS (ldm_st_tail; unet.py:312-313, :363-365)."""
    st = b.st
    hb = self._st_cross(b)
    ops.st_tail(b.att, st.o2[0], st.o2[1], hb, st.fold["geglu"][0], st.ffn_aux, st.ff_out[0], st.ff_out[1],
                st.proj_out[0], st.proj_out[1], b.x, b.out, LN_EPS)

  def _st_o2(self, b):
    """... the o-projection + residual as its own launch, into b.ha: the scratch the stream has left."""
    hb = self._st_cross(b)
    ops.linear(b.att, b.st.o2[0], b.ha, bias=b.st.o2[1], residual=hb, ln=self._lnp(b.st, b.form, 2, b.ha))
    return hb

  def _st_ffn(self, b):
    """LayerNorm -> GEGLU -> FF-out + residual as ONE row-panel launch: the [R*T, 4C] hidden activation never
    reaches HBM (ldm_ffn_geglu; unet.py:313)."""
    st = b.st
    hb = self._st_o2(b)
    ops.ffn_geglu(b.ha, st.fold["geglu"][0], st.ffn_aux, st.ff_out[0], st.ff_out[1], hb, LN_EPS)
    ops.linear(hb, st.proj_out[0], b.out, bias=st.proj_out[1], residual=b.x)

  def _st_geglu(self, b):
    """... the GEGLU projection as its own launch (unet.py:313, :323-325, :335-338): (scratch, hidden activation)."""
    st = b.st
    hb = self._st_o2(b)
    ff = self.buf.get("st_ff", tuple(b.ha.shape[:2]) + (4 * st.c,), self.dtype)
    if b.form.norm == "fold":
      g = st.fold["geglu"]
      ops.linear(b.ha, g[0], ff, bias=g[2], act=ops.ACT_GEGLU, ln_fold=(g[1], LN_EPS))
    else:
      ops.linear(self._normed(st, b.form, 2, b.ha), st.geglu[0], ff, bias=st.geglu[1], act=ops.ACT_GEGLU)
    return hb, ff

  def _st_ffproj(self, b):
    """y = h + FF-out(ff) and proj_out(y) + x are two linear layers with a residual between them: ONE product over
    (ff | h) with the folded weights (Wp W2 | Wp) -- no proj_out launch, no y tensor (unet.py:313, :363-365).  Its
    split-K reduce is left to the GroupNorm that reads `out` next -- the following ResBlock's, on the way down --
    like a convolution's; whatever else comes next flushes it as a plain reduce."""
    _, ff = self._st_geglu(b)
    self._flush()
    self._park(ops.linear(ff, b.st.ffp[0], b.out, bias=b.st.ffp[1], residual=b.x, x2=b.ha,
                          defer_reduce=self._defer_reduce))

  def _st_layers(self, b):
    """FF-out + residual and proj_out + residual, a launch each."""
    st = b.st
    hb, ff = self._st_geglu(b)
    ops.linear(ff, st.ff_out[0], hb, bias=st.ff_out[1], residual=b.ha)
    ops.linear(hb, st.proj_out[0], b.out, bias=st.proj_out[1], residual=b.x)

  _ST_REST = dict(block=_st_block, xtail=_st_xtail, tail=_st_tail, ffn=_st_ffn, ffproj=_st_ffproj, layers=_st_layers)

  def forms(self):
    """[(st index, StForm)]: the form each transformer block took in the last evaluation that reached it."""
    return [(st.index, st.form) for st in self.sts if st.form is not None]

  def _res_st(self, prefix, r, st, x, tall, dst, last=True, res="residual"):
    """ResBlock, then the level's transformer block where it has one, a tap after each.  The last of them writes
    `dst` if nothing of the block follows it (`last`), every other stage scratch.  Returns that last output."""
    scratch = lambda tag: self.buf.get(tag, tuple(x.shape[:3]) + (r.cout,), self.dtype)
    o = self._res(r, x, tall, dst if st is None and last else scratch("blk_r"))
    self._tap(f"{prefix}/{res}", o)
    if st is not None:
      o = self._st(st, o, dst if last else scratch("blk_s"))
      self._tap(f"{prefix}/spatial_transformer", o)
    return o

  # ---- forward ---------------------------------------------------------------------------------
  def forward(self, x, t_rows=None, steps=None, index=None, out=None, shared_t=False, paired_rows=False,
              temb_table=None, pre_decrement=False, context_rows=None, taps=None):
    """x f32 [R,h,w,4].  Timestep either per row (`t_rows` int32 [R]) or, for the
    graph-replayed DDIM loop, `steps[*index]` for every row.  `shared_t=True` with
    t_rows declares that all rows carry t_rows[0].
    `paired_rows=True` declares that rows r and r + R/2 carry the SAME x and t and differ only in their context
    (the classifier-free-guidance batch concat([xt, xt]) of model_runners.py:449-452).  Nothing of the U-Net mixes
    rows and the context first enters at the first cross-attention (unet.py:311), so the launches in front of it
    -- the first ResBlock and the first transformer block up to its self-attention -- are the same numbers for both
    halves: they run once, on R/2 rows (`shared_prefix`, bf16 and float32).
    `temb_table` (from `temb_table(steps)`) with `index`: the step's temb projections are row *index of that table
    (one launch instead of four); `pre_decrement`: that launch first decrements *index, the DDIM loop's counter.
    `context_rows=(lo, hi)`: x has hi - lo rows and row r attends to row lo + r of the resident context (set_context
    projected more rows than this evaluation has): the conditional half (B, 2B) of a classifier-free-guidance batch on
    its own.  The cross-attention launches read contiguous row slices of the projections.
    `taps` (a dict; eager only): the evaluation stores a clone of every stage's output in it, in the storage type,
    under the stage's weight prefix -- conv_in, temb (the whole projected table), input_blocks/{i}/residual |
    spatial_transformer | downsample, middle_block/residual1 | spatial_transformer | residual2,
    output_blocks/{j}/residual | spatial_transformer | upsample, out.  The launches and their order are those of
    the evaluation without taps, and so are the output's bits; on the shared prefix of `paired_rows` a stage has
    R/2 rows and the tap holds those."""
    if taps is not None:
      if not isinstance(taps, dict):
        raise ValueError("forward(taps=) takes a dict")
      if torch.cuda.is_current_stream_capturing():
        raise ValueError("forward(taps=) is eager only: a capturing stream cannot hand out clones")
    assert x.dtype == torch.float32 and x.is_contiguous()
    R, h, w, _ = x.shape
    nlev = max(self.skip_lvl)
    assert h % (1 << nlev) == 0 and w % (1 << nlev) == 0, "latent size must divide by 2**levels"
    assert self.sts[0].ctx_k is not None, "call set_context(context) first"
    if context_rows is None:
      assert self._ctx_rows == R, "call set_context(context) first"
    else:
      lo, hi = (int(v) for v in context_rows)
      assert 0 <= lo and hi <= self._ctx_rows and hi - lo == R, (context_rows, self._ctx_rows, R)
      assert not paired_rows, "paired_rows needs the whole context"
      if self._attn_cap is not None:
        raise ValueError("capture_attention and forward(context_rows=) do not combine")
    if out is None:
      out = torch.empty(R, h, w, self._out_channels, dtype=torch.float32, device=self.device)
    if temb_table is not None:
      assert index is not None and temb_table.shape[1] == self.temb_total
      tall = self.buf.get("temb_all", (1, self.temb_total), torch.float32)
      ops.select_row(temb_table, index, tall, pre_decrement=pre_decrement)
    else:
      assert not pre_decrement
      tall = self._temb(R, t_rows, steps, index, shared_t)
    self._taps, self._tapq = taps, []
    self._tap("temb", tall)
    self._ctx_sel = None if context_rows is None else slice(lo, lo + R)
    self._fwd_index = index
    # a CFG pair: the launches in front of the first cross-attention once, on the first R/2 rows
    pair = bool(paired_rows and self._shared_prefix and R % 2 == 0
                and self.in_blocks[0][0] == "res" and self.in_blocks[0][2] is not None)
    B_, dt = self.buf, self.dtype
    half = R // 2
    n_in, n_out = len(self.in_blocks), len(self.out_blocks)
    # the skip / concat buffers: cats[j] = input of output block j = [previous output | skip n_in - j]
    prev_ch = [self.mid[2].cout] + [b[0].cout for b in self.out_blocks[:-1]]
    cats = []
    for j in range(n_out):
      i = n_in - j
      lv = self.skip_lvl[i]
      cats.append(B_.get(f"cat{j}", (R, h >> lv, w >> lv, prev_ch[j] + self.skip_ch[i]), dt))
    final = B_.get("final", (R, h, w, self.out_blocks[-1][0].cout), dt)
    skip = lambda i: cats[n_in - i][..., prev_ch[n_in - i]:]       # where skip tensor i lives
    # this model's scratch and workspace, the launch plans measured for this row count
    with ops.plan_scope(R, h, dt), ops.workspace_scope(self._ws):
      self._pend = None
      self._gnp = B_.get("gn_partial", (R * 128 * 32 * 2,), torch.float32)
      try:
        if pair:
          # both halves of x are the same rows -- the convolution once, its output copied (the skip tensor is read
          # with all rows by the last output block)
          d0 = skip(0)
          ops.conv3x3_small(x[:half], self.conv_in[0], self.conv_in[1], d0[:half])
          ops.cast(d0[:half], d0[half:])
        else:
          ops.conv3x3_small(x, self.conv_in[0], self.conv_in[1], skip(0))
        self._tap("conv_in", skip(0))
        for i, blk in enumerate(self.in_blocks):
          cur, dst = skip(i), skip(i + 1)
          if blk[0] == "down":
            self._conv_deferred(cur, blk[1], dst, bias=blk[2], stride=2)     # (flushes first: it reads cur)
            self._tap(f"input_blocks/{i}/downsample", dst)
            continue
          _, r, st = blk
          if i == 0 and pair:
            # the pair's common prefix: ResBlock + the transformer block's head on the first R/2 rows, with the
            # launch plans of THAT row count; the block's tail (from the first cross-attention on) on all rows
            self._flush()
            with ops.plan_scope(half, h, dt):
              tmp, tmp_full = self._pair_buf("blk_r", (half,) + tuple(dst.shape[1:3]) + (r.cout,), dt, True)
              self._res(r, cur[:half], tall if tall.shape[0] == 1 else tall[:half], tmp)
              self._tap(f"input_blocks/{i}/residual", tmp)
              self._st(st, tmp, dst, pair=True, x_full=tmp_full)
            self._tap(f"input_blocks/{i}/spatial_transformer", dst)
          else:
            self._res_st(f"input_blocks/{i}", r, st, cur, tall, dst)
        r1, stm, r2 = self.mid
        m2 = self._res_st("middle_block", r1, stm, skip(n_in), tall, None, last=False, res="residual1")
        self._res(r2, m2, tall, cats[0][..., :r2.cout])
        self._tap("middle_block/residual2", cats[0][..., :r2.cout])
        for j, (r, st, up) in enumerate(self.out_blocks):
          dst = final if j + 1 == n_out else cats[j + 1][..., :r.cout]
          o = self._res_st(f"output_blocks/{j}", r, st, cats[j], tall, dst, last=up is None)
          if up is not None:
            self._flush()                                           # it reads o
            if self._phase_upsample:                                # unet.py:44-47
              ops.conv3x3_up2(o, up[0], dst, bias=up[1])
            else:
              ops.conv3x3(o, up[0], dst, bias=up[1], upsample=True)
            self._tap(f"output_blocks/{j}/upsample", dst)
        t0 = B_.get("gn", tuple(final.shape), dt)
        self._gn(final, self.gn_out, GN_EPS_RES, True, t0)
        if self.conv_out_mm is not None:
          ops.conv3x3(t0, self.conv_out_mm, out, bias=self.conv_out[1])
        else:
          ops.conv3x3_small(t0, self.conv_out[0], self.conv_out[1], out)
        self._tap("out", out)
      finally:
        self._flush()
        self._taps, self._tapq = None, []
    return out

  def temb_table(self, steps):
    """[len(steps), sum of Cout] float32: the temb projections of every timestep in `steps` (int32, device) -- the
    same launches, row by row the same arithmetic, as one evaluation makes for its own t (unet.py:125-127, :386).
    The DDIM loop builds it once and hands it to every step (forward(temb_table=...))."""
    n = steps.numel()
    tall = self._temb(n, steps.to(torch.int32).contiguous(), None, None, False, tag="tbl")
    return tall

  def _temb(self, R, t_rows, steps, index, shared_t, tag=""):
    """timestep embedding + MLP + all temb projections (unet.py:125-127, :386): [1 or R, sum of Cout] f32."""
    B_, mc = self.buf, self._model_channels
    f32 = torch.float32
    rt = 1 if (index is not None or shared_t) else R
    emb = B_.get("temb_sin" + tag, (rt, mc), f32)
    if index is not None:
      ops.time_embedding(emb, mc, steps=steps, index=index)
    else:
      ops.time_embedding(emb, mc, t_rows=t_rows)
    th = B_.get("temb_h" + tag, (rt, 4 * mc), f32)
    ops.gemv(emb, self.time1[0], self.time1[1], th, act_out=ops.ACT_SILU)
    temb = B_.get("temb" + tag, (rt, 4 * mc), f32)
    ops.gemv(th, self.time2[0], self.time2[1], temb)
    tall = B_.get("temb_all" + tag, (rt, self.temb_total), f32)
    ops.gemv(temb, self.temb_all[0], self.temb_all[1], tall, act_in=ops.ACT_SILU)
    return tall

  def __call__(self, inputs, time, context=None, y=None, training=False):
    """unet.py:118 contract: inputs [R,h,w,4], time int [R], context [R,T,D]."""
    if training:
      raise NotImplementedError("the HIP path is inference only")
    x = torch.as_tensor(inputs, dtype=torch.float32).to(self.device).contiguous()
    t = torch.as_tensor(time).to(torch.int32).to(self.device).contiguous()
    if context is not None:
      self.set_context(torch.as_tensor(context).to(self.device).contiguous())
    return self.forward(x, t_rows=t)
