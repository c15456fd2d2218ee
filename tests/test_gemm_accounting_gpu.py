"""Every tap, pixel and K element of every ldm_gemm form accounted for, with integer inputs whose correct output is known
exactly (tests/gemm_probes.py: census and selection).  The gate of every case is torch.equal: there is no tolerance.

Forms: every tile index ldm_gemm accepts (0 = the cost model's pick, 1-19), float32 and bf16 where the tile has both, the
persistent tiles with one workgroup per panel and with the default deal; plain rows, the 3x3 convolution at stride 1 / 2
/ 2 without lead pad and over the 2x-upsampled image, the halo-staged tiles, the second A operand, split-K with both
reduce kernels and the deferred reduce, batched and transposed stores, the second output; all through ops.linear,
ops.conv3x3, ops.bmm_nt and ops.linear_t.  Sizes sit on each form's own tile, ring and image edges (G.all_cases()).

Operands are views of NaN-filled buffers (row pitches, channel slices, pad rows): a read outside the operand poisons
the output, and every output buffer must still be NaN outside the [M, N] region the launch owns.  Non-square and odd
images are covered here (tests/test_bench_shapes_gpu.py runs square power-of-two images only).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_probes as G  # noqa: E402

NAN = float("nan")
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def ops():
  from ldm_tf2_amd import ops as _ops
  return _ops


@pytest.fixture()
def spy(monkeypatch):
  """Records the (tile, split) plan and the slab count of every ldm_gemm launch made through ops."""
  o = ops()
  from ldm_tf2_amd._lib import lib
  seen = []

  def wrap(orig):
    def f(p, device, *rest):
      r = orig(p, device, *rest)
      t, s = C.c_int(), C.c_int()
      assert lib.ldm_gemm_plan(C.byref(p), C.byref(t), C.byref(s)) == 0
      seen.append((t.value, s.value, lib.ldm_gemm_splits(C.byref(p))))
      return r
    return f

  monkeypatch.setattr(o, "_gemm", wrap(o._gemm))
  monkeypatch.setattr(o, "_gemm_deferred", wrap(o._gemm_deferred))
  return seen


def put(x, dtype, dev):
  return x.to(F64).to(dtype).to(dev)


def padded(mat, extra, dtype, dev):
  """mat [R, C] as a view of a NaN-filled [R + 1, C + extra] device buffer."""
  R, Cc = mat.shape
  buf = torch.full((R + 1, Cc + extra), NAN, dtype=F64)
  buf[:R, :Cc] = mat.to(F64)
  return buf.to(dtype).to(dev)[:R, :Cc]


def out_rows(rows, cols, extra, off8, dtype, dev):
  """([rows, cols] view with row pitch cols + extra, the NaN-filled flat buffer behind it); off8: the view starts 8
  bytes behind a 16-byte boundary."""
  ld = cols + extra
  off = (4 if dtype == BF else 2) if off8 else 0
  flat = torch.full(((rows + 2) * ld + 16,), NAN, dtype=dtype, device=dev)
  return flat[off:off + (rows + 2) * ld].view(rows + 2, ld)[:rows, :cols], flat


def take(view, flat):
  """The values of `view` as float64 on the host; everything else in `flat` must still be NaN."""
  torch.cuda.synchronize()
  got = view.detach().cpu().to(F64)
  view.fill_(NAN)
  assert bool(torch.isnan(flat).all()), "the launch wrote outside its [M, N] output region"
  return got


def bias_of(c, d, dev):
  """The bias on the device; c.boff: a slice that starts 4 bytes behind a 16-byte boundary of a NaN-filled buffer."""
  if not c.boff:
    return d["bias"].to(F32).to(dev)
  buf = torch.full((c.N + 8,), NAN, dtype=F32)
  buf[1:1 + c.N] = d["bias"].to(F32)
  return buf.to(dev)[1:1 + c.N]


def run(dev, c, d, hold=None):
  """The product of case `c` on data `d` as float64 [Bt, M, N] (N / 2 columns with GEGLU).  `hold`: a list that
  receives (view, flat) of the output before the launch, for a caller that expects the launch to be rejected."""
  o, f = ops(), G.FORMS[c.form]
  dt, odt = f.dt, c.odt
  K1 = c.K - c.K2
  kw = {}
  nout = G.nout_of(c)
  if c.bias:
    kw["bias"] = bias_of(c, d, dev)
  if c.kind == "tstore":
    # the transposed store under an activation: the C ABI permits it, ops.bmm_nt passes no act
    from ldm_tf2_amd._lib import GemmParams
    a = padded(d["a"][0], 0, dt, dev)
    wd = put(d["w"][0], dt, dev).contiguous()
    ldn = (c.M + 7) // 8 * 8 + 8
    flat = torch.full((c.N, ldn), NAN, dtype=odt, device=dev)
    if hold is not None:
      hold.append((flat[:, :c.M], flat))
    p = GemmParams()
    p.a, p.w, p.out, p.bias = o._ptr(a), o._ptr(wd), o._ptr(flat), o._ptr(kw.get("bias"))
    p.lda, p.ldc_m, p.ldc_n = a.stride(0), 1, ldn
    p.M, p.N, p.K, p.batch = c.M, c.N, c.K, 1
    p.act, p.dtype, p.out_dtype, p.alpha = G.ACT_CODES[c.act], o.code(dt), o.code(odt), c.alpha
    p.tile = f.tile
    o._gemm(p, dev)
    return take(flat[:, :c.M], flat).t().reshape(1, c.M, c.N)
  w = d["w"]
  if c.kind == "bmm":
    ab = torch.full((c.Bt, c.M + 1, c.K), NAN, dtype=F64)
    ab[:, :c.M] = d["a"].to(F64)
    a = ab.to(dt).to(dev)[:, :c.M]
    wd = put(w[0] if c.shared_w else w, dt, dev).contiguous()
    if c.trans:
      ldn = (c.M + 7) // 8 * 8 + 8
      flat = torch.full((c.Bt, c.N, ldn), NAN, dtype=odt, device=dev)
      o.bmm_nt(a, wd, flat, alpha=c.alpha, transposed_out=True, tile=f.tile, **kw)
      return take(flat[:, :, :c.M], flat).permute(0, 2, 1).contiguous()
    flat = torch.full((c.Bt, c.M + 1, c.N + 8), NAN, dtype=odt, device=dev)
    o.bmm_nt(a, wd, flat[:, :c.M, :c.N], alpha=c.alpha, tile=f.tile, **kw)
    return take(flat[:, :c.M, :c.N], flat)

  wd = put(w[0], dt, dev).contiguous()
  if c.addend:
    kw["addend"] = d["addend"].to(F32).to(dev)
  res2d = put(d["res"], odt, dev)[:, :nout] if c.res else None
  x2 = padded(d["a2"], c.lda2_x, dt, dev) if c.K2 else None
  split = c.split if f.tile else 0
  if c.kind == "conv":
    _, _, oh, ow = G.conv_dims(c)
    if c.in_slice:
      wide = torch.full((c.B, c.H, c.W, c.Cin + 72), NAN, dtype=F64)
      wide[..., 64:64 + c.Cin] = d["a"].to(F64)
      x = wide.to(dt).to(dev)[..., 64:64 + c.Cin]
    else:
      x = put(d["a"], dt, dev)
    if c.out_slice:
      flat = torch.full((c.B, oh, ow, c.N + 24), NAN, dtype=odt, device=dev)
      out = flat[..., 8:8 + c.N]
    else:
      view, flat = out_rows(c.M, c.N, 0, 0, odt, dev)
      out = flat[:c.M * c.N].view(c.B, oh, ow, c.N)
    if c.res:
      kw["residual"] = res2d.reshape(c.B, oh, ow, c.N)
    if c.K2:
      kw["x2"] = x2.view(c.B, oh, ow, c.K2)
    if hold is not None:
      hold.append((out, flat))
    if c.act:                                                          # ops.conv3x3 passes no act: its parameters + act
      p = o._conv_params(x, wd, out, kw.get("bias"), c.stride, bool(c.up), kw.get("addend"), kw.get("residual"), f.tile,
                         split, bool(c.nlp))
      p.act = G.ACT_CODES[c.act]
      o._gemm(p, dev)
      return take(out, flat).reshape(1, c.M, c.N)
    r = o.conv3x3(x, wd, out, stride=c.stride, upsample=bool(c.up), no_lead_pad=bool(c.nlp), tile=f.tile, split_k=split,
                  defer_reduce=bool(c.defer), **kw)
    if c.defer:
      assert (r is not None) == (G.expected_slabs(c) > 1)
      o.finish(r)
    return take(out, flat).reshape(1, c.M, c.N)

  x = padded(d["a"][0], c.lda_x, dt, dev)
  if c.kind == "lint":
    T = c.M // c.G
    flat = torch.full((c.G, c.N, T + 8), NAN, dtype=odt, device=dev)
    assert o.linear_t_supported(x.view(c.G, T, K1), wd, flat)
    o.linear_t(x.view(c.G, T, K1), wd, flat, tile=f.tile)
    return take(flat[:, :, :T], flat).permute(0, 2, 1).reshape(1, c.M, c.N)
  if c.kind == "out2":
    ns, T = G.TILES[f.tile].bn, c.M // c.G
    qk, qflat = out_rows(c.M, ns, 0, 0, odt, dev)
    vt = torch.full((c.G, c.N - ns, T + 4), NAN, dtype=odt, device=dev)
    o.linear(x, wd, qk, out2=vt, tile=f.tile, split_k=split, **kw)
    g2 = take(vt[:, :, :T], vt).permute(0, 2, 1).reshape(c.M, c.N - ns)
    return torch.cat([take(qk, qflat), g2], 1).reshape(1, c.M, c.N)
  out, flat = out_rows(c.M, nout, c.ldc_x, c.off8, odt, dev)
  if hold is not None:
    hold.append((out, flat))
  if c.res:
    kw["residual"] = res2d
  if c.addend:
    kw["add_rows"] = c.add_rows
  if c.act:
    kw["act"] = G.ACT_CODES[c.act]
  if c.lnf:
    kw["ln_fold"] = (d["cs"].to(F32).to(dev), d["eps"])
  r = o.linear(x, wd, out, alpha=c.alpha, tile=f.tile, split_k=split, x2=x2, defer_reduce=bool(c.defer), **kw)
  if c.defer:
    assert (r is not None) == (G.expected_slabs(c) > 1)
    o.finish(r)
  return take(out, flat).reshape(1, c.M, nout)


def test_tile_table_matches_the_library(dev):
  """bm / bn of gemm_probes.TILES against ops._TILE_DIMS, and against ldm_gemm itself: a second output needs n_split to
  be a multiple of the forced tile's width, so n_split = bn is accepted and n_split = bn - 8 is rejected unlaunched."""
  o = ops()
  from ldm_tf2_amd._lib import LdmHipError
  for t, (bm, bn, _) in o._TILE_DIMS.items():
    assert (G.TILES[t].bm, G.TILES[t].bn) == (bm, bn), t
  assert set(o._TILE_DIMS) == set(G.TILES) - {5}
  for t, tile in G.TILES.items():
    if t in G.PERSISTENT + G.HALO:
      continue
    x = torch.zeros(8, 64, dtype=BF, device=dev)
    w = torch.zeros(tile.bn + 8, 64, dtype=BF, device=dev)
    with pytest.raises(LdmHipError):
      o.linear(x, w, torch.zeros(8, tile.bn - 8, dtype=BF, device=dev), out2=torch.zeros(1, 16, 8, dtype=BF, device=dev), tile=t)
    o.linear(x, w, torch.zeros(8, tile.bn, dtype=BF, device=dev), out2=torch.zeros(1, 8, 8, dtype=BF, device=dev), tile=t)
  torch.cuda.synchronize()


def test_wide_upsampled_image_is_rejected(dev):
  """The upsampled form packs the tap origin of the 2x image into 16 bits per axis: 2 W = 32768 does not fit.  The
  host check rejects it; nothing is launched."""
  o = ops()
  from ldm_tf2_amd._lib import LdmHipError
  x = torch.zeros(1, 1, 16384, 64, dtype=BF, device=dev)
  w = torch.zeros(8, 576, dtype=BF, device=dev)
  with pytest.raises(LdmHipError, match="upsample needs 2\\*H and 2\\*W below 32768"):
    o.conv3x3(x, w, torch.zeros(1, 2, 32768, 8, dtype=BF, device=dev), upsample=True)
  with pytest.raises(LdmHipError, match="upsample needs 2\\*H and 2\\*W below 32768"):
    o.conv3x3(x.view(1, 16384, 1, 64), w, torch.zeros(1, 32768, 2, 8, dtype=BF, device=dev), upsample=True, tile=14)


@pytest.mark.parametrize("c", G.all_cases(), ids=G.case_id)
def test_gemm_accounting(dev, spy, c):
  f = G.FORMS[c.form]
  d = G.probe_census(c)
  got = run(dev, c, d)
  assert len(spy) == 1
  tile, _, slabs = spy[0]
  if f.tile:
    assert tile == f.tile and slabs == G.expected_slabs(c), (G.case_id(c), spy[0])
  msg = G.first_difference(c, got, G.reference(c, d))
  if msg:
    print("CENSUS " + msg)
  failed = ["census: " + msg] if msg else []
  if c.sel:
    cs = G.as_selection(c)
    for ph in G.phases(cs):
      d1 = G.probe_selection(cs, ph)
      msg = G.first_difference(cs, run(dev, cs, d1), G.reference(cs, d1), ph, d1)
      if msg:
        print("SELECTION " + msg)
        failed.append(f"selection phase {ph}: " + msg)
  print(f"ACCT {G.case_id(c)} plan {spy[0]} {'FAILED' if failed else 'exact'}")
  assert not failed, "\n".join(failed)
