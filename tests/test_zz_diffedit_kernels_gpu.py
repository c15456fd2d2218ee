"""DiffEdit's three kernels on the GPU, all through the C ABI: ldm_eps_contrast_accum bit for bit
against the float32 restatement (tests/diffedit_ref.py), ldm_contrast_mask on exact probes and on random inputs whose
band is empty, ldm_store_row as the inverse of ldm_select_row -- every element accounted for, canaries around every
output, the rejections, and the device counter under a captured graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diffedit_ref as DR  # noqa: E402
from ldm_tf2_amd import ops  # noqa: E402
from ldm_tf2_amd._lib import LdmHipError  # noqa: E402

CANARY = -12288.
PAD = 64                                       # floats around every output (a multiple of 4: the views stay aligned)


def _padded(dev, numel, dtype=torch.float32, fill=CANARY):
  buf = torch.full((numel + 2 * PAD,), fill, dtype=dtype, device=dev)
  return buf, buf[PAD:PAD + numel]


def _clean(buf, fill=CANARY):
  return bool((buf[:PAD] == fill).all() and (buf[-PAD:] == fill).all())


# ---- ldm_eps_contrast_accum ---------------------------------------------------------------------------------
ACCUM_SHAPES = [(1, 1, 4), (2, 1023, 4), (3, 256, 3), (2, 37, 1), (1, 5, 16), (5, 1 << 20, 4)]


@pytest.mark.parametrize("shape", ACCUM_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_accum_equals_the_float32_restatement(dev, shape):
  B, cells, c = shape
  g = torch.Generator().manual_seed(11)
  eps = torch.randn(2 * B, cells, c, generator=g)
  eps2 = torch.randn(2 * B, cells, c, generator=g)
  start = torch.rand(B, cells, generator=g)
  buf, acc = _padded(dev, B * cells)
  acc = acc.view(B, cells)
  acc.copy_(start)
  counter = torch.tensor([7], dtype=torch.int32, device=dev)
  ops.eps_contrast_accum(eps.to(dev), acc, counter=counter)
  want = DR.contrast_accum(start.numpy(), eps[:B].numpy(), eps[B:].numpy())
  assert torch.equal(acc.cpu(), torch.from_numpy(want)) and _clean(buf)     # every cell once, nothing outside
  assert counter.item() == 6
  # a second launch accumulates on top; without a counter nothing else moves
  ops.eps_contrast_accum(eps2.to(dev), acc)
  want = DR.contrast_accum(want, eps2[:B].numpy(), eps2[B:].numpy())
  assert torch.equal(acc.cpu(), torch.from_numpy(want)) and _clean(buf) and counter.item() == 6
  ops.eps_contrast_accum(eps2.to(dev), acc, counter=counter)
  assert counter.item() == 5


@pytest.mark.parametrize("shape", [(2, 1023, 4), (3, 256, 3)], ids=["c4", "c3"])
def test_accum_nan_reaches_its_own_cell_only(dev, shape):
  B, cells, c = shape
  g = torch.Generator().manual_seed(12)
  eps = torch.randn(2 * B, cells, c, generator=g)
  hits = [(0, 0, 0), (B - 1, cells - 1, c - 1), (0, cells - 2, 1), (B - 1, 513 % cells, 0)]
  for n, (b, p, j) in enumerate(hits):
    eps[b + (B if n % 2 else 0), p, j] = float("nan")                     # either half
  acc = torch.zeros(B, cells, device=dev)
  ops.eps_contrast_accum(eps.to(dev), acc)
  nan = torch.isnan(acc.cpu())
  want = torch.zeros(B, cells, dtype=torch.bool)
  for b, p, _ in hits:
    want[b, p] = True
  assert torch.equal(nan, want)
  ref = DR.contrast_accum(np.zeros((B, cells), np.float32), eps[:B].numpy(), eps[B:].numpy())
  assert torch.equal(acc.cpu()[~want], torch.from_numpy(ref)[~want])


def test_accum_rejections(dev):
  z = lambda *s: torch.zeros(*s, device=dev)
  off = lambda numel, *s: z(numel + 4)[1:1 + numel].view(*s)              # 4 bytes off a 16-byte boundary
  with pytest.raises(LdmHipError, match="16-byte aligned"):
    ops.eps_contrast_accum(off(64, 4, 4, 4), z(2, 4))
  with pytest.raises(LdmHipError, match="16-byte aligned"):
    ops.eps_contrast_accum(z(4, 4, 4), off(8, 2, 4))
  acc = off(8, 2, 4)
  ops.eps_contrast_accum(off(48, 4, 4, 3), acc)                           # c = 3: the scalar path takes any float pointer
  assert (acc == 0).all()
  with pytest.raises(LdmHipError, match="null pointer"):
    ops.check(ops.lib.ldm_eps_contrast_accum(None, None, None, 1, 4, 4, None), "ldm_eps_contrast_accum")
  e, a = z(2, 4, 4), z(1, 4)
  for B, cells, c in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, 17)):
    with pytest.raises(LdmHipError, match="bad args"):
      ops.check(ops.lib.ldm_eps_contrast_accum(e.data_ptr(), a.data_ptr(), None, B, cells, c, None),
                "ldm_eps_contrast_accum")
  torch.cuda.synchronize()
  assert (a == 0).all()


# ---- ldm_contrast_mask -----------------------------------------------------------------------------------------
def _run_mask(dev, acc, tau, r, outputs=True):
  B, h, w = acc.shape
  (bm, mask), (be, mean), (bt, thr) = _padded(dev, B * h * w), _padded(dev, B), _padded(dev, B)
  bc, count = _padded(dev, B, torch.int32, fill=-77)
  opt = dict(mean_out=mean, thr_out=thr, count_out=count) if outputs else {}
  ops.contrast_mask(torch.from_numpy(acc).to(dev), mask.view(B, h, w), tau, r, **opt)
  assert _clean(bm) and _clean(be) and _clean(bt) and _clean(bc, -77)
  if not outputs:
    assert (mean == CANARY).all() and (thr == CANARY).all() and (count == -77).all()
  return mask.view(B, h, w).cpu().numpy(), mean.cpu().numpy(), thr.cpu().numpy(), count.cpu().numpy()


def _exact_probe(tiles):
  """[3,16,16 * tiles]: per sample a 16 x 16 tile `tiles` times side by side.  Sample 0's tile holds small integers
  times 2^-4, all at least 1, with the sum 512, so that the sum, the mean 2 and the threshold 3 at tau = 1.5 are exact
  in any order: five cells exactly at the threshold (kept), ten and the two outer corners at 5 (edited), the rest
  below.  In its first tile one of the five is one ulp above the threshold (edited): that cell's extra 2^-22 is at most
  half an ulp of any sum from 4 on and is rounded away (the tie goes to even) by the first addition it meets, every
  other cell being at least 1.  Sample 1 is all zeros, sample 2 all 2: neither edits anything.  Returns the maps and
  the raised cell."""
  rest = np.concatenate([np.full(5, 3.), np.full(10, 5.), [2. + 2. ** -4, 2. - 2. ** -4], np.full(196, 2.),
                         np.full(41, 1.)])
  tile = np.empty(256)
  tile[[0, 255]] = 5.                                                       # the corners (0, 0) and (15, 15)
  tile[1:255] = np.random.default_rng(50).permutation(rest)
  assert tile.sum() == 512. and tile.min() >= 1.
  tile = tile.astype(np.float32).reshape(16, 16)
  a = np.tile(tile, (1, tiles))
  acc = np.stack([a, np.zeros_like(a), np.full_like(a, 2.)])
  y, x = (int(v) for v in np.argwhere(tile == 3.)[0])
  acc[0, y, x] = np.nextafter(np.float32(3.), np.float32(4.))
  return acc, (y, x)


@pytest.mark.parametrize("tiles", [1, 16], ids=["16x16", "16x256"])
@pytest.mark.parametrize("r", [0, 1, 3])
def test_mask_exact_probes(dev, tiles, r):
  acc, (y, x) = _exact_probe(tiles)
  n = acc[0].size
  ref = DR.contrast_mask(acc, 1.5, r)
  assert ref["mean"].tolist() == [2., 0., 2.] and ref["thr"].tolist() == [3., 0., 3.]
  plain = DR.contrast_mask(acc, 1.5, 0)
  at = acc[0] == 3.
  assert plain["mask"][0, y, x] == 0. and at.sum() == 5 * tiles - 1 and (plain["mask"][0][at] == 1.).all()
  assert plain["edited"].tolist() == [12 * tiles + 1, 0, 0]
  assert plain["mask"][0, 0, 0] == 0. and plain["mask"][0, 15, 16 * tiles - 1] == 0.          # edits in two corners
  mask, mean, thr, count = _run_mask(dev, acc, 1.5, r)
  assert mean.tobytes() == ref["mean"].tobytes() and thr.tobytes() == ref["thr"].tobytes()
  assert np.array_equal(mask, ref["mask"]) and mask.dtype == np.float32 and set(np.unique(mask)) <= {0., 1.}
  assert np.array_equal(count, ref["edited"]) and count[1] == 0 and count[2] == 0
  assert n - count[0] == int(mask[0].sum())


@pytest.mark.parametrize("case", DR.MASK_CASES, ids=lambda c: "x".join(str(v) for v in c[:3]))
def test_mask_random_inputs(dev, case):
  h, w, r, _ = case
  acc = DR.mask_case_acc(case)
  assert not DR.band(acc, DR.MASK_TAU)[[0, 2]].any()                        # (sample 1 is all zeros: exact in any order)
  ref = DR.contrast_mask(acc, DR.MASK_TAU, r)
  mask, mean, thr, count = _run_mask(dev, acc, DR.MASK_TAU, r)
  assert np.array_equal(mask, ref["mask"]) and np.array_equal(count, ref["edited"])
  rel = np.abs(mean.astype(np.float64)[[0, 2]] - ref["mean64"][[0, 2]]) / ref["mean64"][[0, 2]]
  print(f"{h}x{w}: mean rel err {rel.max():.3e} (bound {h * w * 2.0 ** -24:.3e}); edited {count.tolist()}")
  assert (rel <= h * w * 2. ** -24).all() and mean[1] == 0. and thr[1] == 0.
  assert np.array_equal(thr, (np.float32(DR.MASK_TAU) * mean).astype(np.float32))
  # two runs give identical bits; the optional outputs may be left out
  again = _run_mask(dev, acc, DR.MASK_TAU, r)
  assert all(a.tobytes() == b.tobytes() for a, b in zip((mask, mean, thr, count), again))
  assert np.array_equal(_run_mask(dev, acc, DR.MASK_TAU, r, outputs=False)[0], mask)


def test_mask_single_cell_and_nan(dev):
  one = np.full((2, 1, 1), 3., np.float32)
  for tau, edited in ((0.5, 1), (1., 0), (1.5, 0)):                         # a cell is its own mean
    mask, mean, thr, count = _run_mask(dev, one, tau, 0)
    assert count.tolist() == [edited] * 2 and mask.ravel().tolist() == [1. - edited] * 2 and mean.tolist() == [3., 3.]
  acc = DR.random_acc(2, 5, 7, 46)
  acc[1, 2, 3] = np.nan
  mask, mean, thr, count = _run_mask(dev, acc, 1.5, 1)
  ref = DR.contrast_mask(acc, 1.5, 1)
  assert np.isnan(mean[1]) and np.isnan(thr[1]) and count[1] == 0 and (mask[1] == 1.).all()
  assert np.array_equal(mask, ref["mask"]) and count[0] == ref["edited"][0] > 0


def test_mask_rejections(dev):
  z = lambda *s: torch.zeros(*s, device=dev)
  assert ops.contrast_mask_supported(8, 8192, 3) and not ops.contrast_mask_supported(1, 65537)
  with pytest.raises(LdmHipError, match="ldm_contrast_mask_supported"):
    ops.contrast_mask(z(1, 1, 65537), z(1, 1, 65537), 1.5)                  # one cell more
  with pytest.raises(LdmHipError, match="ldm_contrast_mask_supported"):
    ops.contrast_mask(z(1, 4, 4), z(1, 4, 4), 1.5, 4)
  with pytest.raises(LdmHipError, match="ldm_contrast_mask_supported"):
    ops.contrast_mask(z(1, 4, 4), z(1, 4, 4), 1.5, -1)
  with pytest.raises(LdmHipError, match="null pointer"):
    ops.check(ops.lib.ldm_contrast_mask(None, None, None, None, None, 1, 4, 4, 1.5, 0, None), "ldm_contrast_mask")
  a = z(1, 4, 4)
  with pytest.raises(LdmHipError, match="bad args"):
    ops.check(ops.lib.ldm_contrast_mask(a.data_ptr(), a.data_ptr(), None, None, None, 0, 4, 4, 1.5, 0, None),
              "ldm_contrast_mask")


# ---- ldm_store_row ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 2048, 5 * (1 << 18)], ids=["4", "2048", "5x2^18"])
def test_store_row_is_the_inverse_of_select_row(dev, n):
  rows = 3 if n > 4096 else 6
  g = torch.Generator().manual_seed(13)
  src = torch.randn(n, generator=g).to(dev)
  index = torch.zeros(1, dtype=torch.int32, device=dev)
  for sign, bias, idx, row in ((1, 0, 2, 2), (1, -1, 1, 0), (-1, rows - 1, 0, rows - 1), (-1, rows - 1, rows - 1, 0),
                               (-1, rows - 2, 1, rows - 3)):
    buf, t = _padded(dev, rows * n)
    table = t.view(rows, n)
    index.fill_(idx)
    ops.store_row(src, table, index, index_sign=sign, index_bias=bias)
    assert torch.equal(table[row], src) and _clean(buf) and index.item() == idx
    rest = torch.ones(rows, dtype=torch.bool)
    rest[row] = False
    assert (table[rest.to(dev)] == CANARY).all()
    if n % 4 == 0 and n <= 4096:                                            # select_row reads it back
      out = torch.empty(1, n, device=dev)
      index.fill_(row)
      ops.select_row(table, index, out)
      assert torch.equal(out[0], src)
  # an out-of-range row writes nothing
  for sign, bias, idx in ((1, 0, rows), (1, 0, -1), (-1, rows - 1, rows), (-1, rows - 1, -1), (1, 1 << 30, 1 << 30)):
    buf, t = _padded(dev, rows * n)
    index.fill_(idx)
    ops.store_row(src, t.view(rows, n), index, index_sign=sign, index_bias=bias)
    assert (buf == CANARY).all()


def test_store_row_rejections(dev):
  z = lambda *s: torch.zeros(*s, device=dev)
  i = torch.zeros(1, dtype=torch.int32, device=dev)
  with pytest.raises(LdmHipError, match="multiple of 4"):
    ops.store_row(z(6), z(2, 6), i)
  with pytest.raises(LdmHipError, match="16-byte aligned"):
    ops.store_row(z(12)[1:9], z(2, 8), i)
  with pytest.raises(LdmHipError, match="16-byte aligned"):
    ops.store_row(z(8), z(20)[1:17].view(2, 8), i)
  with pytest.raises(LdmHipError, match="index_sign"):
    ops.store_row(z(8), z(2, 8), i, index_sign=2)
  with pytest.raises(LdmHipError, match="null pointer"):
    ops.check(ops.lib.ldm_store_row(None, None, 8, 2, None, 1, 0, 8, None), "ldm_store_row")


def test_store_row_and_the_counter_under_a_captured_graph(dev):
  """The launches of a captured inversion step that keeps its trajectory, in miniature: the row comes from a counter
  that a later launch of the same graph moves (here ldm_eps_contrast_accum's decrement)."""
  rows, n = 5, 64
  src = torch.zeros(n, device=dev)
  buf, t = _padded(dev, rows * n)
  table = t.view(rows, n)
  eps, acc = torch.ones(2, 16, 4, device=dev), torch.zeros(1, 16, device=dev)
  eps[1] = 3.
  index = torch.tensor([rows - 1], dtype=torch.int32, device=dev)

  def step():
    ops.store_row(src, table, index, index_sign=-1, index_bias=rows - 1)
    ops.eps_contrast_accum(eps, acc, counter=index)

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    step()
  torch.cuda.current_stream().wait_stream(s)
  torch.cuda.synchronize()
  t.fill_(CANARY)
  acc.zero_()
  index.fill_(rows - 1)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, capture_error_mode="thread_local"):
    step()
  for j in range(rows + 2):                    # two replays past the table: their rows are out of range
    src.fill_(float(j + 1))
    g.replay()
  torch.cuda.synchronize()
  assert index.item() == -3 and _clean(buf)
  assert torch.equal(table, torch.arange(1, rows + 1, device=dev, dtype=torch.float32)[:, None].expand(rows, n))
  assert (acc == 8. * (rows + 2)).all()
