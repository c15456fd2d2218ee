"""The captured-graph slots across latent shapes, on the GPU (DESIGN.md sections 14 and 17): a sampler that alternates
between two shapes finds every slot of a shape as it left it -- the same graph objects, the same bits -- while the other
shape's wait in _states; set_preview empties the preview slots of every shape and no other; an eager twin gives the
same bits and fills no slot.  Tiny models, ids and LDM are those of tests/test_img2img_gpu.py (N = 10), batch 2, the
latent shapes (2,16,16,4) and (2,8,8,4): the smallest at which state can cross between shapes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_img2img_gpu as T  # noqa: E402
from test_img2img_gpu import kl_w, txt_w, unet_w  # noqa: E402,F401  (fixtures)

A, B_ = (2, 16, 16, 4), (2, 8, 8, 4)
GS, Q, SCALE, INTERVAL = 5., 3, 2, (300, 700)
PROJ = (0.3 * np.random.default_rng(17).standard_normal((5, 3))).astype(np.float32)
PROJ2 = (0.3 * np.random.default_rng(18).standard_normal((5, 3))).astype(np.float32)
# loop -> (its keywords, the slot it captures into)
LOOPS = {
    "plain": (dict(), "_graph"),
    "preview": (dict(preview_freq=Q), "_pv_graph"),
    "attn": (dict(attn_maps=True), "_am_graph"),
    "sched": (dict(guidance_interval=INTERVAL), "_sched_graphs"),
    "preview_sched": (dict(guidance_interval=INTERVAL, preview_freq=Q), "_pv_sched_graphs"),
}
SLOTS = ("_graph", "_sched_graphs", "_inv_graph", "_pv_graph", "_pv_sched_graphs", "_am_graph", "_dm_graph",
         "_invt_graph", "_de_graph")
BY_FORM = ("_sched_graphs", "_pv_sched_graphs")


def _visit(s, shape):
  """Every loop once at `shape`: {loop: images}."""
  ids = T._ids()
  return {name: s.ddim_p_sample_loop(ids, list(shape), GS, seed=3, **kw).clone() for name, (kw, _) in LOOPS.items()}


def _slots(state):
  """{slot: its graph, or a copy of its dict of graphs} of the sampler or of a parked shape's dict."""
  get = state.get if isinstance(state, dict) else lambda n: getattr(state, n)
  return {n: dict(get(n)) if n in BY_FORM else get(n) for n in SLOTS}


def _same(got, want):
  if isinstance(want, dict):
    return got.keys() == want.keys() and all(got[f] is want[f] for f in want)
  return got is want


def _check_slots(got, want, names=SLOTS):
  for n in names:
    assert _same(got[n], want[n]), n


@pytest.fixture(scope="module")
def run(dev, unet_w, txt_w, kl_w):
  s = T._sampler(dev, torch.float32, unet_w, txt_w, kl_w)
  s.set_preview(PROJ, scale=SCALE, mode="bilinear")
  out = dict(s=s)
  out["images_a"], out["slots_a"] = _visit(s, A), _slots(s)
  out["images_b"], out["slots_b"] = _visit(s, B_), _slots(s)
  return out


def test_every_loop_filled_its_own_slot(run):
  for shape, slots in ((A, run["slots_a"]), (B_, run["slots_b"])):
    for name, (_, slot) in LOOPS.items():
      if slot in BY_FORM:                                       # the interval takes both forms at N = 10
        assert set(slots[slot]) == {True, False}, (shape, name)
      else:
        assert slots[slot] is not None, (shape, name)
    assert all(slots[n] is None for n in ("_inv_graph", "_dm_graph", "_invt_graph", "_de_graph"))
  graphs = lambda slots: [g for n in SLOTS for g in (slots[n].values() if n in BY_FORM else [slots[n]]) if g is not None]
  a, b = graphs(run["slots_a"]), graphs(run["slots_b"])
  assert len(a) == 7 and len(b) == 7 and len({id(g) for g in a + b}) == 14      # a graph per loop, form and shape
  assert tuple(run["images_a"]["plain"].shape) == (2, 128, 128, 3)
  assert tuple(run["images_b"]["plain"].shape) == (2, 64, 64, 3)


def test_a_shape_finds_its_slots_and_its_bits_again(run):
  s = run["s"]
  s.ddim_p_sample_loop(T._ids(), list(B_), GS, seed=3)            # (on B, whatever ran before)
  assert s._state_key == B_ and set(s._states) == {A}
  _check_slots(_slots(s._states[A]), run["slots_a"])
  again_a = _visit(s, A)                                          # back on A: nothing is captured
  assert s._state_key == A and set(s._states) == {B_}
  _check_slots(_slots(s), run["slots_a"])
  _check_slots(_slots(s._states[B_]), run["slots_b"])
  for name in LOOPS:
    assert torch.equal(again_a[name], run["images_a"][name]), name
  again_b = _visit(s, B_)
  _check_slots(_slots(s), run["slots_b"])
  _check_slots(_slots(s._states[A]), run["slots_a"])
  for name in LOOPS:
    assert torch.equal(again_b[name], run["images_b"][name]), name


def test_an_eager_twin_gives_the_same_bits_and_fills_no_slot(dev, run, unet_w, txt_w, kl_w):
  e = T._sampler(dev, torch.float32, unet_w, txt_w, kl_w, use_graph=False)
  e.set_preview(PROJ, scale=SCALE, mode="bilinear")
  for shape, want in ((A, run["images_a"]), (B_, run["images_b"])):
    got = _visit(e, shape)
    for name in LOOPS:
      assert torch.equal(got[name], want[name]), (shape, name)
  for state in (e, e._states[A]):
    assert all(v == ({} if n in BY_FORM else None) for n, v in _slots(state).items())


def test_set_preview_empties_the_preview_slots_of_every_shape_and_no_other(run):
  s, ids = run["s"], T._ids()
  s.ddim_p_sample_loop(ids, list(A), GS, seed=3)                  # (on A, whatever ran before)
  assert s._state_key == A and set(s._states) == {B_}
  s.set_preview(PROJ, scale=SCALE, mode="bilinear")               # the same three: nothing changes
  _check_slots(_slots(s), run["slots_a"])
  s.set_preview(PROJ2, scale=SCALE, mode="bilinear")
  others = [n for n in SLOTS if n not in ("_pv_graph", "_pv_sched_graphs")]
  for state, first in ((s, run["slots_a"]), (s._states[B_], run["slots_b"])):
    now = _slots(state)
    assert now["_pv_graph"] is None and now["_pv_sched_graphs"] == {}
    _check_slots(now, first, others)
  # the next preview loops recapture, on either shape; the plain loop finds its graph and gives its bits
  for shape, first, images in ((A, run["slots_a"], run["images_a"]), (B_, run["slots_b"], run["images_b"])):
    pv = s.ddim_p_sample_loop(ids, list(shape), GS, seed=3, preview_freq=Q)
    assert s._pv_graph is not None and s._pv_graph is not first["_pv_graph"] and s._pv_sched_graphs == {}
    assert torch.equal(pv, images["preview"])                     # (the matrix colours the strips, not the latents)
    plain = s.ddim_p_sample_loop(ids, list(shape), GS, seed=3)
    assert torch.equal(plain, images["plain"])
    _check_slots(_slots(s), first, others)
