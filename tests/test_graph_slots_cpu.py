"""The sampler's captured-graph slots (DESIGN.md sections 14 and 17): the table that declares them and everything
derived from it -- the defaults of a fresh sampler, what travels with a latent shape, what a new buffer address drops
and what the clear-helper empties, here and in the parked shapes.  The nine names are written out below on purpose: a
table that loses one fails here.  No device: a sampler built without models, sentinel objects for graphs."""
import numpy as np

from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler

LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012, v_posterior=0., scale_factor=0.18215, eta=0.,
           num_ddim_steps=10)
# attribute -> (its key's attribute, whether it holds a dict of graphs by form)
SLOTS = {
    "_graph": ("_graph_key", False),
    "_sched_graphs": ("_sched_key", True),
    "_inv_graph": ("_inv_graph_key", False),
    "_pv_graph": ("_pv_graph_key", False),
    "_pv_sched_graphs": ("_pv_sched_key", True),
    "_am_graph": ("_am_graph_key", False),
    "_dm_graph": ("_dm_graph_key", False),
    "_invt_graph": ("_invt_graph_key", False),
    "_de_graph": ("_de_graph_key", False),
}


def _sampler():
  return LatentDiffusionModelSampler(None, None, None, verbose=False, **LDM)


def _empty(by_form):
  return {} if by_form else None


def _fill(target, set_value, tag):
  """A sentinel in every slot and key of `target`; returns {attribute: sentinel}."""
  put = {}
  for name, (key, by_form) in SLOTS.items():
    g = object()
    put[name] = {True: g} if by_form else g
    put[key] = (tag, name)
    set_value(target, name, put[name])
    set_value(target, key, put[key])
  return put


def test_a_fresh_sampler_has_every_slot_empty():
  s = _sampler()
  assert len(SLOTS) == 9
  for name, (key, by_form) in SLOTS.items():
    assert name in vars(s) and key in vars(s), name             # plain instance attributes
    got = getattr(s, name)
    assert got == {} if by_form else got is None, name
    assert getattr(s, key) is None, key
  assert s._states == {} and s._state_key is None
  assert not hasattr(s, "_xt") and not hasattr(s, "_ring") and not hasattr(s, "_win_key")
  dicts = [getattr(s, name) for name, (_, by_form) in SLOTS.items() if by_form]
  assert dicts[0] is not dicts[1]                               # (no shared default)
  assert _sampler()._sched_graphs is not s._sched_graphs


def test_shape_graphs_are_exactly_the_slots_and_their_keys():
  want = set(SLOTS) | {key for key, _ in SLOTS.values()}
  got = LatentDiffusionModelSampler._SHAPE_GRAPHS
  assert len(want) == 18 and len(got) == 18 and set(got) == want
  assert not set(got) & set(LatentDiffusionModelSampler._SHAPE_BUFFERS)


def test_drop_graphs_empties_every_slot_and_keeps_the_keys():
  s = _sampler()
  put = _fill(s, setattr, "cur")
  parked = {}
  s._states[(2, 8, 8, 4)] = parked
  kept = _fill(parked, dict.__setitem__, "parked")
  s._drop_graphs()
  for name, (key, by_form) in SLOTS.items():
    assert getattr(s, name) == _empty(by_form) and type(getattr(s, name)) is type(_empty(by_form)), name
    assert getattr(s, key) == put[key], key                     # (a key without a graph matches nothing)
  assert parked == kept and all(parked[n] is kept[n] for n in kept)   # the current shape's only


def test_the_table_declares_the_nine_slots():
  table = LatentDiffusionModelSampler._GRAPH_SLOTS
  assert len(table) == 9 and dict(table) == SLOTS
  assert list(LatentDiffusionModelSampler._SHAPE_GRAPHS[:9]) == list(table)


def test_clear_slots_here_and_in_every_parked_shape():
  s = _sampler()
  _fill(s, setattr, "cur")
  a, b = {}, {}
  s._states[(2, 8, 8, 4)], s._states[(2, 16, 16, 4)] = a, b
  kept_a, kept_b = _fill(a, dict.__setitem__, "a"), _fill(b, dict.__setitem__, "b")
  a["_xt"] = b["_xt"] = xt = object()
  cur = {n: getattr(s, n) for n in kept_a}
  # the current shape only
  s._clear_slots("_pv_graph", "_pv_sched_graphs")
  assert s._pv_graph is None and s._pv_sched_graphs == {}
  for n in cur:
    if n not in ("_pv_graph", "_pv_sched_graphs"):
      assert getattr(s, n) is cur[n], n                         # every other slot and every key, the cleared ones' too
  assert a == dict(kept_a, _xt=xt) and b == dict(kept_b, _xt=xt)
  # every shape
  s._clear_slots("_am_graph", "_sched_graphs", all_shapes=True)
  assert s._am_graph is None and s._sched_graphs == {}
  assert s._graph is cur["_graph"] and s._de_graph is cur["_de_graph"] and s._am_graph_key == cur["_am_graph_key"]
  for saved, kept in ((a, kept_a), (b, kept_b)):
    assert saved["_am_graph"] is None and saved["_sched_graphs"] == {}
    assert saved["_sched_graphs"] is not s._sched_graphs
    for n in kept:
      if n not in ("_am_graph", "_sched_graphs"):
        assert saved[n] is kept[n], n
    assert saved["_xt"] is xt and set(saved) == set(kept) | {"_xt"}
  assert a["_sched_graphs"] is not b["_sched_graphs"]
  # a name that is no slot is an error, not a new attribute
  try:
    s._clear_slots("_pv_grap")
  except KeyError:
    pass
  else:
    raise AssertionError("_clear_slots took a name that is no slot")
  assert not hasattr(s, "_pv_grap")


def test_a_fresh_shape_resets_the_keys_and_a_parked_one_keeps_them():
  """_alloc_state's bookkeeping without its allocations: torch.empty on the CPU stands in for the device."""
  import torch
  s = _sampler()
  s.device = torch.device("cpu")
  A, Bs = (2, 16, 16, 4), (2, 8, 8, 4)
  s._alloc_state(*A)
  put_a = _fill(s, setattr, "a")
  s._alloc_state(*Bs)                                           # a fresh shape: nothing of A's is visible
  for name, (key, by_form) in SLOTS.items():
    assert getattr(s, name) == _empty(by_form) and getattr(s, key) is None, name
  assert all(s._states[A][n] is put_a[n] for n in put_a) and tuple(s._xt.shape) == Bs
  put_b = _fill(s, setattr, "b")
  s._alloc_state(*A)                                            # seen before: as it was left
  assert all(getattr(s, n) is put_a[n] for n in put_a) and tuple(s._xt.shape) == A
  assert all(s._states[Bs][n] is put_b[n] for n in put_b) and A not in s._states
  assert np.array_equal(sorted(s._states), [Bs])
