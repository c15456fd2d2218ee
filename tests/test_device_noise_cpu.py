"""Device noise source, host side: the generator's definition (tests/philox_ref.py) against
Philox4x32-10's published known answers, the stream words, the moments of the restated normals, the C ABI entries,
the constructor switch and the CLI key.  Nothing runs on a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import philox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "all_in_one_config.yaml")
LDM = dict(num_steps=1000, beta_start=0.00085, beta_end=0.012)
ENTRIES = ("ldm_philox_u32", "ldm_normal_fill", "ldm_q_sample_rng", "ldm_cfg_ddim_update_rng",
           "ldm_cfg_plms_update_rng")

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, result)
KATS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


class _FakeModel:
  device = torch.device("cpu")

  def __init__(self, **kwargs):
    self.kwargs = kwargs


def _sampler(**kw):
  from ldm_tf2_amd.model_runners import LatentDiffusionModelSampler
  return LatentDiffusionModelSampler(_FakeModel(), _FakeModel(), _FakeModel(), **dict(LDM, **kw))


# ---- the generator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kat", KATS, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(kat):
  counter, key, want = kat
  got = R.philox4x32_10([np.array([c]) for c in counter], key)
  assert tuple(int(w[0]) for w in got) == want, [hex(int(w[0])) for w in got]


def test_counter_layout_of_words():
  """words(): element e of sample b is word e & 3 of counter (e >> 2, first + b, stream, 0), key = the seed's halves."""
  w = R.words(0, 0, 0, 1, 16)
  assert tuple(int(x) for x in w[0, :4]) == KATS[0][2]
  seed = (0x299f31d0 << 32) | 0xa4093822
  w = R.words(seed, 0x85a308d3 - 1, 0x13198a2e, 2, 8)
  one = R.philox4x32_10([np.array([1]), np.array([0x85a308d3]), np.array([0x13198a2e]), np.array([0])],
                        (0xa4093822, 0x299f31d0))
  assert [int(x) for x in w[1, 4:8]] == [int(x[0]) for x in one]
  assert R.key_of(seed + (1 << 64)) == R.key_of(seed) == (0xa4093822, 0x299f31d0)     # the seed is taken mod 2^64
  assert R.key_of(-1) == (0xffffffff, 0xffffffff)


def test_uniform_map_and_the_bound_on_z():
  x = np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32)
  u = R.uniform(x, np.float64)
  assert u[0] == u[1] == 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24 and u[-1] == 1 - 2.0 ** -25
  assert (u > 0).all() and (u < 1).all()
  u32 = R.uniform(x, np.float32)
  assert u32.dtype == np.float32 and (u32 > 0).all() and (u32 <= 1).all()
  assert np.array_equal(u32[:4].astype(np.float64), u[:4])          # exact below 1/2
  assert abs(R.Z_MAX - 5.887) < 1e-3
  z = R.normals_from_words(np.array([0, 0, 0xffffffff, 0x40000000], dtype=np.uint32))
  assert abs(z[0] - R.Z_MAX) < 1e-12 and abs(z[1]) < 2e-6          # u0 smallest, angle 2 pi 2^-25


def test_header_constants_are_the_python_streams():
  from ldm_tf2_amd import model_runners as M
  assert (M.XT_STREAM, M.ETA_STREAM, M.ENCODE_STREAM, M.Q_STREAM) == (0, 1 << 29, 1 << 30, (1 << 30) + 1)
  assert (R.XT_STREAM, R.ETA_STREAM, R.ENCODE_STREAM, R.Q_STREAM) == (0, 1 << 29, 1 << 30, (1 << 30) + 1)
  src = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
  env = {}
  for name, expr in re.findall(r"#define\s+LDM_RNG_(\w+)_STREAM\s+(.+)", src):
    env[name] = eval(re.sub(r"(\d+)u", r"\1", expr))
  assert env == dict(XT=M.XT_STREAM, ETA=M.ETA_STREAM, ENCODE=M.ENCODE_STREAM, Q=M.Q_STREAM), env


def test_stream_words_are_pairwise_distinct():
  from ldm_tf2_amd import model_runners as M
  for n in (1, 10, 200, 1000):
    words = [M.XT_STREAM, M.ENCODE_STREAM] + [M.ETA_STREAM + i for i in range(n)] + [M.Q_STREAM + i for i in range(n)]
    assert len(set(words)) == 2 * n + 2 and all(0 <= w < 1 << 32 for w in words)
  # ... and for any DDIM index below 2^29
  top = (1 << 29) - 1
  assert M.XT_STREAM < M.ETA_STREAM and M.ETA_STREAM + top < M.ENCODE_STREAM < M.Q_STREAM
  assert M.Q_STREAM + top < 1 << 32


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_moments_of_the_restatement(dtype):
  n = 1 << 16
  z = R.normals(1234, 0, 7, 1, n, dtype)[0]
  assert z.dtype == dtype
  R.check_moments(z, f"restatement {dtype.__name__}")
  other = R.normals(1234, 1, 7, 1, n, dtype)[0].astype(np.float64)
  z = z.astype(np.float64)
  bound = R.moment_bounds(n)[4]
  corr = float(np.corrcoef(z, other)[0, 1])
  lag1 = float(np.corrcoef(z[:-1], z[1:])[0, 1])
  print(f"correlation with sample 1: {corr:.2e}, lag-1 autocorrelation {lag1:.2e} (bound {bound:.2e})")
  assert abs(corr) < bound and abs(lag1) < bound
  # other streams and seeds are other numbers
  assert not np.array_equal(z, R.normals(1234, 0, 8, 1, n)[0])
  assert not np.array_equal(z, R.normals(1235, 0, 7, 1, n)[0])
  assert not np.array_equal(z, R.normals(1234 + (1 << 32), 0, 7, 1, n)[0])


def test_float32_restatement_is_close_to_float64():
  z64 = R.normals(5, 0, 3, 2, 1 << 14)
  z32 = R.normals(5, 0, 3, 2, 1 << 14, np.float32)
  assert np.abs(z32 - z64).max() < 1e-4


# ---- C ABI --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENTRIES)
def test_header_lib_and_library_agree_on_the_entries(name):
  from ldm_tf2_amd import _lib
  src = open(os.path.join(ROOT, "include", "ldm_hip.h")).read()
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
  assert m, f"include/ldm_hip.h does not declare {name}"
  params = [p.strip() for p in m.group(1).split(",")]
  res, args = _lib.SIGNATURES[name]
  assert res is ctypes.c_int32 and len(args) == len(params)
  for p, a in zip(params, args):
    want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else
            ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_float if p.startswith("float") else
            ctypes.c_int32)
    assert a is want, (p, a)
  assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None


def test_ops_reject_host_tensors():
  from ldm_tf2_amd import ops
  z = torch.zeros(2, 4, 4, 4)
  rng = torch.zeros(4, dtype=torch.int32)
  i = torch.zeros(1, dtype=torch.int32)
  with pytest.raises(ValueError):
    ops.normal_fill(z, rng, 0)
  with pytest.raises(ValueError):
    ops.philox_u32(torch.zeros(2, 64, dtype=torch.int32), rng, 0)
  with pytest.raises(ValueError):
    ops.cfg_ddim_update_rng(torch.zeros(4, 4, 4, 4), z, z.clone(), torch.zeros(10, 4), i, rng, 5.)
  with pytest.raises(ValueError):
    ops.cfg_plms_update_rng(torch.zeros(4, 4, 4, 4), z, z.clone(), torch.zeros(4, 2, 4, 4, 4), torch.zeros(10, 4), i, i,
                            rng, 5.)
  with pytest.raises(ValueError):
    ops.q_sample_rng(z, rng, 0, torch.zeros(2, dtype=torch.int32), torch.zeros(10), torch.zeros(10), z.clone())


# ---- constructor and CLI ------------------------------------------------------------------------------
def test_constructor_switch():
  from ldm_tf2_amd import model_runners as M
  assert _sampler(num_ddim_steps=50)._noise_source == "host"
  assert _sampler(num_ddim_steps=50, noise_source="host")._noise_source == "host"
  s = _sampler(num_ddim_steps=50, eta=1., noise_source="device")
  assert s._noise_source == "device" and s._graph is None and s._rng is None
  assert _sampler(num_ddim_steps=50, sampler="plms", noise_source="device")._sampler == "plms"
  with pytest.raises(ValueError, match="noise_source"):
    _sampler(num_ddim_steps=50, noise_source="gpu")
  assert M.NOISE_SOURCES == ("host", "device")


def test_cli_plumbs_the_noise_source_key(monkeypatch):
  from ldm_tf2_amd import run_ldm_sampler as R_
  with open(CFG) as f:
    cfg = yaml.safe_load(f)
  for name in ("TransformerModel", "UNet", "AutoencoderKL", "AutoencoderVQ"):
    monkeypatch.setattr(R_, name, _FakeModel)
  monkeypatch.setattr(R_, "_load_weights", lambda path, what: None)
  ids = np.zeros((8, 77), dtype=np.int64)
  assert "noise_source" not in cfg["ldm_sampling"]                 # the reference's YAML, unchanged
  assert R_.noise_source_name(cfg) == "host"
  assert R_.build_from_config(cfg, device="cpu")._noise_source == "host"
  call = R_.sampling_call(cfg, ids, 5)
  cfg["ldm_sampling"]["noise_source"] = "device"
  assert R_.noise_source_name(cfg) == "device"
  s = R_.build_from_config(cfg, device="cpu")
  assert s._noise_source == "device" and s._sampler == "ddim"
  got = R_.sampling_call(cfg, ids, 5)                              # the call itself does not depend on the source
  assert got[0] == call[0] == "ddim_p_sample_loop" and got[2] == call[2]
  cfg["ldm_sampling"]["sampler"] = "plms"
  cfg["ldm"]["eta"] = 0.
  assert R_.build_from_config(cfg, device="cpu")._noise_source == "device"
  cfg["ldm_sampling"]["noise_source"] = "philox"
  with pytest.raises(ValueError, match="noise_source"):
    R_.build_from_config(cfg, device="cpu")
