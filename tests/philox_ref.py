"""NumPy restatement of the device noise generator: integer Philox4x32-10 (Salmon et al.,
SC'11), the word -> uniform map, and Box-Muller in float64 and in float32.  Written from the definition, not from
the kernel: the tests hold the kernel against this."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
XT_STREAM, ETA_STREAM, ENCODE_STREAM, Q_STREAM = 0, 1 << 29, 1 << 30, (1 << 30) + 1
Z_MAX = float(np.sqrt(50 * np.log(2.)))          # |z| <= sqrt(-2 ln 2^-25)


def philox4x32_10(counter, key):
  """counter: four uint32 arrays (broadcastable), key: two ints.  Returns four uint64 arrays holding 32-bit words."""
  c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in counter]
  c = list(np.broadcast_arrays(*c))
  k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
  for _ in range(10):
    p0 = np.uint64(M0) * c[0]                      # 32 x 32 -> 64: no overflow in uint64
    p1 = np.uint64(M1) * c[2]
    hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
    hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
    c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
  return c


def key_of(seed):
  seed = int(seed) % (1 << 64)
  return seed & MASK, seed >> 32


def words(seed, first_sample_index, stream, B, n):
  """[B, n] uint32: element e of sample b is word e & 3 of the counter (e >> 2, first + b, stream, 0)."""
  assert n % 4 == 0
  q = np.arange(n // 4, dtype=np.uint64)[None, :]
  g = ((int(first_sample_index) + np.arange(B, dtype=np.uint64)) & np.uint64(MASK))[:, None]
  w = philox4x32_10((q, g, int(stream) & MASK, 0), key_of(seed))
  return np.stack(w, axis=-1).reshape(B, n).astype(np.uint32)


def uniform(x, dtype):
  """u = ((x >> 8) + 0.5) * 2^-24.  float64: exact.  float32: the sum is rounded to nearest even above 2^23."""
  return (((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)).astype(dtype)


def normals_from_words(w, dtype=np.float64):
  """[..., n] words -> [..., n] normals: (x0, x1) -> r cos, r sin; (x2, x3) likewise.  All arithmetic in `dtype`."""
  w = np.asarray(w, dtype=np.uint32)
  p = w.reshape(w.shape[:-1] + (w.shape[-1] // 2, 2))
  u0, u1 = uniform(p[..., 0], dtype), uniform(p[..., 1], dtype)
  r = np.sqrt(dtype(-2.0) * np.log(u0)).astype(dtype)
  a = (dtype(2.0 * np.pi) * u1).astype(dtype)
  z = np.stack([r * np.cos(a).astype(dtype), r * np.sin(a).astype(dtype)], axis=-1).astype(dtype)
  return z.reshape(w.shape)


def normals(seed, first_sample_index, stream, B, n, dtype=np.float64):
  return normals_from_words(words(seed, first_sample_index, stream, B, n), dtype)


def moment_bounds(n):
  """5-sigma bounds that follow from the count alone: (|mean|, |var - 1|, |m4 - 3|, max |z|, |correlation|)."""
  return 5 / np.sqrt(n), 5 * np.sqrt(2. / n), 5 * np.sqrt(96. / n), Z_MAX, 5 / np.sqrt(n)


def moments(z):
  z = np.asarray(z, dtype=np.float64).ravel()
  m = z.mean()
  return m, z.var(), ((z - m) ** 4).mean(), np.abs(z).max()


def check_moments(z, what=""):
  n = np.asarray(z).size
  m, v, m4, mx = moments(z)
  bm, bv, b4, bx, _ = moment_bounds(n)
  print(f"{what} n={n}: mean {m:.3e} (<= {bm:.3e}) var {v:.5f} (+- {bv:.4f}) m4 {m4:.4f} (+- {b4:.4f}) "
        f"max {mx:.3f} (<= {bx:.3f})")
  assert abs(m) <= bm and abs(v - 1) <= bv and abs(m4 - 3) <= b4 and mx <= bx, (what, m, v, m4, mx)
  return m, v, m4, mx
