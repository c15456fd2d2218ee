"""Float64 gates shared by the norm and split-K completion tests (a plain module, imported by both).

Gates, with k a case's offset / sigma:
  float32:  relative L2 <= 2e-6 + 1e-6 k;  max |err| <= 2e-4 max|gamma| for k <= 256
  bfloat16: every element within 1 bf16 ulp (taken at max(|ref|, 2^-6)); relative L2 <= 3e-3
"""
import torch

F32 = torch.float32


def bf16_ulp(ref):
  """One bf16 ulp at max(|ref|, 2^-6): 2^(floor(log2 |v|) - 7)."""
  a = ref.abs().clamp_min(2.0 ** -6)
  _, e = torch.frexp(a)
  return torch.ldexp(torch.ones_like(a), (e - 8).to(torch.int32))


def check(label, got, ref, dtype, k, gmax):
  """got: kernel output (device or CPU, any dtype); ref: float64 reference."""
  got = got.detach().cpu().double()
  ref = ref.double()
  assert got.shape == ref.shape
  assert torch.isfinite(got).all(), f"{label}: non-finite output"
  err = (got - ref).abs()
  rel = ((got - ref).norm() / ref.norm()).item()
  mx = err.max().item()
  print(f"{label}: rel-L2 {rel:.3e}  max|err| {mx:.3e}")
  if dtype == F32:
    assert rel <= 2e-6 + 1e-6 * k, f"{label}: rel-L2 {rel:.3e} > {2e-6 + 1e-6 * k:.3e}"
    if k <= 256:
      assert mx <= 2e-4 * gmax, f"{label}: max|err| {mx:.3e} > {2e-4 * gmax:.3e}"
  else:
    ulp = bf16_ulp(ref)
    worst = (err / ulp).max().item()
    assert worst <= 1.0, f"{label}: an element is {worst:.2f} bf16 ulp from the float64 reference"
    assert rel <= 3e-3, f"{label}: rel-L2 {rel:.3e} > 3e-3"
  return rel
