"""csrc/exact.h keeps its promise in the generated code: a product and a sum written through its helpers stay two
instructions where they are inlined into a translation unit that ALLOWS contraction (no file-level pragma).  A compiler
upgrade that starts fusing them again fails here, not in a bit-exact test that happens to have a pair on the radius."""
import os
import re
import subprocess

import pytest

from pointcontrast_amd import build

PROBE = r"""
#include "exact.h"
using namespace pcmi;
__global__ void probe_muladd(const double* a, const double* b, const double* c, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  o[i] = add_rn(mul_rn(a[i], b[i]), c[i]);
}
__global__ void probe_rigid(const double* m, const double* p, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double q[3];
  rigid_apply(m, 4, p + 3 * i, q);
  o[i] = dist2_rn(q, p);
}
"""


def test_exact_helpers_are_not_contracted(tmp_path):
  try:
    hipcc = build._hipcc()
  except RuntimeError:
    pytest.skip("hipcc not found")
  if os.path.isabs(hipcc) and not os.path.exists(hipcc):
    pytest.skip("hipcc not found")
  src, asm = tmp_path / "probe.hip", tmp_path / "probe.s"
  src.write_text(PROBE)
  cmd = [hipcc] + build.FLAGS + ["-I", build.CSRC, "--cuda-device-only", "-S", str(src), "-o", str(asm)]
  try:
    r = subprocess.run(cmd, capture_output=True, text=True)
  except FileNotFoundError:
    pytest.skip("hipcc not found")
  assert r.returncode == 0, r.stderr
  text = asm.read_text()
  ops = re.findall(r"^\s*(v_[a-z0-9_]*f64[a-z0-9_]*)", text, re.M)
  assert not [o for o in ops if o.startswith(("v_fma_f64", "v_fmac_f64"))], sorted(set(ops))
  assert any(o.startswith("v_mul_f64") for o in ops) and any(o.startswith("v_add_f64") for o in ops), sorted(set(ops))
