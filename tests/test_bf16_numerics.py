"""The arithmetic of the opt-in bf16 conv precision mode (pcmi_set_conv_precision, ME.conv_precision), restated in numpy
(CPU): both operands rounded to bf16 (round to nearest even -- split3's h term), ONE bf16 x bf16 product per 32-channel
chunk, fp32 accumulation.  The numbers this model gives fix the tolerances of tests/test_gpu_bf16.py (-m gpu):
  * against a float64 contraction of the ROUNDED operands it is fp32 round-off class (the products are exact, one
    rounding per chunk): the device result is held to the fp32 kernel's own error there;
  * against the UNROUNDED operands its error is of order 2^-9 of the largest output -- ~4e-3 on the wide-dynamic-range
    operands of test_conv16_x3_split_precision_matches_fp32 -- at least 100x the first error, which is how the GPU test
    tells that the one-term path ran;
  * through a residual chain as deep as Res16UNet34C's the norm-wise relative error of the features (||d|| / ||f||)
    stays under 1e-2, a third of the 3e-2 the GPU network test allows.  (The max-norm error of one element is NOT what
    the network test bounds: over the 5.6 M feature entries of a configs[1] pass its extreme value grows with the
    sample, and the first GPU run measured 3.7e-2 there.)
Also the Python surface: unknown modes are refused, the default is fp32."""
import numpy as np
import pytest

from test_x3_numerics import bf16_rne, contract


def _wide_operands(seed, rows, K, N):
  rng = np.random.RandomState(seed)
  A = (rng.randn(rows, K) * np.exp(rng.randn(rows, 1))).astype(np.float32)  # rows of very different scale
  B = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
  return A, B


def _rel(got, ref):
  return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("cin,cout", [(96, 96), (128, 96), (64, 128), (256, 256)])
def test_one_term_contraction_error_model(cin, cout):
  K = 27 * cin  # the contraction of a 3^3 convolution
  A, B = _wide_operands(cin + cout, 64, K, cout)
  ar, br = bf16_rne(A), bf16_rne(B)
  for part in (ar, br):  # what the kernel multiplies is a bf16 value
    assert np.array_equal(part.view(np.uint32) & 0xFFFF, np.zeros(part.shape, np.uint32))
  y1 = contract([(ar, br)], K)
  e_rounded = _rel(y1, ar.astype(np.float64) @ br.astype(np.float64))
  e_unrounded = _rel(y1, A.astype(np.float64) @ B.astype(np.float64))
  assert e_rounded < 2e-6, "one product per chunk, fp32 accumulation: fp32 round-off class (%.2e)" % e_rounded
  assert 2 ** -13 < e_unrounded < 2 ** -6, "bf16 operands: error of order 2^-9 (%.2e)" % e_unrounded
  assert e_unrounded > 100 * e_rounded, (e_unrounded, e_rounded)


def test_one_term_error_through_a_deep_chain():
  """Res16UNet34C has ~45 convolutions on its longest path, in residual blocks; each rounds its operands once.
  Normalised random residual layers with ReLU (x <- relu(x + x W)): the relative feature error stays at half of the
  network test's 3e-2.  (Without the skip connections the same chain reaches ~2e-2 at depth 32.)"""
  rng = np.random.RandomState(3)
  C, rows, depth = 96, 256, 48
  x = rng.randn(rows, C).astype(np.float32)
  x64 = x.astype(np.float64)
  for _ in range(depth):
    W = (rng.randn(C, C) * np.sqrt(2.0 / C)).astype(np.float32)
    x = np.maximum(contract([(bf16_rne(x), bf16_rne(W))], C) + x, 0)
    x64 = np.maximum(x64 @ W.astype(np.float64) + x64, 0)
    s = np.abs(x64).max()
    x, x64 = (x / s).astype(np.float32), x64 / s
  e = _rel(x, x64)
  e_norm = float(np.linalg.norm(x - x64) / np.linalg.norm(x64))
  assert e < 1.5e-2 and e_norm < 1e-2, (e, e_norm)


def test_conv_precision_surface_rejects_unknown_modes():
  import pointcontrast_amd.minkowski as ME
  from pointcontrast_amd import functional as PF
  from pointcontrast_amd._lib import lib
  assert ME.get_conv_precision() == "fp32"
  for bad in ("fp16", "BF16", "bfloat16", "", None, 1, "tf32"):
    with pytest.raises(ValueError):
      ME.set_conv_precision(bad)
    with pytest.raises(ValueError):
      with ME.conv_precision(bad):
        pass
  assert ME.get_conv_precision() == "fp32"
  assert lib.pcmi_set_conv_precision(7) != 0 and lib.pcmi_get_conv_precision() == PF.CONV_PRECISIONS["fp32"]
  with ME.conv_precision("bf16"):
    assert ME.get_conv_precision() == "bf16"
    with ME.conv_precision("fp32"):
      assert ME.get_conv_precision() == "fp32"
    assert ME.get_conv_precision() == "bf16"
  assert ME.get_conv_precision() == "fp32"
  ME.set_conv_precision("bf16")
  try:
    assert ME.get_conv_precision() == "bf16"
  finally:
    ME.set_conv_precision("fp32")


def test_conv_precision_is_thread_local():
  import threading
  import pointcontrast_amd.minkowski as ME
  seen = []
  with ME.conv_precision("bf16"):
    t = threading.Thread(target=lambda: seen.append(ME.get_conv_precision()))
    t.start()
    t.join()
  assert seen == ["fp32"]


def test_config_default_is_fp32():
  from pointcontrast_amd.lib.config import get_config
  assert get_config([]).misc.conv_precision == "fp32"
  assert get_config(["misc.conv_precision=bf16"]).misc.conv_precision == "bf16"
  from pointcontrast_amd.downstream.semseg import SegmentationTrainer
  from pointcontrast_amd.engine import NativeEngine
  import inspect
  assert inspect.signature(NativeEngine).parameters["conv_precision"].default == "fp32"
  assert inspect.signature(SegmentationTrainer).parameters["conv_precision"].default == "fp32"
