"""Generates tests/golden/golden_segeval.npz by running the REFERENCE'S OWN segmentation-validation functions on a small seeded
input.

Run from the repo root where the reference tree is present:
    python tests/golden/make_golden_segeval.py

What runs, imported unmodified from downstream/semseg/lib of the reference: utils.py (precision_at_one, fast_hist,
per_class_iu, get_prediction, AverageMeter) and test.py (average_precision, i.e. label_binarize + scikit-learn's
average_precision_score(average=None)).  Those files (and the package's __init__) import open3d, omegaconf, MinkowskiEngine and the
point-cloud I/O helpers of lib.pc_utils; empty stand-in modules serve the imports that are absent, because none of the functions used here reaches
them.  The file holds arrays only -- the inputs, what those functions returned, and the number of positives per class (the
installed scikit-learn decides what a class without positives scores: NaN in the reference's version, 0 with a warning from
1.x on; tests compare such classes by `npos`, not by the recorded value).
"""
import os
import sys
import types
import warnings

import numpy as np

REF_ROOT = "/root/reference/downstream/semseg"
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden_segeval.npz")
sys.path.insert(0, os.path.dirname(HERE))
import segeval_ref as S  # noqa: E402

N, C, N_POOL, IGNORE, EMPTY_CLASS = 3000, 7, 37, 255, 4
BATCHES = (1300, 900, 800)  # the rows of the three batches the accumulation is recorded over


def reference_available():
  return os.path.isfile(os.path.join(REF_ROOT, "lib", "test.py"))


def import_reference():
  """(lib.utils, lib.test) of the reference."""
  assert reference_available(), "%s is not present" % REF_ROOT
  stand_ins = {"open3d": (), "omegaconf": ("OmegaConf",), "MinkowskiEngine": ("SparseTensor",),
               "lib.pc_utils": ("colorize_pointcloud", "save_point_cloud")}
  names = ("lib", "lib.utils", "lib.test", "lib.distributed_utils") + tuple(stand_ins)
  saved = {k: sys.modules.get(k) for k in names}
  for k in names:
    sys.modules.pop(k, None)
  for k, attrs in stand_ins.items():
    if k != "lib.pc_utils" and saved[k] is not None:
      sys.modules[k] = saved[k]
      continue
    m = types.ModuleType(k)
    for a in attrs:
      setattr(m, a, None)
    sys.modules[k] = m
  sys.path.insert(0, REF_ROOT)
  try:
    import lib.utils as lu
    import lib.test as lt
    return lu, lt
  finally:
    sys.path.remove(REF_ROOT)
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v


def make_inputs():
  """Rows repeated from a pool of 37 (entries multiples of 0.5: ties between rows are exact), 10 % ignored labels, one class
  that no row is labelled with."""
  rng = np.random.RandomState(20261017)
  logits, idx, pool = S.pool_rows(rng, N_POOL, C, N)
  target = rng.randint(0, C - 1, N)
  target[target >= EMPTY_CLASS] += 1
  target[rng.rand(N) < 0.1] = IGNORE
  return dict(logits=logits, pool_index=idx.astype(np.int64), target=target.astype(np.int64), prob=S.softmax(logits))


def run_reference(inp):
  import torch
  lu, lt = import_reference()
  logits, target, prob = torch.from_numpy(inp["logits"]), torch.from_numpy(inp["target"]), inp["prob"]
  out = {}
  pred = lu.get_prediction(None, logits, target)
  out["pred"] = pred.numpy().astype(np.int64)
  out["score"] = np.float64(lu.precision_at_one(pred, target, IGNORE))
  hist = lu.fast_hist(pred.numpy().flatten(), inp["target"].flatten(), C)
  out["hist"] = hist.astype(np.int64)
  out["iou"] = lu.per_class_iu(hist)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    out["ap"] = np.asarray(lt.average_precision(prob, inp["target"]), np.float64)
  out["npos"] = np.array([(inp["target"] == k).sum() for k in range(C)], np.int64)
  # the accumulation of test() over three batches: the two AverageMeters, the summed histogram, np.nanmean over the batches
  crit = torch.nn.CrossEntropyLoss(ignore_index=IGNORE)
  losses, scores, hist, aps, lo = lu.AverageMeter(), lu.AverageMeter(), np.zeros((C, C)), np.zeros((0, C)), 0
  npos_b = []
  for n in BATCHES:
    x, t = logits[lo:lo + n], target[lo:lo + n]
    p = lu.get_prediction(None, x, t)
    losses.update(float(crit(x.double(), t)), n)
    scores.update(lu.precision_at_one(p, t, IGNORE), n)
    hist += lu.fast_hist(p.numpy().flatten(), t.numpy().flatten(), C)
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")
      aps = np.vstack((aps, lt.average_precision(prob[lo:lo + n], t.numpy())))
    npos_b.append([(t.numpy() == k).sum() for k in range(C)])
    lo += n
  out["acc_loss"], out["acc_score"] = np.float64(losses.avg), np.float64(scores.avg)
  out["acc_hist"], out["acc_aps"], out["acc_npos"] = hist.astype(np.int64), aps, np.asarray(npos_b, np.int64)
  out["acc_miou"] = np.float64(np.nanmean(lu.per_class_iu(hist)) * 100)
  return out


def main():
  inp = make_inputs()
  out = run_reference(inp)
  out.update(inp)
  out["batches"] = np.asarray(BATCHES, np.int64)
  np.savez_compressed(PATH, **out)
  print(PATH, os.path.getsize(PATH), sorted(out))


if __name__ == "__main__":
  main()
