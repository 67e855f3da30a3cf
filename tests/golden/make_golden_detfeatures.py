"""Records tests/golden/golden_detfeatures.npz by running the REFERENCE's own detection datasets, unmodified, with use_height
(and use_color) over small synthetic scans written to a temporary directory:
  python tests/golden/make_golden_detfeatures.py <reference root>

What runs, from downstream/votenet_det_new of the reference: ScannetDetectionDataset.__getitem__ and
SunrgbdDetectionVotesDataset.__getitem__, set up as tests/golden/make_golden_detinput.py sets them up (whose helpers this
script imports): objects made with object.__new__, stand-in modules for plyfile, trimesh and cv2, np.random seeded per run and
np.random.random / np.random.choice wrapped so that the draws are recorded next to the outputs.

Plan (RUNS), SUN RGB-D: scan 0 with use_color off and on, each with augmentation on and off, and scan 1 -- fewer vertices than
num_points (300), sampled with replacement -- augmented with colour.  ScanNet cannot be recorded with colour:
ScannetDetectionDataset with use_color=True raises UnboundLocalError in the reference itself (scannet_detection_dataset.py:108
reads pcl_color, which line 85 assigns only without use_color).  The script asserts that it still does; ScanNet is recorded
with the height column only -- scan 0 with augmentation on and off, scan 1 augmented -- and the tests hold ScanNet's colour
rule to line 88's expression instead.

The SUN RGB-D height is scaled by `point_cloud[:,-1] *= scale_ratio[0,0]`, a float32 column times a numpy float64 scalar in
place: numpy >= 2 multiplies in float64 and rounds once, numpy < 2 multiplies in float32.  The file is recorded with the numpy
installed where this runs (its version is stored under "numpy_version"); pcmi.h states the float64 rule.

The file holds arrays only -- the scans, the recorded draws and the reference's point_clouds -- and is written with fixed zip
timestamps, so that it regenerates byte for byte."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_detinput import NUM_POINTS, Recorder, import_reference, save_npz, scannet_scan, sunrgbd_scan  # noqa: E402

PATH = os.path.join(HERE, "golden_detfeatures.npz")
# (scan, use_color, augment, seed)
RUNS = [(0, False, True, 31), (0, True, True, 32), (0, False, False, 33), (0, True, False, 34), (1, True, True, 35)]


def generate(root):
  sc, su, _ = import_reference(root)
  out = {"num_points": np.int64(NUM_POINTS), "numpy_version": np.array([int(v) for v in np.__version__.split(".")[:2]], dtype=np.int64)}
  tmp = tempfile.mkdtemp(prefix="detfeatures_")
  rng = np.random.RandomState(20261019)
  # ---- ScanNet ---------------------------------------------------------------------------------------------------------------
  nyu = np.asarray(sc.DC.nyu40ids)
  names = []
  for s, (n, k) in enumerate([(500, 4), (120, 2)]):
    vert, ins, sem, boxes = scannet_scan(rng, n, k, nyu)
    name = "scene%04d_00" % s
    names.append(name)
    for suffix, arr in (("_vert", vert), ("_ins_label", ins), ("_sem_label", sem), ("_bbox", boxes)):
      np.save(os.path.join(tmp, name + suffix + ".npy"), arr)
    out["scannet%d_vert" % s] = vert

  def scannet_dataset(color, augment):
    ds = object.__new__(sc.ScannetDetectionDataset)
    ds.data_path, ds.scan_names, ds.num_points = tmp, names, NUM_POINTS
    ds.use_color, ds.use_height, ds.augment = color, True, augment
    return ds

  try:
    scannet_dataset(True, True)[0]
  except UnboundLocalError:
    pass
  else:
    raise AssertionError("the reference's ScanNet dataset now runs with use_color: record it")
  r = 0
  for s, color, augment, seed in RUNS:
    if color and s == 0:
      continue  # scan 0 is recorded without colour already; scan 1, the small one, is recorded without it here
    np.random.seed(seed)
    with Recorder() as rec:
      sample = scannet_dataset(False, augment)[s]
    u = rec.uniform + [0.0, 0.0, 0.5][len(rec.uniform):]
    out.update({"scannet_run%d_scan" % r: np.int64(s), "scannet_run%d_augment" % r: np.int64(augment),
                "scannet_run%d_choices" % r: np.asarray(rec.choices[0], dtype=np.int32),
                "scannet_run%d_flip" % r: np.array([u[0] > 0.5, u[1] > 0.5], dtype=np.int32) if augment else np.zeros(2, np.int32),
                "scannet_run%d_rot_angle" % r: np.float64((u[2] * np.pi / 18) - np.pi / 36) if augment else np.float64(0.0),
                "scannet_run%d_point_clouds" % r: sample["point_clouds"]})
    assert sample["point_clouds"].shape == (NUM_POINTS, 4) and sample["point_clouds"].dtype == np.float32
    r += 1
  out["scannet_runs"] = np.int64(r)
  # ---- SUN RGB-D -------------------------------------------------------------------------------------------------------------
  headings = np.array([-2.5, 7.0, np.pi / 12, 0.0])
  names = []
  for s, (n, k) in enumerate([(450, 4), (100, 2)]):
    pc, boxes, votes = sunrgbd_scan(rng, n, k, headings)
    name = "%06d" % (s + 1)
    names.append(name)
    np.savez_compressed(os.path.join(tmp, name + "_pc.npz"), pc=pc)
    np.save(os.path.join(tmp, name + "_bbox.npy"), boxes)
    np.savez_compressed(os.path.join(tmp, name + "_votes.npz"), point_votes=votes)
    out["sunrgbd%d_pc" % s] = pc
  for r, (s, color, augment, seed) in enumerate(RUNS):
    ds = object.__new__(su.SunrgbdDetectionVotesDataset)
    ds.data_path, ds.scan_names, ds.num_points = tmp, names, NUM_POINTS
    ds.use_color, ds.use_height, ds.augment, ds.use_v1 = color, True, augment, False
    np.random.seed(seed)
    with Recorder() as rec:
      sample = ds[s]
    n = len(out["sunrgbd%d_pc" % s])
    pre = "sunrgbd_run%d_" % r
    # the order of the draws: flip, angle, [gain (3), shift (3), jitter (n), keep (n)], scale
    u = list(rec.uniform)
    if augment:
      assert len(u) == (7 if color else 3)
      if color:
        assert u[2].shape == (3,) and u[3].shape == (3,) and u[4].shape == (n,) and u[5].shape == (n,)
        out.update({pre + "color_gain": 1 + 0.4 * u[2] - 0.2, pre + "color_shift": 0.1 * u[3] - 0.05,
                    pre + "color_jitter_raw": 0.05 * u[4] - 0.025, pre + "color_keep_raw": u[5] > 0.3})
    else:
      assert len(u) == 0
      u = [0.0, 0.5, 0.5]
    out.update({pre + "scan": np.int64(s), pre + "augment": np.int64(augment), pre + "color": np.int64(color),
                pre + "choices": np.asarray(rec.choices[0], dtype=np.int32),
                pre + "flip": np.array([u[0] > 0.5, False], dtype=np.int32) if augment else np.zeros(2, np.int32),
                pre + "rot_angle": np.float64((u[1] * np.pi / 3) - np.pi / 6) if augment else np.float64(0.0),
                pre + "scale": np.float64(u[-1] * 0.3 + 0.85) if augment else np.float64(1.0),
                pre + "point_clouds": sample["point_clouds"]})
    assert sample["point_clouds"].shape == (NUM_POINTS, 7 if color else 4) and sample["point_clouds"].dtype == np.float32
  out["sunrgbd_runs"] = np.int64(len(RUNS))
  for f in os.listdir(tmp):
    os.remove(os.path.join(tmp, f))
  os.rmdir(tmp)
  return out


def main(root):
  out = generate(root)
  save_npz(PATH, out)
  print(PATH, os.path.getsize(PATH), len(out), "arrays")


if __name__ == "__main__":
  main(sys.argv[1])
