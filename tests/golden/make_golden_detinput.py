"""Records tests/golden/golden_detinput.npz by running the REFERENCE's own detection datasets, unmodified, over small synthetic
scans written to a temporary directory:  python tests/golden/make_golden_detinput.py <reference root>

What runs, from downstream/votenet_det_new of the reference: ScannetDetectionDataset.__getitem__
(lib/datasets/scannet/scannet_detection_dataset.py), SunrgbdDetectionVotesDataset.__getitem__
(lib/datasets/sunrgbd/sunrgbd_detection_dataset.py), and VoxelizationDataset.__getitem__ with collate_fn
(models/backbone/sparseconv/voxelized_dataset.py).  The dataset objects are made with object.__new__ and their attributes set
by hand, because their constructors list a data directory inside the reference tree.  plyfile, trimesh and cv2 are not
installed where this runs and are served by empty stand-in modules (nothing that runs here calls them);
ME.utils.sparse_quantize comes from oracle/me_shim.py.  np.random is seeded per scan, and np.random.random and
np.random.choice are wrapped so that the draws they hand out are recorded next to the outputs: they are inputs of our kernels.

The file holds arrays only: the scans, the recorded draws, and every key of the dicts the reference returned.  It is written
with fixed zip timestamps, so that it regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden_detinput.npz")
ROOT = os.path.dirname(os.path.dirname(HERE))
NUM_POINTS = 300
VOXEL_SIZE = 0.2
DICT_KEYS = ["point_clouds", "center_label", "heading_class_label", "heading_residual_label", "size_class_label",
             "size_residual_label", "sem_cls_label", "box_label_mask", "vote_label", "vote_label_mask"]


def import_reference(root):
  """(scannet dataset module, sunrgbd dataset module, voxelized_dataset module) of the reference."""
  vn = os.path.join(root, "downstream", "votenet_det_new")
  assert os.path.isfile(os.path.join(vn, "lib", "utils", "pc_util.py")), "%s is not the reference" % root
  for name in ("plyfile", "trimesh", "cv2"):
    stub = types.ModuleType(name)
    stub.PlyData = stub.PlyElement = None  # pc_util.py: `from plyfile import PlyData, PlyElement`
    sys.modules[name] = stub
  sys.path.insert(0, ROOT)
  from oracle import me_shim
  me_shim.install()
  sys.path.insert(0, vn)
  sys.path.insert(0, os.path.join(vn, "lib", "utils"))

  def load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(vn, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod

  sc = load("ref_scannet_detection_dataset", "lib/datasets/scannet/scannet_detection_dataset.py")
  su = load("ref_sunrgbd_detection_dataset", "lib/datasets/sunrgbd/sunrgbd_detection_dataset.py")
  vx = load("ref_voxelized_dataset", "models/backbone/sparseconv/voxelized_dataset.py")
  return sc, su, vx


class Recorder:
  """Wraps np.random.random and np.random.choice; keeps what they returned."""

  def __enter__(self):
    self.uniform, self.choices = [], []
    self._random, self._choice = np.random.random, np.random.choice
    np.random.random = lambda *a: (self.uniform.append(self._random(*a)), self.uniform[-1])[1]
    np.random.choice = lambda *a, **k: (self.choices.append(self._choice(*a, **k)), self.choices[-1])[1]
    return self

  def __exit__(self, *exc):
    np.random.random, np.random.choice = self._random, self._choice


def scannet_scan(rng, n, k, nyu40ids):
  """A room of n vertices in 9 instances.  Instance 0 is unannotated (semantic 0); instance 1 a wall (semantic 1, not a
  detection class); instance 2 carries TWO semantic labels, a valid one and an invalid one in an order the sampling decides;
  the others a valid class each."""
  vert = np.zeros((n, 6), np.float32)
  ins = rng.randint(0, 9, n).astype(np.int64)
  cen = rng.uniform(-2, 2, (9, 3))
  vert[:, 0:3] = (cen[ins] + rng.uniform(-0.5, 0.5, (n, 3))).astype(np.float32)
  vert[:, 3:6] = rng.randint(0, 256, (n, 3))
  sem_of = np.array([0, 1] + [int(v) for v in rng.choice(nyu40ids, 7)])
  sem = sem_of[ins].astype(np.int64)
  two = np.nonzero(ins == 2)[0]
  sem[two[::2]] = 2  # the floor's label among instance 2's rows
  boxes = np.zeros((k, 7))
  boxes[:, 0:3] = rng.uniform(-2, 2, (k, 3))
  boxes[:, 3:6] = rng.uniform(0.2, 1.5, (k, 3))
  boxes[:, 6] = rng.choice(nyu40ids, k)
  return vert, ins, sem, boxes


def sunrgbd_scan(rng, n, k, headings):
  pc = np.zeros((n, 6), np.float32)
  pc[:, 0:3] = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
  pc[:, 3:6] = rng.uniform(0, 1, (n, 3)).astype(np.float32)
  votes = np.zeros((n, 10))
  on = rng.uniform(size=n) < 0.6
  votes[on, 0] = 1.0
  votes[on, 1:10] = rng.uniform(-0.7, 0.7, (int(on.sum()), 9))
  boxes = np.zeros((k, 8))
  boxes[:, 0:3] = rng.uniform(-2, 2, (k, 3))
  boxes[:, 3:6] = rng.uniform(0.1, 0.9, (k, 3))
  boxes[:, 6] = headings[:k]
  boxes[:, 7] = rng.randint(0, 10, k)
  return pc, boxes, votes


def save_npz(path, arrays):
  """np.savez_compressed with fixed timestamps."""
  with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
    for name in sorted(arrays):
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
      info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      z.writestr(info, buf.getvalue())


def generate(root):
  sc, su, vx = import_reference(root)
  out = {"num_points": np.int64(NUM_POINTS), "voxel_size": np.float64(VOXEL_SIZE)}
  tmp = tempfile.mkdtemp(prefix="detinput_")
  # ---- ScanNet: scans 0..2 augmented (1 is smaller than num_points, 2 has no box), then scan 0 again without augmentation ----
  nyu = np.asarray(sc.DC.nyu40ids)
  out["scannet_nyu40ids"] = nyu.astype(np.int32)
  out["scannet_mean_size_arr"] = np.asarray(sc.DC.mean_size_arr, dtype=np.float64)
  rng = np.random.RandomState(20261018)
  names = []
  for s, (n, k) in enumerate([(500, 5), (120, 3), (400, 0)]):
    vert, ins, sem, boxes = scannet_scan(rng, n, k, nyu)
    name = "scene%04d_00" % s
    names.append(name)
    for suffix, arr in (("_vert", vert), ("_ins_label", ins), ("_sem_label", sem), ("_bbox", boxes)):
      np.save(os.path.join(tmp, name + suffix + ".npy"), arr)
    out.update({"scannet%d_vert" % s: vert[:, 0:3].copy(), "scannet%d_ins" % s: ins.astype(np.int32), "scannet%d_sem" % s: sem.astype(np.int32),
                "scannet%d_bbox" % s: boxes})
  runs = [(0, True, 11), (1, True, 12), (2, True, 18), (0, False, 14)]
  samples = []
  for r, (s, augment, seed) in enumerate(runs):
    ds = object.__new__(sc.ScannetDetectionDataset)
    ds.data_path, ds.scan_names, ds.num_points = tmp, names, NUM_POINTS
    ds.use_color, ds.use_height, ds.augment = False, False, augment
    np.random.seed(seed)
    with Recorder() as rec:
      sample = vx.VoxelizationDataset(ds, voxel_size=VOXEL_SIZE)[s]
    samples.append(sample)
    u = rec.uniform + [0.0, 0.0, 0.5][len(rec.uniform):]
    out.update({"scannet_run%d_scan" % r: np.int64(s), "scannet_run%d_augment" % r: np.int64(augment),
                "scannet_run%d_choices" % r: np.asarray(rec.choices[0], dtype=np.int32),
                "scannet_run%d_flip" % r: np.array([u[0] > 0.5, u[1] > 0.5], dtype=np.int32) if augment else np.zeros(2, np.int32),
                "scannet_run%d_rot_angle" % r: np.float64((u[2] * np.pi / 18) - np.pi / 36) if augment else np.float64(0.0)})
    for key in DICT_KEYS:
      out["scannet_run%d_%s" % (r, key)] = sample[key]
    out["scannet_run%d_voxel_coords" % r], out["scannet_run%d_voxel_inds" % r] = sample["voxel"]
  flips = np.stack([out["scannet_run%d_flip" % r] for r in range(3)])
  assert flips[:, 0].min() == 0 and flips[:, 0].max() == 1 and flips[:, 1].min() == 0 and flips[:, 1].max() == 1, \
      "the seeds no longer give both flips on and off: %s" % flips
  batch = vx.collate_fn(samples[:3])
  out.update({"scannet_batch_voxel_coords": batch["voxel_coords"].numpy(), "scannet_batch_voxel_inds": batch["voxel_inds"].numpy(),
              "scannet_batch_voxel_feats": batch["voxel_feats"].numpy(), "scannet_batch_point_clouds": batch["point_clouds"].numpy()})
  out["scannet_runs"] = np.int64(len(runs))
  # ---- SUN RGB-D: the same plan; headings below 0, above 2 pi and on a bin border -------------------------------------------
  out["sunrgbd_mean_size_arr"] = np.asarray(su.DC.mean_size_arr, dtype=np.float64)
  out["sunrgbd_num_heading_bin"] = np.int64(su.DC.num_heading_bin)
  headings = np.array([-2.5, 7.0, np.pi / 12, 0.0, 3.0, -0.2])
  names = []
  for s, (n, k) in enumerate([(450, 6), (100, 2), (350, 0)]):
    pc, boxes, votes = sunrgbd_scan(rng, n, k, headings)
    name = "%06d" % (s + 1)
    names.append(name)
    np.savez_compressed(os.path.join(tmp, name + "_pc.npz"), pc=pc)
    np.save(os.path.join(tmp, name + "_bbox.npy"), boxes)
    np.savez_compressed(os.path.join(tmp, name + "_votes.npz"), point_votes=votes)
    out.update({"sunrgbd%d_pc" % s: pc[:, 0:3].copy(), "sunrgbd%d_bbox" % s: boxes, "sunrgbd%d_votes" % s: votes})
  runs = [(0, True, 21), (1, True, 23), (2, True, 24), (0, False, 25)]
  samples = []
  for r, (s, augment, seed) in enumerate(runs):
    ds = object.__new__(su.SunrgbdDetectionVotesDataset)
    ds.data_path, ds.scan_names, ds.num_points = tmp, names, NUM_POINTS
    ds.use_color, ds.use_height, ds.augment, ds.use_v1 = False, False, augment, False
    np.random.seed(seed)
    with Recorder() as rec:
      sample = vx.VoxelizationDataset(ds, voxel_size=VOXEL_SIZE)[s]
    samples.append(sample)
    u = rec.uniform + [0.0, 0.5, 0.5][len(rec.uniform):]
    out.update({"sunrgbd_run%d_scan" % r: np.int64(s), "sunrgbd_run%d_augment" % r: np.int64(augment),
                "sunrgbd_run%d_choices" % r: np.asarray(rec.choices[0], dtype=np.int32),
                "sunrgbd_run%d_flip" % r: np.array([u[0] > 0.5, False], dtype=np.int32) if augment else np.zeros(2, np.int32),
                "sunrgbd_run%d_rot_angle" % r: np.float64((u[1] * np.pi / 3) - np.pi / 6) if augment else np.float64(0.0),
                "sunrgbd_run%d_scale" % r: np.float64(u[2] * 0.3 + 0.85) if augment else np.float64(1.0)})
    for key in DICT_KEYS:
      out["sunrgbd_run%d_%s" % (r, key)] = sample[key]
    out["sunrgbd_run%d_voxel_coords" % r], out["sunrgbd_run%d_voxel_inds" % r] = sample["voxel"]
  flips = np.stack([out["sunrgbd_run%d_flip" % r] for r in range(3)])
  assert flips[:, 0].min() == 0 and flips[:, 0].max() == 1, "the seeds no longer give the flip on and off: %s" % flips
  batch = vx.collate_fn(samples[:3])
  out.update({"sunrgbd_batch_voxel_coords": batch["voxel_coords"].numpy(), "sunrgbd_batch_voxel_inds": batch["voxel_inds"].numpy(),
              "sunrgbd_batch_voxel_feats": batch["voxel_feats"].numpy(), "sunrgbd_batch_point_clouds": batch["point_clouds"].numpy()})
  out["sunrgbd_runs"] = np.int64(len(runs))
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
