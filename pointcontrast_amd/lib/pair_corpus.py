"""The pre-training pair corpus, built on the device from exported depth frames.

The reference prepares ScanNetMatchPairDataset's input offline, in three CPU scripts under
pretrain/data_preprocess/scannet_pair/ ("dp/"): back-projection of every depth frame (dp/point_cloud_extractor.py:43-80),
open3d voxel down-sampling plus one KD-tree radius query per point for every ordered pair of frames
(dp/compute_full_overlapping.py:15-84), and the list of pairs with an overlap of at least 0.3 (dp/generate_list.py:20-27).
Here the geometry of a whole scene runs as libpcmi kernels (csrc/corpus.hip):

  process_scene(depths, poses, intrinsic)  arrays in, per-frame world points / voxel centroids / overlap matrices out;
  build_corpus(export_root, target_root)   the export layout of the reference's reader.py in
                                           (<scene>/depth/<n>.png, <scene>/pose/<n>.txt, <scene>/intrinsic/
                                           intrinsic_depth.txt), the files ScanNetMatchPairDataset reads out
                                           (<target>/<scene>/pcd/<n>.npz, <target>/<scene>/pcd/overlap.txt,
                                           <target>/overlap-30-full.txt).  color=True: the RGB of every point as a second
                                           npz member 'color', from <scene>/color/<n>.png or .jpg, intrinsic/intrinsic_color.txt
                                           and intrinsic/extrinsic_{color,depth}.txt (reader.py --export_color_images).

Semantics (tests/pair_corpus_ref.py restates them in numpy; the device output is bit-identical to it):
  * back-projection: d = depth / depth_shift (pixels with d == 0 dropped, the rest in row-major pixel order),
    X = ((u - cx) d) / fx + bx, Y = ((v - cy) d) / fy + by, Z = d, w_r = ((X P[r,0] + Y P[r,1]) + Z P[r,2]) + P[r,3],
    every fp64 operation rounded on its own.  The reference's np.dot (BLAS) may differ in the last bits: this order
    is ours;
  * colour (beyond the reference; tests/pair_color_ref.py): the camera-space point (X, Y, Z) through M = inv(extrinsic_color)
    extrinsic_depth and the colour intrinsic, px = floor(uc + 0.5), py = floor(vc + 0.5); the pixel's RGB if it lies inside the
    image and q2 > 0, else (0, 0, 0), counted per frame as "uncolored" (pcmi_corpus_backproject_color in include/pcmi.h);
  * a frame is dropped when its pose has a non-finite entry ("pose"), any of its points is NaN ("nan", the
    reference's rule, dp/compute_full_overlapping.py:16) or it has no points ("empty"); no npz is written for it;
  * voxel centroids as open3d's voxel_down_sample: origin = min bound - voxel / 2, index = floor((p - origin) / voxel),
    centroid = the voxel's points summed in ascending order / count, rows in order of first occurrence;
  * C[i, j] = #{q in D_j : some p in D_i within r = 1.5 voxel} (pcmi_match_radius's rounding and <=), M = C / |D_j|,
    overlap(i < j) = max(M[i, j], M[j, i]) formatted with "{}".format;
  * paths in overlap.txt and the corpus list are relative to the target root (the reference writes the paths its glob
    returned), so data.dataset_root_dir=<target> data.scannet_match_dir=overlap-30-full.txt reads the output as is.
"""
import concurrent.futures
import ctypes as C
import os
import re
import threading
import time
import zipfile

import numpy as np

LIST_NAME = "overlap-30-full.txt"
IO_THREADS = 8  # PNG decoding and npz writing (a fixed small pool: the host may be shared)
REASONS = ("pose", "nan", "empty")
_FRAME_RE = re.compile(r"^(\d+)\.png$")


# ---- export layout -------------------------------------------------------------------------------------------------
def list_frames(scene_dir, frame_skip=1):
  """Frame names of <scene>/depth/<n>.png in ascending integer order of <n>, every frame_skip-th one."""
  if frame_skip < 1:
    raise ValueError("frame_skip must be >= 1 (got %r)" % (frame_skip,))
  ddir = os.path.join(scene_dir, "depth")
  if not os.path.isdir(ddir):
    raise FileNotFoundError("%s: no depth/ directory (expected the reader.py export layout <scene>/depth/<n>.png)" % scene_dir)
  names = [m.group(1) for m in (_FRAME_RE.match(f) for f in os.listdir(ddir)) if m]
  names.sort(key=int)
  return names[::frame_skip]


def read_intrinsic(scene_dir):
  path = os.path.join(scene_dir, "intrinsic", "intrinsic_depth.txt")
  if not os.path.exists(path):
    raise FileNotFoundError("%s: missing depth intrinsic %s" % (scene_dir, path))
  K = np.loadtxt(path, dtype=np.float64)
  if K.shape != (4, 4):
    raise ValueError("%s: expected a 4x4 matrix, got shape %s" % (path, K.shape))
  return K


def read_pose(scene_dir, name):
  path = os.path.join(scene_dir, "pose", name + ".txt")
  if not os.path.exists(path):
    raise FileNotFoundError("%s: missing camera pose %s for depth frame %s.png" % (scene_dir, path, name))
  P = np.loadtxt(path, dtype=np.float64)
  if P.shape != (4, 4):
    raise ValueError("%s: expected a 4x4 matrix, got shape %s" % (path, P.shape))
  return P


def read_depth(path):
  """16-bit PNG depth (millimetres) as uint16 [H, W], decoded with PIL."""
  from PIL import Image
  with Image.open(path) as im:
    a = np.asarray(im)
  if a.ndim != 2 or a.dtype.kind not in "ui" or (a.size and (a.min() < 0 or a.max() > 65535)):
    raise ValueError("%s: not a single-channel 16-bit depth image (mode %s, dtype %s)" % (path, im.mode, a.dtype))
  return a.astype(np.uint16)


def read_color(path):
  """A colour frame (PNG or JPEG) as uint8 [Hc, Wc, 3], decoded with PIL; an alpha channel is dropped."""
  from PIL import Image
  with Image.open(path) as im:
    mode = im.mode
    a = np.asarray(im)
  if mode not in ("RGB", "RGBA") or a.ndim != 3 or a.shape[2] < 3 or a.dtype != np.uint8:
    raise ValueError("%s: not an 8-bit RGB image (mode %s, shape %s, dtype %s)" % (path, mode, a.shape, a.dtype))
  return np.ascontiguousarray(a[:, :, :3])


def color_path(scene_dir, name):
  """<scene>/color/<n>.png, or <n>.jpg if there is no PNG (reader.py --export_color_images writes JPEG)."""
  for ext in (".png", ".jpg"):
    path = os.path.join(scene_dir, "color", name + ext)
    if os.path.exists(path):
      return path
  raise FileNotFoundError("%s: missing colour image color/%s.png (or .jpg) for depth frame %s.png" % (scene_dir, name, name))


def _read_4x4(path):
  A = np.loadtxt(path, dtype=np.float64)
  if A.shape != (4, 4):
    raise ValueError("%s: expected a 4x4 matrix, got shape %s" % (path, A.shape))
  return A


def read_color_calibration(scene_dir):
  """(color_intrinsic, depth_to_color): intrinsic/intrinsic_color.txt (required) and M = inv(extrinsic_color) extrinsic_depth in
  fp64, each extrinsic the identity where its file is absent -- a camera-space point of the depth camera times M is that point
  in the colour camera."""
  idir = os.path.join(scene_dir, "intrinsic")
  path = os.path.join(idir, "intrinsic_color.txt")
  if not os.path.exists(path):
    raise FileNotFoundError("%s: missing colour intrinsic %s" % (scene_dir, path))
  ext = {}
  for which in ("color", "depth"):
    p = os.path.join(idir, "extrinsic_%s.txt" % which)
    ext[which] = _read_4x4(p) if os.path.exists(p) else np.eye(4)
  return _read_4x4(path), np.linalg.inv(ext["color"]) @ ext["depth"]


def write_members(path, members):
  """An npz of {name: array}, stored, with a fixed zip timestamp: identical inputs give byte-identical files."""
  tmp = path + ".tmp"
  with zipfile.ZipFile(tmp, "w", compression=zipfile.ZIP_STORED, allowZip64=True) as zf:
    for name, a in members.items():
      info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
      a = np.asarray(a)  # (scalars stay 0-d)
      with zf.open(info, "w", force_zip64=True) as f:
        np.lib.format.write_array(f, a if a.flags.c_contiguous else np.ascontiguousarray(a), allow_pickle=False)
  os.replace(tmp, path)


def write_npz(path, pcd, color=None):
  """np.savez(path, pcd=pcd) with a fixed zip timestamp, so that identical inputs give byte-identical files.  color (uint8
  [n, 3]): a second member 'color' behind it; without one the file is what it was before colours existed."""
  members = dict(pcd=np.ascontiguousarray(pcd, dtype=np.float64))
  if color is not None:
    color = np.ascontiguousarray(color, dtype=np.uint8)
    if color.shape != (len(members["pcd"]), 3):
      raise ValueError("%s: color is %s for %d points" % (path, color.shape, len(members["pcd"])))
    members["color"] = color
  write_members(path, members)


def format_overlap(x):
  return "{}".format(float(x))


def pair_lines(scene, names, M):
  """`<scene>/pcd/<a>.npz <scene>/pcd/<b>.npz overlap` for every pair a < b of valid frames (frame order)."""
  n = len(names)
  out = []
  for i in range(n):
    for j in range(i + 1, n):
      out.append("%s/pcd/%s.npz %s/pcd/%s.npz %s" % (scene, names[i], scene, names[j], format_overlap(max(M[i, j], M[j, i]))))
  return out


def select_lines(lines, threshold):
  """The lines whose overlap is >= threshold (dp/generate_list.py:26)."""
  return [ln for ln in lines if float(ln.split()[2]) >= threshold]


# ---- one scene on the device ---------------------------------------------------------------------------------------
def centroids_and_overlap(vpts, voffs_np, voxel_size, dev, gpu_s):
  """What follows the points of V views, whatever made them (back-projected depth frames here, the visible vertices of a scan
  in lib/scan_views.py): vpts fp64 [n, 3] on the device, view k's rows voffs_np[k] ... voffs_np[k + 1].  Voxel centroids and
  overlap counts on the current device (the caller holds torch.cuda.device(dev)); returns dict(points, centroids, C, M) as
  process_scene documents them and adds the stages' seconds to gpu_s."""
  import torch
  from .._lib import check, lib
  from ..runtime import cur_stream, ptr, ws_args
  st = cur_stream(dev)
  V = len(voffs_np) - 1
  voffs = torch.from_numpy(voffs_np).to(dev)
  voffs_h = (C.c_int64 * (V + 1))(*voffs_np.tolist())
  n = int(voffs_np[-1])

  t0 = time.perf_counter()
  cent = torch.empty((n, 3), dtype=torch.float64, device=dev)
  coffs = torch.empty(V + 1, dtype=torch.int64, device=dev)
  coffs_h = (C.c_int64 * (V + 1))()
  ws, wsb = ws_args(lib.pcmi_corpus_voxel_centroids_workspace_bytes(n, V), dev)
  check(lib.pcmi_corpus_voxel_centroids(ptr(vpts), ptr(voffs), voffs_h, V, float(voxel_size), ptr(cent), ptr(coffs), coffs_h,
                                        ws, wsb, st))  # syncs
  gpu_s["voxel_centroids"] = time.perf_counter() - t0

  t0 = time.perf_counter()
  counts = torch.empty((V, V), dtype=torch.int32, device=dev)
  ws, wsb = ws_args(lib.pcmi_corpus_overlap_workspace_bytes(int(coffs_h[V]), V), dev)
  check(lib.pcmi_corpus_overlap_counts(ptr(cent), ptr(coffs), coffs_h, V, 1.5 * voxel_size, ptr(counts), ws, wsb, st))
  Cm = counts.cpu().numpy().astype(np.int64)  # waits for the count kernel
  gpu_s["overlap_counts"] = time.perf_counter() - t0

  t0 = time.perf_counter()
  coffs_np = np.frombuffer(coffs_h, dtype=np.int64).copy()
  pts_h = vpts.cpu().numpy()
  cent_h = cent[:coffs_np[-1]].cpu().numpy()
  gpu_s["download"] = time.perf_counter() - t0
  nv = np.diff(coffs_np)
  return dict(points=[pts_h[voffs_np[k]:voffs_np[k + 1]] for k in range(V)],
              centroids=[cent_h[coffs_np[k]:coffs_np[k + 1]] for k in range(V)],
              C=Cm, M=Cm.astype(np.float64) / nv[None, :].astype(np.float64))


def process_scene(depths, poses, intrinsic, voxel_size=0.05, depth_shift=1000.0, device=None, colors=None, color_intrinsic=None,
                  depth_to_color=None):
  """Back-projection, validity, voxel centroids and overlap counts of the F frames of one scene.

  depths: uint16 [F, H, W]; poses: [F, 4, 4] camera-to-world; intrinsic: the 4x4 depth intrinsic.  Returns a dict:
    valid [F] bool, reasons [F] str ("" or one of REASONS), dropped {reason: count}, frames (indices of the valid
    frames), points / centroids (lists of fp64 [n, 3], one per valid frame), C (int64 [V, V], zero diagonal),
    M (fp64 [V, V], C[i, j] / |D_j|), gpu_s {stage: seconds}.
  colors: uint8 [F, Hc, Wc, 3] with color_intrinsic (the 4x4 colour intrinsic) and depth_to_color (4x4, None: identity)
    adds colors (a list of uint8 [n, 3] per valid frame, aligned with points: pcmi_corpus_backproject_color's rule) and
    uncolored (int64 [F]: the points of every frame, valid or not, that no pixel of its colour image covers)."""
  import torch
  from .._lib import check, lib
  from ..runtime import cur_stream, ptr, ws_args

  depths = np.ascontiguousarray(depths, dtype=np.uint16)
  if depths.ndim != 3 or depths.shape[0] == 0:
    raise ValueError("depths must be [F, H, W] with F >= 1 (got shape %s)" % (depths.shape,))
  F, H, W = depths.shape
  poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(F, 4, 4)
  intrinsic = np.ascontiguousarray(intrinsic, dtype=np.float64).reshape(4, 4)
  dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
  gpu_s = {}
  with torch.cuda.device(dev):
    st = cur_stream(dev)
    t0 = time.perf_counter()
    d_depth = torch.from_numpy(depths.view(np.int16)).to(dev)  # the same bytes; the kernel reads uint16
    d_pose = torch.from_numpy(poses).to(dev)
    pts = torch.empty((F * H * W, 3), dtype=torch.float64, device=dev)
    offs = torch.empty(F + 1, dtype=torch.int64, device=dev)
    nan = torch.empty(F, dtype=torch.int32, device=dev)
    offs_h = (C.c_int64 * (F + 1))()
    K = (C.c_double * 16)(*intrinsic.reshape(-1).tolist())
    ws, wsb = ws_args(lib.pcmi_corpus_backproject_workspace_bytes(F, H, W), dev)
    check(lib.pcmi_corpus_backproject(ptr(d_depth), F, H, W, K, ptr(d_pose), float(depth_shift), ptr(pts), ptr(offs), ptr(nan),
                                      offs_h, ws, wsb, st))  # syncs
    gpu_s["backproject"] = time.perf_counter() - t0
    if colors is not None:
      colors = np.ascontiguousarray(colors, dtype=np.uint8)
      if colors.ndim != 4 or colors.shape[0] != F or colors.shape[3] != 3 or color_intrinsic is None:
        raise ValueError("colors must be [F, Hc, Wc, 3] for the %d depth frames, with color_intrinsic (got shape %s)" % (F, colors.shape,))
      t0 = time.perf_counter()
      Kc = (C.c_double * 16)(*np.asarray(color_intrinsic, dtype=np.float64).reshape(4, 4).reshape(-1).tolist())
      Mdc = (C.c_double * 16)(*(np.eye(4) if depth_to_color is None else np.asarray(depth_to_color, dtype=np.float64)).reshape(4, 4).reshape(-1).tolist())
      d_img = torch.from_numpy(colors).to(dev)
      col = torch.empty((F * H * W, 3), dtype=torch.uint8, device=dev)
      unc = torch.empty(F, dtype=torch.int64, device=dev)
      col_offs = torch.empty(F + 1, dtype=torch.int64, device=dev)
      ws, wsb = ws_args(lib.pcmi_corpus_backproject_color_workspace_bytes(F, H, W), dev)
      check(lib.pcmi_corpus_backproject_color(ptr(d_depth), F, H, W, K, float(depth_shift), ptr(d_img), colors.shape[1], colors.shape[2], Kc,
                                              Mdc, ptr(col), ptr(unc), ptr(col_offs), None, ws, wsb, st))  # does not wait
      unc_np = unc.cpu().numpy()  # waits for the colour kernel
      gpu_s["backproject_color"] = time.perf_counter() - t0
      del d_img
    del d_depth

    offs_np = np.frombuffer(offs_h, dtype=np.int64).copy()
    sizes = np.diff(offs_np)
    nan_np = nan.cpu().numpy()
    reasons = np.full(F, "", dtype=object)
    reasons[sizes == 0] = "empty"
    reasons[nan_np > 0] = "nan"
    reasons[~np.isfinite(poses).reshape(F, -1).all(1)] = "pose"  # the pose is checked first: its points are meaningless
    valid = reasons == ""
    frames = np.flatnonzero(valid)
    V = len(frames)
    out = dict(valid=valid, reasons=[str(r) for r in reasons], dropped={r: int((reasons == r).sum()) for r in REASONS},
               frames=frames, gpu_s=gpu_s)
    if colors is not None:
      out.update(colors=[], uncolored=unc_np)
    if V == 0:
      out.update(points=[], centroids=[], C=np.zeros((0, 0), np.int64), M=np.zeros((0, 0), np.float64))
      return out
    if V == F:
      vpts, voffs_np = pts[:offs_np[-1]], offs_np
    else:  # the valid frames' rows, contiguous
      vpts = torch.cat([pts[offs_np[f]:offs_np[f + 1]] for f in frames])
      voffs_np = np.concatenate([[0], np.cumsum(sizes[frames])]).astype(np.int64)
    if colors is not None:  # (rows as the points': the same offsets)
      col_h = col[:offs_np[-1]].cpu().numpy()
      out["colors"] = [col_h[offs_np[f]:offs_np[f + 1]] for f in frames]
      del col
    out.update(centroids_and_overlap(vpts, voffs_np, voxel_size, dev, gpu_s))
  return out


# ---- whole export ----------------------------------------------------------------------------------------------------
def _load_scene(scene_dir, frame_skip, pool, color=False):
  t0 = time.perf_counter()
  names = list_frames(scene_dir, frame_skip)
  K = read_intrinsic(scene_dir)
  poses = np.stack([read_pose(scene_dir, n) for n in names]) if names else np.zeros((0, 4, 4))
  depths = list(pool.map(read_depth, [os.path.join(scene_dir, "depth", n + ".png") for n in names]))
  shapes = {d.shape for d in depths}
  if len(shapes) > 1:
    raise ValueError("%s: depth frames of different sizes %s" % (scene_dir, sorted(shapes)))
  decode_s = time.perf_counter() - t0
  colors = None
  if color:  # (timed apart: full-size colour frames cost far more to decode than the depth)
    t0 = time.perf_counter()
    Kc, M = read_color_calibration(scene_dir)
    images = list(pool.map(read_color, [color_path(scene_dir, n) for n in names]))
    shapes = {a.shape for a in images}
    if len(shapes) > 1:
      raise ValueError("%s: colour frames of different sizes %s" % (scene_dir, sorted(shapes)))
    colors = dict(colors=np.stack(images) if images else None, color_intrinsic=Kc, depth_to_color=M, decode_s=time.perf_counter() - t0)
  return names, K, poses, (np.stack(depths) if depths else None), decode_s, colors


def build_corpus(export_root, target_root, voxel_size=0.05, threshold=0.3, frame_skip=1, scenes=None, depth_shift=1000.0,
                 device=None, io_threads=IO_THREADS, log=None, color=False):
  """Writes <target>/<scene>/pcd/<n>.npz (valid frames only), <target>/<scene>/pcd/overlap.txt and
  <target>/overlap-30-full.txt (the pairs with overlap >= threshold, scenes in sorted order).  PNG decoding of the next
  scene and npz writing of the previous one overlap the GPU work.  Returns one summary dict per scene; log (a callable)
  gets one line per scene.
  color: every npz gets a second member 'color' (uint8 [n, 3], the RGB of each point) from <scene>/color/<n>.png or .jpg,
  intrinsic/intrinsic_color.txt and, where present, intrinsic/extrinsic_color.txt and extrinsic_depth.txt; 'pcd', the overlap
  files and the list are what they are without it.  The summaries gain uncolored (points no colour pixel covers, over all
  frames of the scene) and color_decode_s."""
  if scenes is None:
    scenes = [s for s in os.listdir(export_root) if os.path.isdir(os.path.join(export_root, s, "depth"))]
  scenes = sorted(scenes)
  io_threads = max(1, min(int(io_threads), 16))
  os.makedirs(target_root, exist_ok=True)
  summaries, lines_of = [], {}
  with concurrent.futures.ThreadPoolExecutor(io_threads) as pool, concurrent.futures.ThreadPoolExecutor(1) as loader:
    lock = threading.Lock()
    write_s, writes_of = {}, {}

    def timed_write(scene, fn, *args):
      t = time.perf_counter()
      fn(*args)
      with lock:
        write_s[scene] = write_s.get(scene, 0.0) + time.perf_counter() - t

    def finish(s):  # waits for the scene's files, then reports it
      for w in writes_of.pop(s["scene"]):
        w.result()
      s["write_s"] = write_s.get(s["scene"], 0.0)
      if log is not None:
        log(_summary_line(s))

    nxt = loader.submit(_load_scene, os.path.join(export_root, scenes[0]), frame_skip, pool, color) if scenes else None
    for k, scene in enumerate(scenes):
      names, K, poses, depths, decode_s, cin = nxt.result()
      if k + 1 < len(scenes):  # the next scene decodes while this one is on the GPU
        nxt = loader.submit(_load_scene, os.path.join(export_root, scenes[k + 1]), frame_skip, pool, color)
      pdir = os.path.join(target_root, scene, "pcd")
      os.makedirs(pdir, exist_ok=True)
      if names and color:
        r = process_scene(depths, poses, K, voxel_size=voxel_size, depth_shift=depth_shift, device=device, colors=cin["colors"],
                          color_intrinsic=cin["color_intrinsic"], depth_to_color=cin["depth_to_color"])
      elif names:
        r = process_scene(depths, poses, K, voxel_size=voxel_size, depth_shift=depth_shift, device=device)
      else:
        r = dict(frames=np.zeros(0, np.int64), dropped={x: 0 for x in REASONS}, points=[], M=np.zeros((0, 0)), gpu_s={},
                 colors=[], uncolored=np.zeros(0, np.int64))
      vnames = [names[f] for f in r["frames"]]
      lines = pair_lines(scene, vnames, r["M"])
      lines_of[scene] = lines
      cols = r["colors"] if color else [None] * len(vnames)
      ws = [pool.submit(timed_write, scene, write_npz, os.path.join(pdir, name + ".npz"), p, c) for name, p, c in zip(vnames, r["points"], cols)]
      ws.append(pool.submit(timed_write, scene, _write_lines, os.path.join(pdir, "overlap.txt"), lines))
      writes_of[scene] = ws
      summaries.append(dict(scene=scene, frames=len(names), used=len(vnames), dropped=r["dropped"], pairs=len(lines),
                            over_threshold=len(select_lines(lines, threshold)), gpu_s=sum(r["gpu_s"].values()),
                            gpu_stages=r["gpu_s"], decode_s=decode_s))
      if color:
        summaries[-1].update(uncolored=int(np.sum(r["uncolored"])), color_decode_s=cin["decode_s"])
      del r
      if k > 0:  # the previous scene's files were written while this one ran
        finish(summaries[k - 1])
    if summaries:
      finish(summaries[-1])
  _write_lines(os.path.join(target_root, LIST_NAME), select_lines([ln for s in scenes for ln in lines_of[s]], threshold))
  return summaries


def _write_lines(path, lines):
  with open(path, "w") as f:
    for ln in lines:
      f.write(ln + "\n")


def _summary_line(s):
  d = s["dropped"]
  line = ("%s: %d frames, %d used, dropped %d (pose %d, nan %d, empty %d), %d pairs, %d >= threshold, gpu %.3f s, "
          "png decode %.3f s, npz write %.3f s" %
          (s["scene"], s["frames"], s["used"], sum(d.values()), d["pose"], d["nan"], d["empty"], s["pairs"],
           s["over_threshold"], s["gpu_s"], s["decode_s"], s["write_s"]))
  if "uncolored" in s:
    line += ", uncolored %d, colour decode %.3f s" % (s["uncolored"], s["color_decode_s"])
  return line
