"""The pre-training pair corpus from whole scans: virtual depth views of a reconstruction, on the device.

lib/pair_corpus.py needs posed depth frames; a user who holds only reconstructions (ScanNet's _vh_clean_2.ply meshes without
the .sens streams, S3DIS rooms, Matterport, a LiDAR or photogrammetry scan) has none.  Here one scan becomes many partial
views the way a pinhole depth camera would see it: every vertex through every virtual camera, frustum plus z-buffer
occlusion (csrc/views.hip; the rule is stated in include/pcmi.h and restated in numpy in tests/views_ref.py).  A view's
points are the scan's own vertices that the camera sees -- xyz[rows], nothing quantised or snapped to a pixel -- so the
correspondences between two views are exact.  Everything after that is pair_corpus.py's, unchanged: voxel centroids, overlap
counts, pair_lines, select_lines, write_npz and the list ScanNetMatchPairDataset reads.

  ViewDraws                                    the random quantities of a scan's cameras, as data;
  render_views(xyz, poses, intrinsic, H, W)    visible rows, offsets and coverage of every camera;
  process_scan(xyz, poses, intrinsic, H, W)    process_scene's dict for the views of one scan;
  build_corpus_from_scans(scan_root, target)   <scene>.npz / .npy / .ply (or ScanNet's <scene>/<scene>_vh_clean_2.ply) in,
                                               <target>/<scene>/pcd/<k>.npz, <target>/<scene>/pcd/overlap.txt,
                                               <target>/<scene>/views.npz and <target>/overlap-30-full.txt out.

This has no counterpart in the reference.  The camera model and every default (n_views 64, 240 x 320 pixels, fx = fy = 288,
splat 3, rel_tol 0.05, z_near 0.1, z_far 10, cameras 1.0 ... 1.8 m above the lowest point pitched -30 ... 0 degrees, coverage
at least 0.5) are this project's choice and have NOT been tuned; nobody has measured whether a corpus built this way
pre-trains as well as one built from recorded frames."""
import concurrent.futures
import math
import os
import threading
import time
import zlib

import numpy as np

from . import pair_corpus as pc

REASONS = ("pose", "empty", "coverage")
INSET = 0.3  # metres a camera stands inside the scan's bounding box


# ---- cameras -----------------------------------------------------------------------------------------------------------
def camera_pose(position, yaw, pitch, up_axis=2):
  """Camera-to-world 4x4 with the columns x right, y down, z forward (ScanNet's pose convention).  With (a, b, up) the
  right-handed cyclic order of the axes: forward = cos(pitch) (cos(yaw) e_a + sin(yaw) e_b) + sin(pitch) e_up,
  right = sin(yaw) e_a - cos(yaw) e_b, down = forward x right."""
  a, b = (up_axis + 1) % 3, (up_axis + 2) % 3
  fwd, right = np.zeros(3), np.zeros(3)
  fwd[a], fwd[b], fwd[up_axis] = math.cos(pitch) * math.cos(yaw), math.cos(pitch) * math.sin(yaw), math.sin(pitch)
  right[a], right[b] = math.sin(yaw), -math.cos(yaw)
  P = np.eye(4)
  P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = right, np.cross(fwd, right), fwd, position
  return P


class ViewDraws:
  """The random quantities of a scan's F cameras: index int64 [F] (a scan point each), u_height, u_yaw, u_pitch float64 [F]
  uniform in [0, 1), with the parameters they are read under (up_axis, height and pitch_deg ranges).  poses(xyz) is the
  formula: the camera stands above the chosen point's position in the two ground axes, clipped to INSET inside the bounding
  box of the scan's finite points (the middle where the box is narrower than 2 INSET), at min(up) + height[0] + u_height
  (height[1] - height[0]); yaw = 2 pi u_yaw, pitch = radians(pitch_deg[0] + u_pitch (pitch_deg[1] - pitch_deg[0])); the
  matrix is camera_pose's.  The defaults are untuned."""

  def __init__(self, index, u_height, u_yaw, u_pitch, up_axis=2, height=(1.0, 1.8), pitch_deg=(-30.0, 0.0)):
    self.index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
    F = self.index.shape[0]
    self.u_height, self.u_yaw, self.u_pitch = (np.ascontiguousarray(u, dtype=np.float64).reshape(F) for u in (u_height, u_yaw, u_pitch))
    if up_axis not in (0, 1, 2):
      raise ValueError("up_axis must be 0, 1 or 2 (got %r)" % (up_axis,))
    self.up_axis = int(up_axis)
    self.height = (float(height[0]), float(height[1]))
    self.pitch_deg = (float(pitch_deg[0]), float(pitch_deg[1]))

  @property
  def n_views(self):
    return self.index.shape[0]

  @classmethod
  def sample(cls, rng, xyz, n_views, up_axis=2, height=(1.0, 1.8), pitch_deg=(-30, 0)):
    """rng: a np.random.RandomState of the caller's.  One randint(0, n) per view, then the three uniforms of every view."""
    n = np.asarray(xyz).shape[0]
    if n < 1 or n_views < 0:
      raise ValueError("ViewDraws.sample: %d points, %d views" % (n, n_views))
    index = rng.randint(0, n, size=n_views)
    u = rng.random_sample((3, n_views))
    return cls(index, u[0], u[1], u[2], up_axis=up_axis, height=height, pitch_deg=pitch_deg)

  def poses(self, xyz):
    xyz = np.asarray(xyz, dtype=np.float64)
    fin = xyz[np.isfinite(xyz).all(1)]
    if len(fin) == 0:
      raise ValueError("ViewDraws.poses: the scan has no finite point")
    lo, hi = fin.min(0), fin.max(0)
    out = np.zeros((self.n_views, 4, 4))
    for f in range(self.n_views):
      pos = np.array(xyz[self.index[f]], dtype=np.float64)
      for a in range(3):
        if a == self.up_axis:
          pos[a] = lo[a] + self.height[0] + self.u_height[f] * (self.height[1] - self.height[0])
        elif hi[a] - lo[a] < 2 * INSET or not np.isfinite(pos[a]):
          pos[a] = 0.5 * (lo[a] + hi[a])
        else:
          pos[a] = min(max(pos[a], lo[a] + INSET), hi[a] - INSET)
      yaw = 2.0 * math.pi * self.u_yaw[f]
      pitch = math.radians(self.pitch_deg[0] + self.u_pitch[f] * (self.pitch_deg[1] - self.pitch_deg[0]))
      out[f] = camera_pose(pos, yaw, pitch, self.up_axis)
    return out

  def members(self):
    return dict(draw_index=self.index, draw_u_height=self.u_height, draw_u_yaw=self.u_yaw, draw_u_pitch=self.u_pitch,
                up_axis=np.int64(self.up_axis), height_range=np.array(self.height), pitch_deg_range=np.array(self.pitch_deg))

  @classmethod
  def from_members(cls, z):
    """From a views.npz (or any mapping with members()' keys)."""
    return cls(z["draw_index"], z["draw_u_height"], z["draw_u_yaw"], z["draw_u_pitch"], up_axis=int(z["up_axis"]),
               height=tuple(z["height_range"]), pitch_deg=tuple(z["pitch_deg_range"]))


def pinhole_intrinsic(height, width, focal):
  """4x4, fx = fy = focal, the principal point at the image's centre ((W - 1) / 2, (H - 1) / 2)."""
  K = np.eye(4)
  K[0, 0] = K[1, 1] = float(focal)
  K[0, 2], K[1, 2] = (width - 1) / 2.0, (height - 1) / 2.0
  return K


def world_to_camera(poses):
  """np.linalg.inv of every camera-to-world pose, one at a time, in fp64 on the host; a pose with a non-finite entry gives
  a matrix of NaNs (no point is projectable through it).  A singular finite pose is a ValueError."""
  poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
  out = np.full(poses.shape, np.nan)
  for f, P in enumerate(poses):
    if np.isfinite(P).all():
      try:
        out[f] = np.linalg.inv(P)
      except np.linalg.LinAlgError:
        raise ValueError("pose %d is singular:\n%s" % (f, P)) from None
  return out


# ---- one scan on the device --------------------------------------------------------------------------------------------
def _render(d_xyz, poses, intrinsic, H, W, z_near, z_far, splat, rel_tol, gpu_s):
  import torch
  from .. import functional as PF
  K = np.asarray(intrinsic, dtype=np.float64)
  if K.shape not in ((3, 3), (4, 4)):
    raise ValueError("intrinsic must be 3x3 or 4x4 (got shape %s)" % (K.shape,))
  fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
  t0 = time.perf_counter()
  d_w2c = torch.from_numpy(world_to_camera(poses)).to(d_xyz.device)
  zbuf = PF.view_zbuffer(d_xyz, d_w2c, fx, fy, cx, cy, H, W, z_near=z_near, z_far=z_far, splat=splat)
  rows, offsets, offs_np, pixels, _ = PF.view_visible(d_xyz, d_w2c, fx, fy, cx, cy, zbuf, z_near=z_near, z_far=z_far, rel_tol=rel_tol)
  pixels_np = pixels.cpu().numpy()  # waits for the compaction too
  gpu_s["views"] = time.perf_counter() - t0
  return rows, offs_np, pixels_np


def render_views(xyz, poses, intrinsic, H, W, z_near=0.1, z_far=10.0, splat=3, rel_tol=0.05, device=None):
  """xyz fp64 [n, 3] (world frame), poses [F, 4, 4] camera-to-world, intrinsic 3x3 or 4x4 -> dict(rows int32 [total], the
  visible scan rows of every view, ascending; offsets int64 [F + 1]; pixels int64 [F]; coverage fp64 [F] = pixels / (H W);
  gpu_s {stage: seconds})."""
  import torch
  xyz = np.ascontiguousarray(xyz, dtype=np.float64)
  if xyz.ndim != 2 or xyz.shape[1] != 3:
    raise ValueError("xyz must be [n, 3] (got shape %s)" % (xyz.shape,))
  dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
  gpu_s = {}
  with torch.cuda.device(dev):
    rows, offs_np, pixels = _render(torch.from_numpy(xyz).to(dev), poses, intrinsic, H, W, z_near, z_far, splat, rel_tol, gpu_s)
    rows = rows.cpu().numpy()
  return dict(rows=rows, offsets=offs_np, pixels=pixels, coverage=pixels.astype(np.float64) / np.float64(H * W), gpu_s=gpu_s)


def process_scan(xyz, poses, intrinsic, H, W, z_near=0.1, z_far=10.0, splat=3, rel_tol=0.05, color=None, voxel_size=0.05,
                 min_coverage=0.5, device=None):
  """The views of one scan through the corpus stages.  Returns process_scene's dict -- valid [F] bool, reasons [F] str ("" or
  one of REASONS), dropped {reason: count}, frames (indices of the kept views), points / centroids (lists of fp64 [n, 3], one
  per kept view), C, M, gpu_s -- plus rows (a list of int32 arrays: the scan rows of every kept view, points[k] = xyz[rows[k]]
  exactly), coverage fp64 [F] and, with color (uint8 [n, 3]), colors (color[rows[k]]).
  A view is dropped for a pose with a non-finite entry ("pose"), for no visible row ("empty"), or for fewer than
  min_coverage of its pixels holding a depth ("coverage"), checked in that order."""
  import torch
  xyz = np.ascontiguousarray(xyz, dtype=np.float64)
  if xyz.ndim != 2 or xyz.shape[1] != 3:
    raise ValueError("xyz must be [n, 3] (got shape %s)" % (xyz.shape,))
  poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
  F = poses.shape[0]
  if color is not None:
    color = np.ascontiguousarray(color, dtype=np.uint8)
    if color.shape != xyz.shape:
      raise ValueError("color is %s for xyz %s" % (color.shape, xyz.shape))
  dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
  gpu_s = {}
  with torch.cuda.device(dev):
    d_xyz = torch.from_numpy(xyz).to(dev)
    d_rows, offs_np, pixels = _render(d_xyz, poses, intrinsic, H, W, z_near, z_far, splat, rel_tol, gpu_s)
    coverage = pixels.astype(np.float64) / np.float64(H * W)
    sizes = np.diff(offs_np)
    reasons = np.full(F, "", dtype=object)
    reasons[coverage < min_coverage] = "coverage"
    reasons[sizes == 0] = "empty"
    reasons[~np.isfinite(poses).reshape(F, -1).all(1)] = "pose"
    valid = reasons == ""
    frames = np.flatnonzero(valid)
    V = len(frames)
    out = dict(valid=valid, reasons=[str(r) for r in reasons], dropped={r: int((reasons == r).sum()) for r in REASONS},
               frames=frames, coverage=coverage, gpu_s=gpu_s)
    if V == 0:
      out.update(rows=[], points=[], centroids=[], C=np.zeros((0, 0), np.int64), M=np.zeros((0, 0), np.float64))
      if color is not None:
        out["colors"] = []
      return out
    vrows = d_rows if V == F else torch.cat([d_rows[offs_np[f]:offs_np[f + 1]] for f in frames])
    voffs_np = np.concatenate([[0], np.cumsum(sizes[frames])]).astype(np.int64)
    vpts = d_xyz.index_select(0, vrows.long())  # the scan's own vertices, bit for bit
    rows_h = vrows.cpu().numpy()
    out.update(pc.centroids_and_overlap(vpts, voffs_np, voxel_size, dev, gpu_s))
  out["rows"] = [rows_h[voffs_np[k]:voffs_np[k + 1]] for k in range(V)]
  if color is not None:
    out["colors"] = [color[r] for r in out["rows"]]
  return out


# ---- scans on disk -----------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_vertices(path):
  """(xyz float64 [n, 3], color uint8 [n, 3] or None) of a PLY file's `vertex` element: format ascii or binary_little_endian
  1.0; the properties x, y, z and, if all three are there, red, green, blue (uchar); every other scalar property is skipped by
  its declared size, other elements are not read.  Anything else -- another format, a list property in or before the vertex
  element, an unknown type, a short file -- is a ValueError that says what was found."""
  with open(path, "rb") as f:
    data = f.read()
  end = data.find(b"end_header")
  if not data.startswith(b"ply") or end < 0:
    raise ValueError("%s: not a PLY file (no 'ply' ... 'end_header' header)" % path)
  nl = data.find(b"\n", end)
  if nl < 0:
    raise ValueError("%s: the header's last line does not end" % path)
  body = nl + 1
  fmt, elements = None, []  # elements: [name, count, [(property, dtype or None for a list)]]
  for raw in data[:end].decode("ascii", "replace").splitlines()[1:]:
    tok = raw.split()
    if not tok or tok[0] in ("comment", "obj_info"):
      continue
    if tok[0] == "format":
      fmt = " ".join(tok[1:])
    elif tok[0] == "element" and len(tok) == 3:
      elements.append([tok[1], int(tok[2]), []])
    elif tok[0] == "property" and elements:
      if tok[1] == "list":
        elements[-1][2].append((tok[-1], None))
      elif len(tok) == 3 and tok[1] in _PLY_TYPES:
        elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
      else:
        raise ValueError("%s: property of unknown type %r" % (path, raw))
    else:
      raise ValueError("%s: header line %r" % (path, raw))
  if fmt not in ("ascii 1.0", "binary_little_endian 1.0"):
    raise ValueError("%s: format %r (ascii 1.0 and binary_little_endian 1.0 are read)" % (path, fmt))
  k = next((i for i, e in enumerate(elements) if e[0] == "vertex"), None)
  if k is None:
    raise ValueError("%s: no vertex element (elements: %s)" % (path, [e[0] for e in elements]))
  for name, _, props in elements[:k + 1]:
    lists = [p for p, t in props if t is None]
    if lists:
      raise ValueError("%s: list property %r in element %r, at or before the vertices" % (path, lists[0], name))
  _, n, props = elements[k]
  names = [p for p, _ in props]
  if len(set(names)) != len(names) or not all(a in names for a in "xyz"):
    raise ValueError("%s: vertex properties %s (x, y and z are needed, each once)" % (path, names))
  has_color = all(c in names for c in ("red", "green", "blue"))
  if has_color and any(t != "u1" for p, t in props if p in ("red", "green", "blue")):
    raise ValueError("%s: red, green, blue of types %s (uchar is read)" % (path, [t for p, t in props if p in ("red", "green", "blue")]))
  if fmt.startswith("binary"):
    skip = sum(c * sum(np.dtype(t).itemsize for _, t in pr) for _, c, pr in elements[:k])
    dt = np.dtype([(p, "<" + t) for p, t in props])
    if len(data) < body + skip + n * dt.itemsize:
      raise ValueError("%s: %d bytes after the header, %d vertices of %d bytes need %d" % (path, len(data) - body, n, dt.itemsize,
                                                                                          skip + n * dt.itemsize))
    v = np.frombuffer(data, dtype=dt, count=n, offset=body + skip)
    col = lambda p: v[p]
  else:
    lines = data[body:].decode("ascii", "replace").splitlines()
    skip = sum(c for _, c, _ in elements[:k])
    if len(lines) < skip + n:
      raise ValueError("%s: %d lines after the header, %d vertices need %d" % (path, len(lines), n, skip + n))
    try:
      tab = np.array([ln.split() for ln in lines[skip:skip + n]], dtype=np.float64).reshape(n, -1)
    except ValueError:
      raise ValueError("%s: a vertex line is not %d numbers" % (path, len(props))) from None
    if tab.shape[1] != len(props):
      raise ValueError("%s: vertex lines of %d numbers for %d properties" % (path, tab.shape[1], len(props)))
    col = lambda p: tab[:, names.index(p)]
  xyz = np.stack([np.asarray(col(a), dtype=np.float64) for a in "xyz"], 1) if n else np.zeros((0, 3))
  color = None
  if has_color:
    color = np.stack([np.asarray(col(c)).astype(np.uint8) for c in ("red", "green", "blue")], 1) if n else np.zeros((0, 3), np.uint8)
  return np.ascontiguousarray(xyz), color


def list_scans(scan_root):
  """{scene: path} of the scans under scan_root: <scene>.npz, <scene>.npy, <scene>.ply and <scene>/<scene>_vh_clean_2.ply."""
  out = {}
  for name in sorted(os.listdir(scan_root)):
    path = os.path.join(scan_root, name)
    stem, ext = os.path.splitext(name)
    if os.path.isfile(path) and ext in (".npz", ".npy", ".ply"):
      if stem in out:
        raise ValueError("%s: scene %s is there twice (%s and %s)" % (scan_root, stem, os.path.basename(out[stem]), name))
      out[stem] = path
    elif os.path.isdir(path) and os.path.isfile(os.path.join(path, name + "_vh_clean_2.ply")):
      if name in out:
        raise ValueError("%s: scene %s is there twice (%s and %s/)" % (scan_root, name, os.path.basename(out[name]), name))
      out[name] = os.path.join(path, name + "_vh_clean_2.ply")
  return out


def read_scan(path):
  """(xyz float64 [n, 3], color uint8 [n, 3] or None) from .npz (xyz, optionally color), .npy ([n, 3] or [n, 6], the last three
  columns colours 0 ... 255) or .ply."""
  ext = os.path.splitext(path)[1]
  if ext == ".ply":
    xyz, color = read_ply_vertices(path)
  elif ext == ".npz":
    with np.load(path) as z:
      if "xyz" not in z.files:
        raise ValueError("%s: no member 'xyz' (members: %s)" % (path, z.files))
      xyz, color = z["xyz"], (z["color"] if "color" in z.files else None)
  elif ext == ".npy":
    a = np.load(path)
    if a.ndim != 2 or a.shape[1] not in (3, 6):
      raise ValueError("%s: an array of shape %s ([n, 3] or [n, 6] is read)" % (path, a.shape))
    xyz, color = a[:, :3], (a[:, 3:] if a.shape[1] == 6 else None)
  else:
    raise ValueError("%s: not a .npz, .npy or .ply scan" % path)
  xyz = np.ascontiguousarray(xyz, dtype=np.float64)
  if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
    raise ValueError("%s: xyz of shape %s ([n, 3] with n >= 1 is needed)" % (path, xyz.shape))
  if color is not None:
    color = np.asarray(color)
    if color.shape != xyz.shape or (color.dtype != np.uint8 and (color.min() < 0 or color.max() > 255)):
      raise ValueError("%s: colours of shape %s, dtype %s for %d points (values 0 ... 255)" % (path, color.shape, color.dtype, len(xyz)))
    color = np.ascontiguousarray(color.astype(np.uint8))
  return xyz, color


def scene_rng(seed, scene):
  """The generator of one scene's draws: seeded by (seed, crc32 of the scene's name), so a scene's cameras do not depend on
  which other scenes are built with it."""
  return np.random.RandomState([int(seed) & 0xffffffff, zlib.crc32(scene.encode("utf-8"))])


def _load_scan(path, scene, n_views, seed, up_axis, cam_height, pitch_deg):
  t0 = time.perf_counter()
  xyz, color = read_scan(path)
  draws = ViewDraws.sample(scene_rng(seed, scene), xyz, n_views, up_axis=up_axis, height=cam_height, pitch_deg=pitch_deg)
  return xyz, color, draws, draws.poses(xyz), time.perf_counter() - t0


def build_corpus_from_scans(scan_root, target_root, n_views=64, seed=0, height=240, width=320, focal=288.0, z_near=0.1, z_far=10.0,
                            splat=3, rel_tol=0.05, min_coverage=0.5, voxel_size=0.05, threshold=0.3, scenes=None, up_axis=2,
                            cam_height=(1.0, 1.8), pitch_deg=(-30, 0), device=None, io_threads=pc.IO_THREADS, log=None):
  """Writes, for every scan under scan_root (list_scans; scenes: a subset of their names), <target>/<scene>/pcd/<k>.npz for
  every kept view k ('pcd', and 'color' when the scan has colours), <target>/<scene>/pcd/overlap.txt, <target>/<scene>/views.npz
  (poses, intrinsic, the parameters, the draws, every view's reason and coverage: enough to build the scene again) and
  <target>/overlap-30-full.txt (the pairs with overlap >= threshold, scenes in sorted order).  Reading the next scan and
  writing the previous one's files overlap the GPU work, as in build_corpus.  The same seed gives byte-identical files.
  Returns one summary dict per scene; log (a callable) gets one line per scene.  The defaults are untuned (module docstring)."""
  found = list_scans(scan_root)
  if scenes is None:
    scenes = list(found)
  missing = [s for s in scenes if s not in found]
  if missing:
    raise FileNotFoundError("%s: no scan for %s (found: %s)" % (scan_root, missing, sorted(found)))
  scenes = sorted(scenes)
  io_threads = max(1, min(int(io_threads), 16))
  os.makedirs(target_root, exist_ok=True)
  K = pinhole_intrinsic(height, width, focal)
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

    def load(scene):
      return loader.submit(_load_scan, found[scene], scene, n_views, seed, up_axis, cam_height, pitch_deg)

    nxt = load(scenes[0]) if scenes else None
    for k, scene in enumerate(scenes):
      xyz, color, draws, poses, decode_s = nxt.result()
      if k + 1 < len(scenes):  # the next scan is read while this one is on the GPU
        nxt = load(scenes[k + 1])
      pdir = os.path.join(target_root, scene, "pcd")
      os.makedirs(pdir, exist_ok=True)
      r = process_scan(xyz, poses, K, height, width, z_near=z_near, z_far=z_far, splat=splat, rel_tol=rel_tol, color=color,
                       voxel_size=voxel_size, min_coverage=min_coverage, device=device)
      vnames = [str(int(f)) for f in r["frames"]]
      lines = pc.pair_lines(scene, vnames, r["M"])
      lines_of[scene] = lines
      cols = r["colors"] if color is not None else [None] * len(vnames)
      ws = [pool.submit(timed_write, scene, pc.write_npz, os.path.join(pdir, name + ".npz"), p, c)
            for name, p, c in zip(vnames, r["points"], cols)]
      ws.append(pool.submit(timed_write, scene, pc._write_lines, os.path.join(pdir, "overlap.txt"), lines))
      members = dict(poses=poses, intrinsic=K, image_size=np.array([height, width], np.int64), z_range=np.array([z_near, z_far]),
                     splat=np.int64(splat), rel_tol=np.float64(rel_tol), min_coverage=np.float64(min_coverage),
                     voxel_size=np.float64(voxel_size), seed=np.int64(seed), reasons=np.array(r["reasons"], dtype="U8"),
                     coverage=r["coverage"], **draws.members())
      ws.append(pool.submit(timed_write, scene, pc.write_members, os.path.join(target_root, scene, "views.npz"), members))
      writes_of[scene] = ws
      summaries.append(dict(scene=scene, points=len(xyz), frames=n_views, used=len(vnames), dropped=r["dropped"], pairs=len(lines),
                            over_threshold=len(pc.select_lines(lines, threshold)), gpu_s=sum(r["gpu_s"].values()),
                            gpu_stages=r["gpu_s"], decode_s=decode_s))
      del r
      if k > 0:  # the previous scene's files were written while this one ran
        finish(summaries[k - 1])
    if summaries:
      finish(summaries[-1])
  pc._write_lines(os.path.join(target_root, pc.LIST_NAME), pc.select_lines([ln for s in scenes for ln in lines_of[s]], threshold))
  return summaries


def _summary_line(s):
  d = s["dropped"]
  return ("%s: %d points, %d views, %d used, dropped %d (pose %d, empty %d, coverage %d), %d pairs, %d >= threshold, gpu %.3f s, "
          "scan read %.3f s, npz write %.3f s" % (s["scene"], s["points"], s["frames"], s["used"], sum(d.values()), d["pose"], d["empty"],
                                                  d["coverage"], s["pairs"], s["over_threshold"], s["gpu_s"], s["decode_s"], s["write_s"]))
