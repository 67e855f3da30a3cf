"""numpy restatement of the two colour rules of include/pcmi.h, written from the header: pcmi_corpus_backproject_color (a colour
for every back-projected point) and pcmi_pair_color_features (the batch features from those colours).  Every fp64 operation
below is one IEEE operation on arrays, in the header's order (numpy does not contract a * b + c into an FMA); the tests compare
the device output with this bit for bit."""
import numpy as np


def self_coding_image(height, width):
  """uint8 [height, width, 3] whose pixel (x, y) says where it is: r = x % 256, g = y % 256, b = x // 256 + 16 (y // 256)."""
  y, x = np.divmod(np.arange(height * width, dtype=np.int64), width)
  return np.stack([x % 256, y % 256, x // 256 + 16 * (y // 256)], 1).astype(np.uint8).reshape(height, width, 3)


def pixel_of(color):
  """The (x, y) a self_coding_image colour stands for (images below 4096 x 4096)."""
  c = np.asarray(color, np.int64)
  return c[..., 0] + 256 * (c[..., 2] % 16), c[..., 1] + 256 * (c[..., 2] // 16)


def project(depth, intrinsic, color_intrinsic, depth_to_color=None, depth_shift=1000.0):
  """One frame, the pixels with depth != 0 in row-major order: (uc, vc, q2, px, py, hit) of the header's rule."""
  K, Kc = np.asarray(intrinsic, np.float64).reshape(4, 4), np.asarray(color_intrinsic, np.float64).reshape(4, 4)
  M = np.eye(4) if depth_to_color is None else np.asarray(depth_to_color, np.float64).reshape(4, 4)
  fx, fy, cx, cy, bx, by = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 3], K[1, 3]
  fxc, fyc, cxc, cyc = Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]
  H, W = depth.shape
  v, u = np.divmod(np.arange(H * W, dtype=np.int64), W)
  raw = np.asarray(depth).reshape(-1)
  keep = raw != 0
  u, v = u[keep].astype(np.float64), v[keep].astype(np.float64)
  with np.errstate(all="ignore"):
    d = raw[keep].astype(np.float64) / np.float64(depth_shift)
    X = ((u - cx) * d) / fx + bx
    Y = ((v - cy) * d) / fy + by
    q = [((X * M[r, 0] + Y * M[r, 1]) + d * M[r, 2]) + M[r, 3] for r in range(3)]
    uc = (fxc * q[0]) / q[2] + cxc
    vc = (fyc * q[1]) / q[2] + cyc
    px, py = np.floor(uc + 0.5), np.floor(vc + 0.5)
  return uc, vc, q[2], px, py


def backproject_color_ref(depths, intrinsic, colors, color_intrinsic, depth_to_color=None, depth_shift=1000.0):
  """depths uint16 [F, H, W], colors uint8 [F, Hc, Wc, 3] -> (color uint8 [n, 3] in pcmi_corpus_backproject's row order, uncolored
  int64 [F], offsets int64 [F + 1])."""
  depths, colors = np.asarray(depths), np.asarray(colors)
  F, (Hc, Wc) = len(depths), colors.shape[1:3]
  out, uncolored, offsets = [], np.zeros(F, np.int64), np.zeros(F + 1, np.int64)
  for f in range(F):
    uc, vc, q2, px, py = project(depths[f], intrinsic, color_intrinsic, depth_to_color, depth_shift)
    with np.errstate(all="ignore"):  # decided on the doubles; only the hits are converted
      hit = (q2 > 0) & np.isfinite(uc) & np.isfinite(vc) & (px >= 0) & (px < Wc) & (py >= 0) & (py < Hc)
    c = np.zeros((len(uc), 3), np.uint8)
    c[hit] = colors[f][py[hit].astype(np.int64), px[hit].astype(np.int64)]
    out.append(c)
    uncolored[f] = int((~hit).sum())
    offsets[f + 1] = offsets[f] + len(c)
  return np.concatenate(out) if out else np.zeros((0, 3), np.uint8), uncolored, offsets


def features_of(color_rows, on, noise_rows, mu, sigma):
  """fp32((c / 255 - 0.5) + (mu + sigma z)) with jitter, fp32(c / 255 - 0.5) without; rows already gathered."""
  v = np.asarray(color_rows, np.uint8).astype(np.float64) / np.float64(255.0) - np.float64(0.5)
  if on and noise_rows is not None:
    v = v + (np.float64(mu) + np.float64(sigma) * np.asarray(noise_rows, np.float32).astype(np.float64))
  return v.astype(np.float32)


def color_features_ref(color, vox, noise=None, jitter_on=None, mu=0.0, sigma=0.01, out_rows=None, sentinel=None):
  """pcmi_pair_color_features on pair_voxelize's result `vox` (tests/pair_input_ref.pair_voxelize's dict, or the device's as
  numpy): (F0, F1).  out_rows / sentinel: buffers of out_rows rows filled with `sentinel` first, rows outside them not written
  (None: exactly the rows of each side)."""
  voff, side, first = np.asarray(vox["vox_offsets"]), np.asarray(vox["side_offsets"]), np.asarray(vox["first_index"])
  B = side.shape[1] - 1
  color = np.asarray(color, np.uint8)
  out = []
  for s in range(2):
    rows = int(side[s, B]) if out_rows is None else int(out_rows)
    F = np.full((rows, 3), 0.0 if sentinel is None else sentinel, np.float32)
    for b in range(B):
      c = 2 * b + s
      idx = first[voff[c]:voff[c + 1]]
      on = noise is not None and jitter_on is not None and bool(jitter_on[c])
      vals = features_of(color[idx], on, None if noise is None else np.asarray(noise)[idx], mu, sigma)
      dst = int(side[s, b]) + np.arange(len(idx))
      ok = dst < rows
      F[dst[ok]] = vals[ok]
    out.append(F)
  return out[0], out[1]
