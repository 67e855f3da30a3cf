"""Pre-training batches built on the device, one call per batch (csrc/pair_input.hip; include/pcmi.h "The input of contrastive
pre-training"): what ScanNetMatchPairDataset.__getitem__ and default_collate_pair_fn (lib/ddp_data_loaders.py, the reference's
pc/lib/ddp_data_loaders.py:52-112, :196-265) do item by item on the host -- scale, rotation about the centroid, first-occurrence
voxelisation, correspondences within the search radius, feature jitter, collation -- for the raw frames of a whole batch.

  PairDraws          every random quantity of a batch, drawn on the host in the dataset's order (or the identity);
  PairInputPipeline  raw frames + draws -> the collate's dict as DEVICE tensors: one upload, one blocking read-back;
  DevicePairLoader   the loader behind data.device_batch=True: DataLoader workers only read the npz files, the training
                     process draws and runs the pipeline.

Differences from the host loader (INTEGRATION.md "Loader"): the centroid and T1 inv(T0) are evaluated in the fixed order pcmi.h
states (numpy's mean, linalg.inv and @ may differ in the last bits); the jitter noise comes from a torch.Generator and belongs
to the voxel's first RAW point; a flagged pair raises."""
import os
import random

import numpy as np
import torch
import torch.utils.data

from .. import functional as PF
from .._lib import PcmiError
from . import synthetic
from .data_sampler import DistributedInfSampler, InfSampler


class PairDraws:
  """The random quantities of one batch of B pairs: scale float64 [B] (1 where the dataset does not scale), rot float64
  [2 B, 3, 3] (cloud 2 b, cloud 2 b + 1), jitter_on bool [2 B], and the standard normals of the feature jitter: `noise` (float32
  [n_raw, 3], one row per raw point of the batch) or a torch.Generator to draw them with."""

  def __init__(self, scale, rot, jitter_on, noise=None, generator=None):
    self.scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
    B = self.scale.shape[0]
    self.rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(2 * B, 3, 3)
    self.jitter_on = np.ascontiguousarray(jitter_on).astype(bool).reshape(2 * B)
    self.noise, self.generator = noise, generator

  @property
  def n_pairs(self):
    return self.scale.shape[0]

  @classmethod
  def identity(cls, n_pairs):
    return cls(np.ones(n_pairs), np.tile(np.eye(3), (2 * n_pairs, 1, 1)), np.zeros(2 * n_pairs, bool))

  @classmethod
  def sample(cls, config, n_pairs, randg, generator=None, jitter_p=0.95):
    """Draws as ScanNetMatchPairDataset.__getitem__ does, item by item: from `random` the scale coin and the scale
    (trainer.use_random_scale), from `randg` rand(3) and rand(1) for T0, then for T1 (trainer.use_random_rotation;
    synthetic._rotation's closed form), then from `random` FeatureJitter's two coins."""
    tr = config.trainer
    scale, rot, on = np.ones(n_pairs), np.tile(np.eye(3), (2 * n_pairs, 1, 1)), np.zeros(2 * n_pairs, bool)
    for b in range(n_pairs):
      if tr.use_random_scale and random.random() < 0.95:
        scale[b] = tr.min_scale + (tr.max_scale - tr.min_scale) * random.random()
      if tr.use_random_rotation:
        for s in range(2):
          axis = randg.rand(3) - 0.5
          rot[2 * b + s] = synthetic._rotation(axis, tr.rotation_range * np.pi / 180.0 * (randg.rand(1)[0] - 0.5))
      for s in range(2):
        on[2 * b + s] = random.random() < jitter_p
    return cls(scale, rot, on, generator=generator)


class PairInputPipeline:
  """frames: a list of (xyz0, xyz1) raw arrays [n, 3] (float32 or float64, as the npz stores them); draws: a PairDraws.
  Returns the collate's dict as device tensors -- pcd0, pcd1, sinput0_C, sinput0_F, sinput1_C, sinput1_F, correspondences, T_gt
  -- with len_batch (a host list, from the read-back) and n_queries (the distinct values of column 0 of the correspondences).
  The tensors are views of buffers sized for the raw rows.  jitter = (mu, sigma) of the feature noise, None: features are 1.
  Frames of a corpus built with colours are (xyz0, xyz1, rgb0, rgb1), rgb uint8 [n, 3] -- all frames of a batch or none: the
  features are then rgb / 255 - 0.5 of the voxel's first point (+ the noise), as ScanNetMatchPairDataset's with data.use_color.
  One upload (raw rows, colours and draws in one buffer), one blocking read-back (counts, flags, n_queries); a second one when the
  correspondences did not fit match_capacity and the fill ran again (last_readbacks)."""

  def __init__(self, voxel_size, search_multiplier, random_rotation=True, device=None, jitter=(0.0, 0.01), match_capacity=None):
    self.voxel_size, self.search_multiplier = float(voxel_size), float(search_multiplier)
    self.random_rotation, self.jitter = bool(random_rotation), jitter
    self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    self.match_capacity = match_capacity  # None: 16 rows per raw point for the first batch, then what the batches needed (+ 25 %)
    self.last_readbacks = 0
    self._staging, self._staging_event = None, None

  def _upload(self, sections, rows, row_dtype):
    """The byte sections (numpy arrays, each a multiple of 8 bytes) and, behind them, the clouds `rows` ([n_c, 3] each, stored as
    row_dtype) as ONE host -> device copy through a persistent pinned buffer; returns the device views in order, the
    concatenated rows last."""
    sizes = [a.nbytes for a in sections]
    head, n = sum(sizes), sum(a.shape[0] for a in rows)
    row_bytes = 3 * np.dtype(row_dtype).itemsize
    total = max(head + n * row_bytes, 8)
    if self._staging is None or self._staging.numel() < total:
      self._staging, self._staging_event = torch.empty(int(total * 1.25) + 4096, dtype=torch.uint8).pin_memory(), None
    if self._staging_event is not None:
      self._staging_event.synchronize()  # the previous batch's copy out of this buffer (long finished)
    host = self._staging.numpy()
    at = 0
    for a, sz in zip(sections, sizes):
      if sz:
        host[at:at + sz] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
      at += sz
    host_rows = host[head:head + n * row_bytes].view(row_dtype).reshape(n, 3)
    at = 0
    for a in rows:  # each cloud straight into the pinned buffer (converted on the way if the batch mixes the two types)
      np.copyto(host_rows[at:at + a.shape[0]], a, casting="same_kind")
      at += a.shape[0]
    dev = self._staging[:total].to(self.device, non_blocking=True)
    self._staging_event = torch.cuda.Event()
    self._staging_event.record(torch.cuda.current_stream(self.device))
    out, at = [], 0
    for a, sz in zip(sections, sizes):
      out.append(dev[at:at + sz].view(getattr(torch, a.dtype.name)).reshape(a.shape))
      at += sz
    out.append(dev[head:head + n * row_bytes].view(getattr(torch, np.dtype(row_dtype).name)).reshape(n, 3))
    return out

  def __call__(self, frames, draws):
    B = len(frames)
    if B < 1 or B > PF.PAIR_MAX_PAIRS or draws.n_pairs != B:
      raise ValueError("PairInputPipeline: %d pairs (1 .. %d) with draws for %d" % (B, PF.PAIR_MAX_PAIRS, draws.n_pairs))
    clouds = [np.asarray(a) for f in frames for a in f[:2]]
    for a in clouds:
      if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("PairInputPipeline: a frame is an [n, 3] array, got %s" % (a.shape,))
    dt = np.float32 if all(a.dtype == np.float32 for a in clouds) else np.float64
    lens = [a.shape[0] for a in clouds]
    n = sum(lens)
    colored = [len(f) >= 4 for f in frames]
    if any(colored) and not all(colored):
      raise ValueError("PairInputPipeline: frames %s come with colours, the others without" % [b for b in range(B) if colored[b]])
    sections = []
    if colored[0]:  # the colours of the raw rows: one uint8 section in the same upload, padded to a multiple of 8 bytes
      rgb = np.zeros((3 * n + 7) // 8 * 8, np.uint8)
      at = 0
      for b, f in enumerate(frames):
        for s in range(2):
          c = np.asarray(f[2 + s])
          if c.dtype != np.uint8 or c.ndim != 2 or c.shape[1] != 3 or c.shape[0] != lens[2 * b + s]:
            raise ValueError("PairInputPipeline: pair %d: rgb%d is %s %s for %d points (uint8 [n, 3] expected)" %
                             (b, s, c.dtype, c.shape, lens[2 * b + s]))
          rgb[at:at + c.size] = c.reshape(-1)
          at += c.size
      sections = [rgb]
    radius = np.float64(self.voxel_size * self.search_multiplier) * draws.scale  # radius *= scale, ddp_data_loaders.py
    on = np.zeros(2 * B, np.int32)  # (an even number of words: every section is a multiple of 8 bytes, the raw rows come last)
    on[:] = draws.jitter_on if self.jitter is not None else 0
    with torch.cuda.device(self.device):
      offs_d, scale_d, radius_d, rot_d, on_d, *rgb_d, raw_d = self._upload(
          [np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), draws.scale, radius, draws.rot.reshape(-1, 9), on] + sections, clouds, dt)
      noise = None
      if self.jitter is not None and draws.jitter_on.any():
        if draws.noise is not None:
          noise = torch.as_tensor(draws.noise).to(self.device)
          if tuple(noise.shape) != (n, 3):
            raise ValueError("PairInputPipeline: noise is %s for %d raw rows" % (tuple(noise.shape), n))
        elif draws.generator is not None:
          g = draws.generator
          noise = torch.randn((n, 3), generator=g, dtype=torch.float32, device=g.device).to(self.device)
        else:
          raise ValueError("PairInputPipeline: the draws switch the feature jitter on but carry neither noise nor a generator")
      mu, sigma = self.jitter if self.jitter is not None else (0.0, 0.0)
      flags = torch.zeros(B, dtype=torch.int32, device=self.device)
      tf = PF.pair_transform(raw_d, offs_d, scale_d, rot_d if self.random_rotation else None, flags)
      vx = PF.pair_voxelize(tf["points"], offs_d, self.voxel_size, flags)
      # (the first batch: lib/device_loader.py's guess of 16 rows per point; later batches: what the batches before needed)
      cap = max(int(self.match_capacity), 1) if self.match_capacity is not None else min(max(16 * n, 1024), (1 << 31) - 1)
      mt = PF.pair_match(vx, tf["trans"], radius_d, cap, flags)
      co = PF.pair_collate(vx, tf["trans"], noise, on_d, mu, sigma)
      if rgb_d:  # sinput{0,1}_F from the colours, over the collate's ones
        PF.pair_color_features(rgb_d[0][:3 * n].view(n, 3), vx, co, noise, on_d, mu, sigma)
      back = torch.cat([vx["n_vox"], mt["pair_counts"], mt["totals"], flags.to(torch.int64)]).cpu().numpy()  # THE read-back
      self.last_readbacks = 1
      n_vox, totals, fl = back[:2 * B], back[3 * B:3 * B + 4], back[3 * B + 4:]
      msg = PF.pair_flags_message(fl)
      if msg is not None:
        raise PcmiError(msg)
      if totals[2]:  # the correspondences did not fit: the fill once more, with the room the exact count asks for (the collate
        cap = int(totals[0])  # in between uses no workspace: the cells and counts of the first call are still there)
        mt = PF.pair_match(vx, tf["trans"], radius_d, cap, flags, fill_only=True)
        again = mt["totals"].cpu().numpy()
        self.last_readbacks = 2
        if again[2] or again[0] != totals[0]:
          raise PcmiError("pre-training input: the match needed %d rows, then %d" % (totals[0], again[0]))
      if self.match_capacity is None or totals[2]:
        self.match_capacity = max(int(self.match_capacity or 0), int(totals[0] * 1.25) + 1024)
    N = (int(n_vox[0::2].sum()), int(n_vox[1::2].sum()))
    out = {"correspondences": mt["pairs"][:int(totals[0])], "T_gt": co["T_gt"],
           "len_batch": [[int(n_vox[2 * b]), int(n_vox[2 * b + 1])] for b in range(B)], "n_queries": int(totals[1])}
    for s in (0, 1):
      for key in ("pcd%d", "sinput%d_C", "sinput%d_F"):
        out[key % s] = co[key % s][:N[s]]
    return out


class RawPairFiles(torch.utils.data.Dataset):
  """The two raw 'pcd' arrays of every line of the pair list (data.dataset_root_dir / data.scannet_match_dir): all a loader
  worker does with data.device_batch=True.  data.use_color: the two 'color' arrays behind them, (xyz0, xyz1, rgb0, rgb1)."""

  def __init__(self, config):
    self.use_color = bool(config.data.get("use_color", False))
    self.root = config.data.dataset_root_dir
    if not self.root or not config.data.scannet_match_dir:
      raise ValueError("data.device_batch=True needs data.dataset_root_dir and data.scannet_match_dir (the pair list)")
    with open(os.path.join(self.root, config.data.scannet_match_dir)) as f:
      self.files = [ln.split()[:2] for ln in f if len(ln.split()) >= 2]

  def __len__(self):
    return len(self.files)

  def __getitem__(self, idx):
    if not self.use_color:
      return tuple(np.load(os.path.join(self.root, p))["pcd"] for p in self.files[idx])
    from .ddp_data_loaders import load_frame
    xyz, rgb = zip(*(load_frame(os.path.join(self.root, p), True) for p in self.files[idx]))
    return xyz + rgb


def _as_list(items):
  return list(items)


class DevicePairLoader:
  """data.device_batch=True: an infinite iterator of device batches.  A DataLoader (misc.train_num_thread workers, which never
  touch the GPU) reads the raw frames with make_data_loader's infinite samplers; next() draws PairDraws.sample on the training
  process and runs PairInputPipeline."""

  def __init__(self, config, batch_size, num_threads=None, device=None):
    self.config = config
    self.batch_size = batch_size // config.misc.num_gpus  # per-GPU batch, as make_data_loader
    self.dataset = RawPairFiles(config)
    threads = config.misc.train_num_thread if num_threads is None else num_threads
    sampler = DistributedInfSampler(self.dataset) if config.misc.num_gpus > 1 else InfSampler(self.dataset, shuffle=True)
    self.loader = torch.utils.data.DataLoader(self.dataset, batch_size=self.batch_size, shuffle=False, num_workers=threads,
                                              collate_fn=_as_list, sampler=sampler, drop_last=True)
    self.pipeline = PairInputPipeline(config.data.voxel_size, config.trainer.positive_pair_search_voxel_size_multiplier,
                                      random_rotation=config.trainer.use_random_rotation, device=device)
    self.randg = np.random.RandomState()
    self.generator = torch.Generator(device=self.pipeline.device)
    self.generator.manual_seed(config.misc.get("seed", 0))
    self._it = None

  def reset_seed(self, seed=0):
    self.randg.seed(seed)
    self.generator.manual_seed(seed)

  def __len__(self):
    return len(self.loader)

  def close(self):
    """Ends the reading workers (they would otherwise live as long as the iterator)."""
    self._it = None

  def __iter__(self):
    if self._it is None:
      self._it = iter(self.loader)
    return self

  def __next__(self):
    if self._it is None:
      self._it = iter(self.loader)
    frames = next(self._it)
    return self.pipeline(frames, PairDraws.sample(self.config, len(frames), self.randg, self.generator))
