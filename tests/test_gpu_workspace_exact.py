"""The entry points that no other test file runs at exactly their queried workspace AND one byte short: pcmi_pair_transform,
pcmi_corpus_overlap_counts, pcmi_components_compact, pcmi_instance_scores and pcmi_offset_loss_fwd.  Through the Python wrappers, with a workspace of exactly the queried size between
guard bands (c_contract._ExactWorkspace): the same arrays as with the wrappers' shared workspace, both bands intact, and one
byte less refused with PCMI_ERR_WORKSPACE before anything is written.

Where every other entry point that carves a workspace (csrc/internal.h: Carve, require_ws) has that test:
  test_gpu_firstrow.py          pcmi_voxelize, pcmi_match_radius, pcmi_corpus_backproject, pcmi_corpus_voxel_centroids,
                                pcmi_pair_voxelize, pcmi_pair_match, pcmi_gather_points_bwd (build_inverse_lists)
  test_gpu_c_contract.py        pcmi_pair_select
  test_gpu_pair_color.py        pcmi_corpus_backproject_color (and pcmi_pair_color_features, whose 256 bytes no kernel uses)
  test_gpu_semseg_input.py      pcmi_elastic_blur, pcmi_seg_transform, pcmi_seg_quantize, pcmi_seg_color_augment
  test_gpu_insseg_input.py      pcmi_instance_relabel, pcmi_seg_crop_ladder
  test_gpu_detect_input.py      pcmi_det_votes_from_instances, pcmi_det_voxelize
  test_gpu_detect_features.py   pcmi_segment_quantile
  test_gpu_views.py             pcmi_views_visible
  test_gpu_nearest.py           pcmi_nearest_point
  test_gpu_insseg.py            pcmi_radius_components (the other three entries of cluster.hip: exact only; short here)
  test_gpu_kmeans.py            pcmi_kmeans_assign, pcmi_kmeans_pp_step
  test_gpu_proposals.py         pcmi_proposal_overlap
  test_gpu_insbench.py          pcmi_instance_bench_ap
  test_gpu_segeval.py           pcmi_seg_eval_rows, pcmi_seg_ap
  test_gpu_ap.py                pcmi_det_ap
  test_gpu_detect_dispatch.py   pcmi_fps, pcmi_nn_distance_bwd, pcmi_group_points_bwd / pcmi_three_interpolate_bwd
  test_gpu_votehead.py          pcmi_group_rows_bwd
  test_gpu_rowspool.py          pcmi_bn_maxpool_fwd_train, pcmi_bn_maxpool_bwd, pcmi_interp_rows_bwd
  test_gpu_featmatch.py         pcmi_feat_nn"""
import numpy as np
import pytest
import torch

from c_contract import DEV, _exact_and_short, _same_arrays, exact_ws  # noqa: F401  (exact_ws is a fixture)

pytestmark = pytest.mark.gpu


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rotation(rng):
  q, _ = np.linalg.qr(rng.randn(3, 3))
  return q * np.sign(np.linalg.det(q))


def test_pair_transform_workspace(exact_ws):
  """Two pairs, 930 rows: the per-chunk partial sums of the workspace are written and read only with a rotation (the centring)."""
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(21)
  sizes = [300, 280, 150, 200]
  offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
  raw = _dev((rng.rand(offs[-1], 3) * 4 - 2).astype(np.float32))
  scale, rot = _dev(rng.uniform(0.8, 1.2, 2)), _dev(np.stack([_rotation(rng) for _ in range(4)]))

  def run():
    out = PF.pair_transform(raw, _dev(offs), scale, rot)
    assert out["flags"].cpu().tolist() == [0, 0]
    return [out[k].cpu().numpy() for k in ("points", "T", "trans", "flags")]
  _exact_and_short(exact_ws, run, _same_arrays)


def test_cluster_workspaces(exact_ws):
  """pcmi_components_compact, pcmi_instance_scores and pcmi_offset_loss_fwd (test_gpu_insseg.py runs them at exactly the queried
  size but never a byte short) behind pcmi_radius_components: two scenes of 300 and 257 rows, six planted blobs, two groups."""
  from pointcontrast_amd import functional as PF
  rng = np.random.RandomState(23)
  n, offs = 557, [0, 300, 557]
  centre = rng.randint(0, 6, n)
  xyz = _dev((np.eye(3)[centre % 3] * (1 + centre // 3)[:, None] + rng.randn(n, 3) * 0.01).astype(np.float32))
  group, score = _dev((centre % 2).astype(np.int32)), _dev(rng.rand(n).astype(np.float32))
  target = _dev(rng.randn(n, 3).astype(np.float32))

  def run():
    label = PF.radius_components(xyz, offs, group, 0.1)
    c = PF.components_compact(label, offs, group, 5, 32)
    count = int(c["count"].cpu())
    assert 6 <= count <= 12
    mean = PF.instance_scores(score, c["instance"], c["size"][:count])
    norm, direction = PF.OffsetLossFunction.apply(xyz, target, c["instance"])
    return [label.cpu().numpy(), c["instance"].cpu().numpy(), c["root"].cpu().numpy(), c["size"].cpu().numpy(), mean.cpu().numpy(),
            norm.detach().cpu().numpy(), direction.detach().cpu().numpy()]
  _exact_and_short(exact_ws, run, _same_arrays, calls=4, short_at=(1, 2, 3))


def test_corpus_overlap_workspace(exact_ws):
  """pcmi_corpus_overlap_counts, call 2 of process_scene (test_gpu_firstrow.py cuts calls 0 and 1 short): two frames of 257 and
  300 valid pixels that see the same surface, so the cell lists, the frame of every point and the error word are all used."""
  from pointcontrast_amd.lib import pair_corpus
  rng = np.random.RandomState(22)
  w = 300
  depths = rng.randint(900, 1100, size=(2, 1, w)).astype(np.uint16)
  depths[0, 0, 257:] = 0  # invalid pixels: frame 0 has 257 points
  K = np.eye(4)
  K[0, 0] = K[1, 1] = 100.0
  K[0, 2] = w / 2

  def run():
    out = pair_corpus.process_scene(depths, np.stack([np.eye(4), np.eye(4)]), K, voxel_size=0.05, device=DEV)
    assert [len(p) for p in out["points"]] == [257, w] and out["C"][0, 1] > 0
    return [out["points"][1], out["centroids"][0], out["centroids"][1], out["C"]]
  _exact_and_short(exact_ws, run, _same_arrays, calls=3, short_at=(2,))
