"""python -m pointcontrast_amd.make_pair_corpus --export DIR --target DIR [--voxel-size --threshold --frame-skip --scenes --color]

Builds the pre-training pair corpus from a reader.py export (<scene>/depth/<n>.png, <scene>/pose/<n>.txt,
<scene>/intrinsic/intrinsic_depth.txt) on the GPU (lib/pair_corpus.py): <target>/<scene>/pcd/<n>.npz,
<target>/<scene>/pcd/overlap.txt and <target>/overlap-30-full.txt, which ddp_train reads with
data.dataset=ScanNetMatchPairDataset data.dataset_root_dir=<target> data.scannet_match_dir=overlap-30-full.txt.
--color adds the RGB of every point to the npz files (member 'color') from reader.py --export_color_images' output
(<scene>/color/<n>.png or .jpg, intrinsic/intrinsic_color.txt, extrinsic_color.txt, extrinsic_depth.txt): data.use_color=True."""
import argparse
import sys


def main(argv=None):
  ap = argparse.ArgumentParser(prog="python -m pointcontrast_amd.make_pair_corpus", description=__doc__.split("\n\n")[1])
  ap.add_argument("--export", required=True, help="root of the exported scenes")
  ap.add_argument("--target", required=True, help="output root (the training run's data.dataset_root_dir)")
  ap.add_argument("--voxel-size", type=float, default=0.05)
  ap.add_argument("--threshold", type=float, default=0.3, help="smallest overlap kept in the corpus list (inclusive)")
  ap.add_argument("--frame-skip", type=int, default=1, help="use every n-th exported frame")
  ap.add_argument("--scenes", nargs="*", default=None, help="scene directories to process (default: all)")
  ap.add_argument("--color", action="store_true", help="add the colour of every point to the npz files (for data.use_color=True)")
  args = ap.parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    sys.exit("make_pair_corpus: no GPU -- the corpus kernels run only on a gfx950 device")
  from .lib import pair_corpus
  out = pair_corpus.build_corpus(args.export, args.target, voxel_size=args.voxel_size, threshold=args.threshold,
                                 frame_skip=args.frame_skip, scenes=args.scenes, color=args.color, log=lambda s: print(s, flush=True))
  print("%d scenes, %d pairs, %d in %s" % (len(out), sum(s["pairs"] for s in out), sum(s["over_threshold"] for s in out),
                                           pair_corpus.LIST_NAME), flush=True)


if __name__ == "__main__":
  main()
