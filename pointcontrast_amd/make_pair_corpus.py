"""python -m pointcontrast_amd.make_pair_corpus --export DIR --target DIR [--voxel-size --threshold --frame-skip --scenes --color]
python -m pointcontrast_amd.make_pair_corpus --scans DIR --target DIR [--views 64 --seed 0 --width --height --focal --splat --rel-tol
                                                                       --min-coverage --voxel-size --threshold --scenes]

Builds the pre-training pair corpus from a reader.py export (<scene>/depth/<n>.png, <scene>/pose/<n>.txt,
<scene>/intrinsic/intrinsic_depth.txt) on the GPU (lib/pair_corpus.py): <target>/<scene>/pcd/<n>.npz,
<target>/<scene>/pcd/overlap.txt and <target>/overlap-30-full.txt, which ddp_train reads with
data.dataset=ScanNetMatchPairDataset data.dataset_root_dir=<target> data.scannet_match_dir=overlap-30-full.txt.
--color adds the RGB of every point to the npz files (member 'color') from reader.py --export_color_images' output
(<scene>/color/<n>.png or .jpg, intrinsic/intrinsic_color.txt, extrinsic_color.txt, extrinsic_depth.txt): data.use_color=True.
--scans builds the same files from whole scans instead (<scene>.npz / .npy / .ply or <scene>/<scene>_vh_clean_2.ply), through
virtual depth views of every scan (lib/scan_views.py; the view parameters' defaults are untuned); colours are carried when the
scan has them."""
import argparse
import sys


def parse_args(argv=None):
  ap = argparse.ArgumentParser(prog="python -m pointcontrast_amd.make_pair_corpus", description=__doc__.split("\n\n")[1])
  src = ap.add_mutually_exclusive_group(required=True)
  src.add_argument("--export", help="root of the exported scenes")
  src.add_argument("--scans", help="root of whole scans (<scene>.npz / .npy / .ply or <scene>/<scene>_vh_clean_2.ply)")
  ap.add_argument("--target", required=True, help="output root (the training run's data.dataset_root_dir)")
  ap.add_argument("--voxel-size", type=float, default=0.05)
  ap.add_argument("--threshold", type=float, default=0.3, help="smallest overlap kept in the corpus list (inclusive)")
  ap.add_argument("--frame-skip", type=int, default=1, help="use every n-th exported frame (--export)")
  ap.add_argument("--scenes", nargs="*", default=None, help="scene directories (--export) or scan names (--scans) to process (default: all)")
  ap.add_argument("--color", action="store_true", help="add the colour of every point to the npz files (for data.use_color=True; --export)")
  ap.add_argument("--views", type=int, default=64, help="virtual cameras per scan (--scans)")
  ap.add_argument("--seed", type=int, default=0, help="seed of the cameras' draws (--scans)")
  ap.add_argument("--width", type=int, default=320, help="pixels of a virtual view (--scans)")
  ap.add_argument("--height", type=int, default=240)
  ap.add_argument("--focal", type=float, default=288.0, help="fx = fy of the virtual camera, pixels (--scans)")
  ap.add_argument("--splat", type=int, default=3, help="pixels a point covers in the z-buffer: odd, 1 ... 7 (--scans)")
  ap.add_argument("--rel-tol", type=float, default=0.05, help="relative depth tolerance of the visibility test (--scans)")
  ap.add_argument("--min-coverage", type=float, default=0.5, help="views with a smaller share of occupied pixels are dropped (--scans)")
  return ap.parse_args(argv)


def main(argv=None):
  args = parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    sys.exit("make_pair_corpus: no GPU -- the corpus kernels run only on a gfx950 device")
  from .lib import pair_corpus
  if args.scans is not None:
    from .lib import scan_views
    out = scan_views.build_corpus_from_scans(args.scans, args.target, n_views=args.views, seed=args.seed, height=args.height,
                                             width=args.width, focal=args.focal, splat=args.splat, rel_tol=args.rel_tol,
                                             min_coverage=args.min_coverage, voxel_size=args.voxel_size, threshold=args.threshold,
                                             scenes=args.scenes, log=lambda s: print(s, flush=True))
  else:
    out = pair_corpus.build_corpus(args.export, args.target, voxel_size=args.voxel_size, threshold=args.threshold,
                                   frame_skip=args.frame_skip, scenes=args.scenes, color=args.color, log=lambda s: print(s, flush=True))
  print("%d scenes, %d pairs, %d in %s" % (len(out), sum(s["pairs"] for s in out), sum(s["over_threshold"] for s in out),
                                           pair_corpus.LIST_NAME), flush=True)


if __name__ == "__main__":
  main()
