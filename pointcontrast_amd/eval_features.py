"""Scores a pre-trained checkpoint by feature matching on held-out pairs, without training:

  python -m pointcontrast_amd.eval_features misc.weight=CKPT data.dataset=ScanNetMatchPairDataset \\
      data.dataset_root_dir=ROOT data.val_match_dir=LIST [trainer.val_max_batches=N] [val.num_queries=5000 ...]

builds the trainer's network, loads the weights (misc.weight, as the trainers do), runs ContrastiveLossTrainer.validate over
the list and prints the metrics as ONE JSON line on stdout (the per-pair arrays are left out).  The reference has no
counterpart; the metrics are those of lib/feature_match.py.  Single process, single GPU."""
import json
import logging
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # as ddp_train

import numpy as np
import torch

from .lib.config import get_config
from .lib.ddp_data_loaders import make_val_data_loader


def evaluate(overrides):
  """The metrics dict (with `pairs`) of the checkpoint misc.weight on the validation list."""
  from .ddp_train import get_trainer
  config = get_config(overrides)
  if not config.misc.weight:
    raise ValueError("eval_features needs misc.weight=<checkpoint>")
  torch.manual_seed(config.misc.seed)
  np.random.seed(config.misc.seed)
  trainer = get_trainer(config.trainer.trainer)(config=config, data_loader=None)
  loader = make_val_data_loader(config, config.trainer.batch_size)
  return trainer.validate(loader, config.trainer.get("val_max_batches", None))


def main(argv=None):
  logging.basicConfig(level=logging.WARNING, stream=sys.stderr)
  overrides = [a for a in (argv if argv is not None else sys.argv[1:]) if "=" in a]
  m = evaluate(overrides)
  print(json.dumps({k: v for k, v in m.items() if k != "pairs"}, sort_keys=True), flush=True)
  return m


if __name__ == "__main__":
  main()
