"""``python -m skoots_amd.train --config-file F.yaml [-b/--batch] [--log 0-4] [--precision bf16|mixed|fp32] [--seed N]``
(reference: skoots/train/__main__.py:37-113).  ``--batch``: ``--config-file`` names a folder, every ``*.yaml`` in it is
one run.  A run writes ``<TRAIN.SAVE_PATH>/<config file's base name>.trch`` and ``.csv``."""
from __future__ import annotations

import argparse
import glob
import logging
import os
import socket
from typing import List, Optional

from ..config import cfg_to_dict, load_cfg_from_file

LOG_LEVELS = [logging.DEBUG, logging.INFO, logging.WARNING, logging.ERROR, logging.CRITICAL]


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="skoots-train (MI355X)", description="SKOOTS Training Parameters")
    parser.add_argument("--config-file", type=str, required=True, help="YAML config file for training")
    parser.add_argument("-b", "--batch", action="store_true", help="Batch execute a folder of training config files")
    parser.add_argument("--log", type=int, default=3, choices=range(5),
                        help="Log Level: 0-Debug, 1-Info, 2-Warning, 3-Error, 4-Critical")
    parser.add_argument("--precision", default="bf16", choices=("bf16", "mixed", "fp32"),
                        help="precision of the step (bf16 is the reference's dtype)")
    parser.add_argument("--seed", type=int, default=101196, help="seed of the initial weights and the augmentation")
    return parser


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank: int, world_size: int, port: int, cfg_plain: dict, precision: str, seed: int, run_name: str,
               log_level: int) -> None:
    """One rank of a multi-GPU run, in a fresh process: builds the default process group, then trains."""
    import torch
    import torch.distributed as dist
    from ..config import get_cfg_defaults, merge_cfg
    from .trainer import train
    logging.basicConfig(level=LOG_LEVELS[log_level], force=True,
                        format=f"[%(asctime)s] skoots-train rank{rank} [%(levelname)s]: %(message)s")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world_size))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", device_id=torch.device("cuda", rank))
    try:
        train(merge_cfg(get_cfg_defaults(), cfg_plain), precision, seed, rank, world_size, run_name)
    finally:
        dist.destroy_process_group()


def main(argv: Optional[List[str]] = None) -> List[str]:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=LOG_LEVELS[args.log], format="[%(asctime)s] skoots-train [%(levelname)s]: %(message)s")
    configs = sorted(glob.glob(os.path.join(args.config_file, "*.yaml"))) if args.batch else [args.config_file]
    if args.batch:
        logging.info("found %d config files at: %s", len(configs), args.config_file)
    from .trainer import resolve_world_size, train
    written = []
    for f in configs:
        cfg = load_cfg_from_file(f)
        run_name = os.path.splitext(os.path.basename(f))[0]
        world_size = resolve_world_size(cfg)
        if world_size == 1:
            written.append(train(cfg, args.precision, args.seed, 0, 1, run_name))
        else:
            # fresh child processes (spawn start method): this process has not touched the GPU and does not
            import torch.multiprocessing as mp
            mp.spawn(_rank_main, args=(world_size, _free_port(), cfg_to_dict(cfg), args.precision, args.seed, run_name,
                                       args.log), nprocs=world_size, join=True)
            written.append(os.path.join(cfg.TRAIN.SAVE_PATH, run_name + ".trch"))
        logging.info("finished the run of config file: %s", f)
    return written


if __name__ == "__main__":
    main()
