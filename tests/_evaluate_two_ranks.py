"""Helper of tests/test_gpu_evaluate.py::test_two_ranks_merge_to_the_one_process_result: launched by torch.distributed.run with
two ranks that share cuda:0 over gloo (rehearsal of the one-rank-per-GPU RCCL job on a one-GPU box).  Each rank evaluates its
shard_range of the table with evaluate_table, which merges the statistics; rank 0 stores the merged ErrorStats and both shard
ranges for the parent test to compare with the one-process evaluation of the whole table."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _evaluate_util import net_card  # noqa: E402
from irbfn_amd import configs, distributed, evaluate  # noqa: E402
from irbfn_amd.model import WCRBFNet  # noqa: E402


def main():
    inp, out = sys.argv[1], sys.argv[2]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    world = dist.get_world_size()
    d = np.load(inp)
    net = WCRBFNet.from_config(net_card(7, d["y"].shape[1])[0])
    params = {"params": {"rbf_list": {"centers": d["centers"], "log_sigs": d["log_sigs"]},
                         "linear": {"kernel": d["kernel"], "bias": d["bias"]}}}
    stats = evaluate.evaluate_table(net, params, d["x"], d["y"], "cartesian_st", np.array(configs.DYN_PARAMS), batch_size=501)
    s, argmax, hist, rows = stats.to_host()
    if dist.get_rank() == 0:
        shards = np.array([v for r in range(world) for v in distributed.shard_range(d["x"].shape[0], r, world)])
        np.savez(out, stats=s, argmax=argmax, hist=hist, rows=rows, shards=shards)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
