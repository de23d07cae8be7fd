"""
Multi-GPU plumbing: one process per GPU, batches (event x TPC-group) sharded across ranks, one
all-gather of the compact hit rows to reassemble the per-pixel ADC output.

The exchange itself is RCCL behind the C-ABI (csrc/comm.hip, larndsim_amd/comm.py); this module only decides which batches
a rank owns: ``shard_batches`` / ``shard_segments`` for bench.py, ``shard_events`` (whole events) for the drop-in driver
(cli/simulate_pixels.py --n_gpus).  No torch here: tests/test_cpu_dist.py rehearses the gather's two-step algorithm over gloo on its own.
"""
import os

import numpy as np

from . import batching


def env_world():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))


def shard_segments(batch_id, order, table, rank, world):
    """Segment indices (into the original array) and re-based batch ids of this rank's shard."""
    brank = batching.shard_batches(table, world)
    sorted_bid = batch_id[order]
    nsim = int((batch_id >= 0).sum())
    sel = np.zeros(len(order), dtype=bool)
    sel[:nsim] = brank[sorted_bid[:nsim]] == rank
    idx = order[sel]
    return idx, batch_id[idx]


def shard_events(table, world):
    """Contiguous runs of whole events over ``world`` ranks, balanced by segment count: int32 rank per batch of ``table``
    (batching.assign_batches).  The batches of one event -- its TPC groups and sub-batches -- always land on one rank, and rank
    r's batches precede rank r + 1's, so the ranks' results concatenated in rank order are the one-rank order.  An event
    goes to the rank whose share of the segment total holds the event's midpoint; a rank may end up with no event."""
    rank = np.zeros(len(table), dtype=np.int32)
    if world <= 1 or len(table) == 0:
        return rank
    ev = np.array([t[0] for t in table])
    sizes = np.array([t[3] for t in table], dtype=np.int64)
    starts = np.flatnonzero(np.r_[True, ev[1:] != ev[:-1]])
    ev_sizes = np.add.reduceat(sizes, starts)
    mid = np.cumsum(ev_sizes) - ev_sizes / 2.0
    ev_rank = np.minimum((mid * world / max(int(sizes.sum()), 1)).astype(np.int64), world - 1)
    rank[:] = np.repeat(ev_rank, np.diff(np.r_[starts, len(table)]))
    return rank
