"""CPU: the host side of the sharded drop-in driver (simulate_pixels.py --n_gpus): event sharding, the merge order of the
ranks' compact results on rank 0, and a rehearsal of the self-launch (no GPU call)."""
import os
import subprocess
import sys
import time

import numpy as np

import helpers as H
from larndsim_amd import dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")


def _random_table(rng, n_events):
    """(event, tpc group, sub-batch, n segments) rows like batching.assign_batches: events ascending, 1-4 batches each"""
    table = []
    for ev in np.sort(rng.choice(10 * n_events + 5, n_events, replace=False)):
        for k in range(int(rng.integers(1, 5))):
            table.append((int(ev), k // 2, k % 2, int(rng.integers(1, 400))))
    return table


def test_shard_events_whole_events_contiguous_balanced():
    rng = np.random.default_rng(5)
    for trial in range(60):
        n_events = int(rng.integers(1, 40))
        world = int(rng.integers(1, 9)) if trial % 3 else n_events + int(rng.integers(1, 4))   # also more ranks than events
        table = _random_table(rng, n_events)
        rank = dist.shard_events(table, world)
        assert rank.shape == (len(table),) and rank.dtype == np.int32
        assert ((0 <= rank) & (rank < world)).all()
        assert (np.diff(rank) >= 0).all()                          # contiguous runs, in rank order
        ev = np.array([t[0] for t in table])
        for e in np.unique(ev):                                     # an event never straddles two ranks
            assert len(np.unique(rank[ev == e])) == 1
        sizes = np.array([t[3] for t in table])
        ev_size = {e: sizes[ev == e].sum() for e in np.unique(ev)}
        per_rank = np.bincount(rank, weights=sizes, minlength=world)
        ideal = sizes.sum() / world
        assert np.abs(per_rank - ideal).max() <= max(ev_size.values()), (trial, per_rank, ideal)
    assert (dist.shard_events([], 4) == 0).all() and len(dist.shard_events([], 4)) == 0
    assert (dist.shard_events(_random_table(rng, 5), 1) == 0).all()


def _random_compact(rng, table, pix_pool):
    """a chain launch's compact result (ChargeChain.download_compact layout) over the batches of ``table``: a batch's first
    row always present (hits or not), hits / track slots / fractions per row"""
    hp, trk, hits, frac = [], [], [], []
    for b, t in enumerate(table):
        n_rows = int(rng.integers(1, 6))
        pix = rng.choice(pix_pool, n_rows, replace=False)
        for i in range(n_rows):
            nh = int(rng.integers(0 if i == 0 else 1, 4))
            nt = int(rng.integers(1, 5)) if nh else 0
            hp.append((len(hp), int(pix[i]), b, nh, nt | (256 if i == 0 else 0)))
            trk.extend(rng.integers(0, t[3], nt).tolist())
            for h in range(nh):
                hits.append((b, int(pix[i]), int(rng.integers(1, 256)), h, float(rng.uniform(0, 2000.0))))
                f = rng.uniform(0, 1, nt)
                frac.extend((f / f.sum()).tolist())
    from larndsim_amd.comm import HIT_ROW
    hit_rows = np.array(hits, dtype=HIT_ROW)
    return dict(hit_pixels=np.array(hp, dtype=np.int32).reshape(-1, 5), track_segments=np.array(trk, dtype=np.int64),
                hit_rows=hit_rows, hit_charge=rng.uniform(0, 1e4, len(hit_rows)), fractions=np.array(frac),
                has_fractions=True)


def _slice_compact(c, a, b):
    """rows [a, b) of the hit pixels of a compact result, with their parts: what one rank's gathered stream holds"""
    hp = c["hit_pixels"]
    nh, nt = hp[:, 3].astype(np.int64), (hp[:, 4] & 255).astype(np.int64)
    h0, t0, f0 = (np.r_[0, np.cumsum(v)] for v in (nh, nt, nh * nt))
    return dict(hit_pixels=hp[a:b].copy(), track_segments=c["track_segments"][t0[a]:t0[b]].copy(),
                hit_rows=c["hit_rows"][h0[a]:h0[b]].copy(), hit_charge=c["hit_charge"][h0[a]:h0[b]].copy(),
                fractions=c["fractions"][f0[a]:f0[b]].copy(), has_fractions=True)


def _export(pieces, table, event_times, seg_ids, trj_ids):
    """the driver's compact export with WRITE_BATCH_SIZE 1, piece after piece: one build_packets_compact per batch run"""
    from larndsim_amd import packets
    event_of_batch = np.array([t[0] for t in table], dtype=np.int64)
    first_seg = np.r_[0, np.cumsum([t[3] for t in table])][:-1].astype(np.int64)
    pk, assn = [], []
    for c in pieces:
        rb = c["hit_pixels"][:, 2]
        starts = np.flatnonzero(np.r_[True, rb[1:] != rb[:-1]]) if len(rb) else np.zeros(0, dtype=np.int64)
        for a, b in zip(starts, np.r_[starts[1:], len(rb)]):
            rows = packets.compact_to_rows(c, event_of_batch, first_seg, seg_ids, trj_ids, rows=(int(a), int(b)))
            ev = int(event_of_batch[rb[a]])
            p, s = packets.build_packets_compact(**rows, event_start_times=np.array([event_times[ev]]))
            pk.append(p)
            assn.append(s)
    return np.concatenate(pk), np.concatenate(assn)


def test_rank_pieces_exported_in_rank_order_equal_the_whole():
    """rank 0 exports every rank's gathered compact stream after its own: split at event boundaries into N pieces (each with
    its own part offsets, like ldsim_comm_gathered_compact_download's per-rank download) and exported in rank order, the
    packets and association rows are byte-identical to exporting the whole"""
    H.load_cfg("module0", noise_zero=False)
    g = H.gold("packets_module0.npz")
    pix_pool = np.unique(g["unique_pix"])
    rng = np.random.default_rng(11)
    for trial in range(4):
        table = _random_table(rng, 14)
        c = _random_compact(rng, table, pix_pool)
        n_seg = sum(t[3] for t in table)
        seg_ids = rng.permutation(n_seg).astype(np.int64)
        trj_ids = rng.integers(0, 30, n_seg).astype(np.int64)
        ev_max = max(t[0] for t in table)
        event_times = np.cumsum(rng.exponential(1e5, ev_max + 1))
        whole = _export([c], table, event_times, seg_ids, trj_ids)
        assert len(whole[0]) > 50
        for world in (2, 3, 5, 20):
            brank = dist.shard_events(table, world)
            row_rank = brank[c["hit_pixels"][:, 2]]
            cuts = np.searchsorted(row_rank, np.arange(world + 1), side="left")
            pieces = [_slice_compact(c, int(cuts[r]), int(cuts[r + 1])) for r in range(world)]
            assert sum(len(p["hit_rows"]) for p in pieces) == len(c["hit_rows"])
            got = _export(pieces, table, event_times, seg_ids, trj_ids)
            assert got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes(), (trial, world)


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def _started_pids(stdout):
    """pids the ranks of a rehearsal report when they start"""
    return [int(ln.rsplit("pid ", 1)[1].rstrip(")")) for ln in stdout.decode().splitlines()
            if ln.startswith("rehearsal:") and "started (pid" in ln]


def _alive(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    with open(f"/proc/{pid}/stat") as f:                            # (a zombie is not alive)
        return f.read().rsplit(")", 1)[1].split()[0] != "Z"


def test_cli_n_gpus_self_launch_rehearsal(tmp_path):
    """`simulate_pixels.py --n_gpus 2` without a launcher starts two fresh ranks that meet over the id hand-out;
    LDSIM_CLI_REHEARSAL stops them before any GPU call.  A WORLD_SIZE that contradicts --n_gpus is refused; a rank that exits
    non-zero ends the command non-zero within a bounded time, the surviving rank killed."""
    args = ["--input_filename", str(tmp_path / "in.npy"), "--output_filename", str(tmp_path / "out.npz"), "--n_gpus", "2"]
    r = subprocess.run([sys.executable, CLI] + args, env=_env(LDSIM_CLI_REHEARSAL="1"), capture_output=True, timeout=180)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    met = sorted(ln for ln in r.stdout.decode().splitlines() if ln.startswith("rehearsal:") and ln.endswith(" met"))
    assert met == ["rehearsal: rank 0 of 2 met", "rehearsal: rank 1 of 2 met"] and len(_started_pids(r.stdout)) == 2
    assert not os.path.exists(tmp_path / "out.npz")
    # a launcher whose WORLD_SIZE contradicts --n_gpus
    r = subprocess.run([sys.executable, CLI] + args, env=_env(LDSIM_CLI_REHEARSAL="1", WORLD_SIZE="3", RANK="0"),
                       capture_output=True, timeout=60)
    assert r.returncode != 0 and b"WORLD_SIZE=3" in r.stderr and b"rehearsal:" not in r.stdout
    # rank 1 dies before the rendezvous: rank 0 would wait for it; the parent ends it and fails
    t0 = time.time()
    r = subprocess.run([sys.executable, CLI] + args, env=_env(LDSIM_CLI_REHEARSAL="1", LDSIM_CLI_REHEARSAL_FAIL_RANK="1"),
                       capture_output=True, timeout=100)
    assert r.returncode != 0 and time.time() - t0 < 60 and b"ranks failed" in r.stderr
    assert b" met" not in r.stdout
    pids = _started_pids(r.stdout)
    assert len(pids) == 2 and not any(_alive(p) for p in pids)
    # --raw_arrays with more than one rank: refused before any rank starts
    r = subprocess.run([sys.executable, CLI] + args + ["--raw_arrays"], env=_env(LDSIM_CLI_REHEARSAL="1"), capture_output=True,
                       timeout=60)
    assert r.returncode != 0 and b"--raw_arrays" in r.stderr and not _started_pids(r.stdout)
