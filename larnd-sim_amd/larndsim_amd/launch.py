"""
Starting the ranks of a sharded run (cli/simulate_pixels.py --n_gpus) -- standard library only: the self-launching parent
imports this and nothing that loads numpy, the HIP library or the GPU.
"""
import os
import socket
import subprocess
import time
import uuid


def dist_mode(n_gpus, force_dist, environ=None):
    """(rank, world) of this process for --n_gpus / --force_dist; world None = the plain one-process run.  Without --n_gpus a
    launcher's WORLD_SIZE is ignored; with it WORLD_SIZE (when set) must equal N.  N = 1 runs the RCCL path only with
    --force_dist.  ValueError on a contradiction."""
    env = os.environ if environ is None else environ
    if n_gpus is None:
        if force_dist:
            raise ValueError("--force_dist needs --n_gpus")
        return 0, None
    n_gpus = int(n_gpus)
    if n_gpus < 1:
        raise ValueError("--n_gpus must be >= 1")
    if "WORLD_SIZE" in env and int(env["WORLD_SIZE"]) != n_gpus:
        raise ValueError(f"--n_gpus {n_gpus} but the launcher set WORLD_SIZE={env['WORLD_SIZE']}")
    if n_gpus == 1 and not force_dist:
        return 0, None
    return int(env.get("RANK", "0")), n_gpus


def launch_ranks(cmd, n, env_extra=None, poll_s=0.2, grace_s=10.0, timeout=None):
    """``n`` fresh child processes running ``cmd``, one rank each (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set; never an exec
    of this process).  Every child is polled; on the first non-zero exit the others are terminated, then killed after
    ``grace_s``; so are all of them when ``timeout`` seconds pass (code 124).  Returns (worst exit code, [(rank, code) of the
    failed ranks]).  Touches no GPU."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:          # a free port for the ranks' rendezvous
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    job = uuid.uuid4().hex
    procs = []
    deadline = None if timeout is None else time.time() + timeout
    try:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), LDSIM_JOB_ID=job, **(env_extra or {}))
            procs.append(subprocess.Popen(cmd, env=env))
        bad = []
        while True:
            codes = [p.poll() for p in procs]
            bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
            if bad or all(c is not None for c in codes):
                break
            if deadline is not None and time.time() > deadline:
                bad = [(r, 124) for r, c in enumerate(codes) if c is None]
                break
            time.sleep(poll_s)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        deadline = time.time() + grace_s
        for p in procs:
            try:
                p.wait(timeout=max(deadline - time.time(), 0.1))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    if not bad:
        return 0, []
    return max(1, max(abs(c) for _, c in bad) & 0xFF), bad
