"""Random states of the noisy stages -- mirrors ``numba.cuda.random.create_xoroshiro128p_states`` as the reference's driver
uses it (cli/simulate_pixels.py:92-104,396: one table of 262144 xoroshiro128p states, seeded once, advanced in place by
the kernels).  The table lives in the process-wide GPU context; state ``ip`` serves pixel row ``ip`` of a
``fee.get_adc_values`` call or of a chain launch.  The generator is third-party (module ``numba``) and restated from its
published algorithm (csrc/rng.h): noisy outputs are reproducible with a seed, not pinned to the reference's."""
import ctypes as C

import numpy as np

from . import lib

xoroshiro128p_dtype = np.dtype([("s0", "<u8"), ("s1", "<u8")], align=True)


class RngStates:
    """Handle to the device-resident state table."""

    def __init__(self, n, seed, ctx=None):
        self.n, self.seed = int(n), int(seed)
        self.ctx = ctx or lib.context()
        lib.check(lib.load().ldsim_rng_seed(self.ctx, C.c_uint64(self.seed & (2 ** 64 - 1)), C.c_int64(self.n)))

    def __len__(self):
        return self.n

    def copy_to_host(self, n=None):
        n = self.n if n is None else int(n)
        out = np.zeros(n, dtype=xoroshiro128p_dtype)
        lib.check(lib.load().ldsim_rng_states_download(self.ctx, lib.ptr(out), C.c_int64(n)))
        return out


def create_xoroshiro128p_states(n, seed=0, ctx=None):
    return RngStates(n, seed, ctx)


def maybe_create_rng_states(n, seed=0, rng_states=None, ctx=None):
    """cli/simulate_pixels.py:92-104: create the table, or extend a shorter one with a fresh
    ``create_xoroshiro128p_states(n - len, seed)`` chain; a long enough table is returned untouched."""
    if rng_states is None:
        return RngStates(n, seed, ctx)
    if int(n) > len(rng_states):
        lib.check(lib.load().ldsim_rng_extend(rng_states.ctx, C.c_int64(int(n)), C.c_uint64(int(seed) & (2 ** 64 - 1))))
        rng_states.n = int(n)
    return rng_states


# ---- keyed streams (opt-in: ChargeChain.seed_keyed, simulate_pixels.py --rng keyed) ----------------------------------------
# Every draw is Philox4x32-10 of (run seed, stage tag, stream key, draw index) (csrc/rng.h).  The stream keys are folds of the
# identity of what is simulated -- never of its position in a launch or in the call history -- so a keyed run gives the same
# numbers at any chunking, rank count or event subset.
MASK64 = (1 << 64) - 1
KEY_ROOT = 0x6A09E667F3BCC909
TAG_FEE, TAG_LIGHT_FLUCT, TAG_LIGHT_NOISE, TAG_MC, TAG_CHARGE = 1, 2, 3, 4, 5


def _fin(z):
    """SplitMix64's output function on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u64(x):
    """int / int array -> uint64 (two's complement for negative values)"""
    a = np.asarray(x)
    if a.dtype == np.uint64:
        return a
    return (a.astype(np.int64)).view(np.uint64) if a.dtype.kind in "iu" else np.asarray(int(x) & MASK64, dtype=np.uint64)


def key_mix(h, *fields):
    """fold identity fields into key h: h' = fin(h ^ fin(x + 0x9E3779B97F4A7C15)), field by field (rng.h key_mix);
    broadcasts over arrays"""
    h = _u64(h)
    for x in fields:
        with np.errstate(over="ignore"):
            h = _fin(h ^ _fin(_u64(x) + np.uint64(0x9E3779B97F4A7C15)))
    return h


def batch_key(i_mod, event_id, tpc_group, sub_batch):
    """key of one batch of batching.assign_batches' table: its identity (module, event, TPC group, sub-batch), not its index"""
    return int(key_mix(np.uint64(KEY_ROOT), i_mod, event_id, tpc_group, sub_batch))


def call_key(i_mod, event_id, tpc_group, sub_batch):
    """key of the light calls (response, triggers, detector noise) of one sub-batch; sub_batch -1: the empty group's
    waveforms"""
    return int(key_mix(np.uint64(KEY_ROOT), i_mod, event_id, tpc_group, sub_batch))


def batch_keys(table, i_mod):
    """one key per batch id of ``table`` (batching.assign_batches: rows (event, TPC group, sub-batch, n))"""
    t = np.asarray([(int(r[0]), int(r[1]), int(r[2])) for r in table], dtype=np.int64).reshape(-1, 3)
    return key_mix(np.uint64(KEY_ROOT), np.full(len(t), i_mod, dtype=np.int64), t[:, 0], t[:, 1], t[:, 2]).astype(np.uint64)


def keyed_draws(stream_keys, n_draws, first=0, tag=TAG_FEE, normal=True, ctx=None):
    """device draws [first, first + n_draws) of each keyed stream (ldsim_rng_keyed_normals / _uniforms), [n][n_draws] float32;
    the ctx must be in keyed mode"""
    keys = np.ascontiguousarray(stream_keys, dtype=np.uint64).ravel()
    out = np.zeros((len(keys), int(n_draws)), dtype=np.float32)
    f = lib.load().ldsim_rng_keyed_normals if normal else lib.load().ldsim_rng_keyed_uniforms
    lib.check(f(ctx or lib.context(), C.c_uint32(int(tag)), lib.ptr(keys), C.c_int64(len(keys)), C.c_uint32(int(first)),
                C.c_int32(int(n_draws)), lib.ptr(out)))
    return out
