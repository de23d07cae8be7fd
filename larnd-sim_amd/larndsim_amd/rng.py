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
TAG_FEE, TAG_LIGHT_FLUCT, TAG_LIGHT_NOISE, TAG_MC, TAG_CHARGE, TAG_LUT = 1, 2, 3, 4, 5, 6
TAG_GEN = 7      # the track generator's walks and sources (track_generator.py)


def philox4x32_10(ctr, key):
    """Philox4x32-10 in numpy (csrc/rng.h philox4x32_10): ctr [..][4], key [..][2] -> [..][4] uint32"""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i].copy() for i in range(4)]
    k0 = np.asarray(key, dtype=np.uint64)[..., 0].copy()
    k1 = np.asarray(key, dtype=np.uint64)[..., 1].copy()
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def keyed_block_uniforms(seed, tag, keys, m):
    """the four uniforms of Philox block ``m`` of each keyed stream (draws 4m .. 4m + 3; csrc/rng.h keyed_block, keyed_u01),
    [..][4] float32 in (0, 1], on the host"""
    keys, m = np.broadcast_arrays(np.asarray(keys, dtype=np.uint64), np.asarray(m, dtype=np.uint64))
    seed = int(seed) & MASK64
    ctr = np.stack([m, keys & np.uint64(0xFFFFFFFF), keys >> np.uint64(32), np.full(keys.shape, tag, dtype=np.uint64)], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), keys.shape + (2,))
    x = philox4x32_10(ctr, key)
    return ((x >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


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
