"""CPU: the key bits the chain's pair-list sort looks at (ldsim_debug_sort_key_ranges, host arithmetic of sort.hip).

key = batch << 36 | pixel << 4 | ring code.  The launch sorts [0, e0) and then, stably, [b1, e1): the order is that of one sort
over [0, 36 + bb) if and only if no key has a bit set outside the two ranges.  The split is taken only where it saves an 8-bit
pass of the radix sort; else the single range [0, 36 + bb) comes back."""
import ctypes as C

import pytest

from larndsim_amd import lib

K = (7, 8, 15, 16, 20)
PIXEL_MAX = sorted({(1 << k) - 1 for k in K} | {1 << k for k in K})
N_BATCHES = (1, 2, 3, 256, 257)
RADIX_BITS = 8


def _ranges(pixel_max, n_batches):
    r = (C.c_int32 * 3)()
    lib.check(lib.load().ldsim_debug_sort_key_ranges(C.c_uint64(pixel_max), C.c_int64(n_batches), r))
    return tuple(r)


def _passes(bits):
    return -(-bits // RADIX_BITS)


@pytest.mark.parametrize("n_batches", N_BATCHES)
@pytest.mark.parametrize("pixel_max", PIXEL_MAX)
def test_every_key_is_zero_outside_the_ranges(pixel_max, n_batches):
    e0, b1, e1 = _ranges(pixel_max, n_batches)
    assert 0 < e0 <= 64 and 0 <= b1 <= e1 <= 64
    covered = (1 << e0) - 1
    if e1 > b1:
        assert b1 >= e0                      # the second range lies above the first one
        covered |= ((1 << e1) - 1) & ~((1 << b1) - 1)
    # the keys with the most bits set: the largest batch, pixel and ring code, and each of them alone; every other key of the
    # launch has its bits inside the union of the fields these fill up to their highest bit
    fields = [(n_batches - 1) << 36, pixel_max << 4, 15]
    top = lambda v: (1 << v.bit_length()) - 1      # every value below v lies under this mask
    for f, shift in zip(fields, (36, 4, 0)):
        assert (top(f >> shift) << shift) & ~covered == 0, (hex(f), e0, b1, e1)


@pytest.mark.parametrize("n_batches", N_BATCHES)
@pytest.mark.parametrize("pixel_max", PIXEL_MAX)
def test_single_range_unless_a_pass_is_saved(pixel_max, n_batches):
    e0, b1, e1 = _ranges(pixel_max, n_batches)
    bb = (n_batches - 1).bit_length()
    single = 36 + bb
    split = _passes(4 + pixel_max.bit_length()) + _passes(bb)
    if split < _passes(single):
        assert e0 == 4 + pixel_max.bit_length()
        assert (b1, e1) == ((36, 36 + bb) if bb else (0, 0))
        assert _passes(e0) + _passes(e1 - b1) < _passes(single)
    else:
        assert (e0, b1, e1) == (single, 0, 0)


def test_module0_sorts_four_passes_instead_of_six():
    # module0: 140 x 280 pixels in 2 TPCs, 20 batches per launch of the bench
    e0, b1, e1 = _ranges(140 * 280 * 2 - 1, 20)
    assert (e0, b1, e1) == (4 + 17, 36, 41) and _passes(e0) + _passes(e1 - b1) == 4 and _passes(41) == 6


def test_bad_arguments_are_refused():
    r = (C.c_int32 * 3)()
    assert lib.load().ldsim_debug_sort_key_ranges(C.c_uint64(1), C.c_int64(0), r) != 0
    assert lib.load().ldsim_debug_sort_key_ranges(C.c_uint64(1), C.c_int64(1), None) != 0
