"""GPU: every device buffer, stream and event of a context has an owner (csrc/ldsim_dev.h: DevBuf, Stream, Event), counted by
``ldsim_debug_live_objects``.  Nothing is left when the last context is destroyed, nothing is made again from one pass to the
next, a stage call or a cleared table gives back what it took.  Each test runs tests/ctx_lifetime_driver.py in a process of
its own (the suite's process-wide context is left alone) and asserts on the counts it wrote."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(TESTS, "ctx_lifetime_driver.py")
BUF, STREAM, EVENT = 0, 1, 2


def _drive(tmp_path, case, timeout=240):
    out = tmp_path / f"{case}.json"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, DRIVER, case, str(out)], env=env, capture_output=True, timeout=timeout)
    assert r.returncode == 0, (case, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
    with open(out) as f:
        res = json.load(f)
    print(case, json.dumps(res))
    return res


@pytest.fixture(scope="module")
def cycle(tmp_path_factory):
    """two full passes in one context, then its destruction (shared by the first two tests)"""
    return _drive(tmp_path_factory.mktemp("ctx_lifetime"), "cycle")


def test_full_cycle_then_destroy_leaves_nothing(cycle):
    """RNG table, field map, upload, quench_drift, light incidence, photon sums over the tile lists (once on the light stream)
    and with truth slots, light response, chain launches in two pair ranges with fractions, overlapped download, compact
    build and accumulation, hit accumulation: while the context lives all three counts are > 0 (the counter counts), after
    ldsim_ctx_destroy all three are exactly 0."""
    assert cycle["start"] == [0, 0, 0]
    assert all(c > 0 for c in cycle["pass1"]), cycle["pass1"]
    assert cycle["pass1"][STREAM] == 4, cycle["pass1"]        # main, copy, light and tables' stream
    assert cycle["same_adc"]
    assert cycle["destroyed"] == [0, 0, 0]


def test_second_pass_makes_nothing_new(cycle):
    """the same pass again in the same context on the same input: no buffer, stream or event more than after the first"""
    assert cycle["pass2"] == cycle["pass1"]


def test_stage_calls_leave_nothing_behind(tmp_path):
    """ldsim_track_pixel_map, ldsim_sum_pixel_signals, ldsim_get_adc_values, ldsim_digitize (12 pixel rows of the golden
    chain) and ldsim_scintillation_effect (8 detector rows): the counts right after each call equal those right before it"""
    res = _drive(tmp_path, "stage_calls")
    assert 8 <= res["rows"]["pixels"] <= 16 and 8 <= res["rows"]["detectors"] <= 16
    assert [c["name"] for c in res["calls"]] == ["ldsim_track_pixel_map", "ldsim_sum_pixel_signals", "ldsim_get_adc_values",
                                                 "ldsim_digitize", "ldsim_scintillation_effect"]
    for c in res["calls"]:
        assert c["after"] == c["before"], c
    assert res["did_work"]
    assert res["destroyed"] == [0, 0, 0]


def test_replacing_and_clearing_tables(tmp_path):
    """a second response table of another shape replaces the first (same count); pixel thresholds add a buffer that
    ldsim_clear_pixel_tables gives back; a field map (nodes, descriptors, anode view) is given back by ldsim_clear_field_maps"""
    res = _drive(tmp_path, "tables")
    assert res["response_2"][BUF] == res["response_1"][BUF]
    assert res["thresholds_set"][BUF] == res["response_2"][BUF] + 1
    assert res["tables_cleared"][BUF] == res["response_2"][BUF]
    assert res["map_set"][BUF] > res["before_map"][BUF]
    assert res["maps_cleared"][BUF] == res["before_map"][BUF]
    assert res["destroyed"] == [0, 0, 0]


def test_a_context_outlives_the_destruction_of_another(tmp_path):
    """two contexts, the first destroyed: the counts stay > 0, a chain in the second gives the adc_list it gave before, and
    its destruction brings all three counts to 0"""
    res = _drive(tmp_path, "two_contexts")
    assert all(c > 0 for c in res["first_destroyed"]), res
    assert all(a < b for a, b in zip(res["first_destroyed"], res["both"])), res
    assert res["same_adc"]
    assert res["destroyed"] == [0, 0, 0]
