"""GPU: the FEE stage (fee_setup_kernel's per-pixel record -> pixel_adc kernels) against results recorded before the
stage was restructured.  The restructuring (launch constants computed once, one set-up pass per pixel) must not move any bit,
so the expected values are not tolerances but CRC-32s of the arrays' bytes.

Fixture: tests/golden/fee_setup_record.json, written by this file itself,

    python tests/test_fee_setup_record.py --record [PATH]

run on an MI355X with the library built from the commit before the change (the one whose pixel_adc_body counted its keys,
computed its tick range and built wtap[] / G[] per pixel).  For every case it holds the shape and the CRC-32 (zlib) of
adc_list, adc_ticks_list, adc_digit, track_pixel_map, current_fractions, unique_pix and of the compact download's hit
pixels, hit rows, hit charges, track segments and fractions, plus the hit and overflow counts.

Cases, on each of module0, 2x2_no_modvar and ndlar (3000 synthetic segments in one event, so that tracks cross):
  quiet     noise off: the one-wave instantiation over the set-up record, the 256-thread one for pixels whose slots' windows span
            more than FEE_SPAN ticks (the case counts such pixels on the host, n_wide: 114 on module0, 38 on 2x2, none on ndlar)
  one_class the same input with option fee_one_class: every pixel through the 256-thread instantiation without the record
  overflow  MAX_TRACKS_PER_PIXEL = 2: pixels with more pairs than slots (the case checks that the overflow counter moved)
  table     FEE noise from the xoroshiro table
  keyed     FEE noise from keyed streams, drawn inline in the scan
Every GPU run is a fresh process with a time limit of its own; nothing is retried."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "larnd-sim_amd")
TESTS = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(TESTS, "golden", "fee_setup_record.json")
CFGS = ("module0", "2x2_no_modvar", "ndlar")
CASES = ("quiet", "one_class", "overflow", "table", "keyed")
N_SEG = 3000
FEE_SPAN = 512          # csrc/kernels_fee.hip


def _crc(a):
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": a.dtype.str, "crc32": zlib.crc32(a.tobytes()) & 0xFFFFFFFF}


def _wide_pixels(out, seg_dev, bid):
    """pixels whose slots' segments are further apart in drift time than FEE_SPAN ticks: their windows cannot fit the
    one-wave instantiation's LDS, whatever the windows' own widths"""
    from larndsim_amd import consts
    first = {int(b): int(np.flatnonzero(bid == b)[0]) for b in np.unique(bid[bid >= 0])}
    tpm, t = out["track_pixel_map"], seg_dev["t"].astype(np.float64)
    base = np.array([first[int(b)] for b in out["batch"]])
    n = 0
    for u in np.flatnonzero((tpm >= 0).sum(axis=1) > 1):
        tt = t[base[u] + tpm[u][tpm[u] >= 0]]
        n += (tt.max() - tt.min()) / consts.detector.TIME_SAMPLING > FEE_SPAN
    return int(n)


def run_case(cfg, case):
    """one case in this process: {array name: shape / dtype / crc32, counters}"""
    import helpers as H
    from larndsim_amd import batching, consts, lib, synth
    from larndsim_amd.chain import ChargeChain
    H.load_cfg(cfg, noise_zero=case not in ("table", "keyed"))
    if case == "overflow":
        consts.sim.MAX_TRACKS_PER_PIXEL = 2
    seg = synth.make_segments(N_SEG, seed=synth.SEED_BASE + 31, segs_per_event=N_SEG)
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    seg, bid = np.ascontiguousarray(seg[order]), bid[order]
    ch = ChargeChain(synth.make_response("survey"))
    ch.upload(seg, bid)
    ch.quench_drift()
    if case == "table":
        ch.seed_rng(5)
    elif case == "keyed":
        ch.seed_keyed(5)
        ch.set_batch_keys(table, 1)
    if case == "one_class":
        lib.set_option("fee_one_class", 1, ch.ctx)
    n_sim = int((bid >= 0).sum())
    st = ch.run(0, n_sim, want_fractions=True)
    out = ch.download(fractions=True)
    cpt = ch.download_compact()
    res = {k: _crc(out[k]) for k in ("unique_pix", "adc_list", "adc_ticks_list", "adc_digit", "track_pixel_map",
                                     "current_fractions")}
    for k in ("hit_pixels", "track_segments", "hit_rows", "hit_charge", "fractions"):
        res["compact_" + k] = _crc(cpt[k])
    res["n_unique"] = int(st.n_unique)
    res["n_overflow"] = int(st.n_overflow)
    res["n_hits"] = int((out["adc_list"] != 0).sum())
    res["hit_count_rows"] = int(ch.compact_hits()[1])
    if case == "quiet":
        res["n_wide"] = _wide_pixels(out, ch.download_segments(seg.copy()), bid)
    return res


def _child(cfg):
    """all cases of a configuration, each in a fresh process; stops at the first that fails"""
    got = {}
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", cfg, case], capture_output=True, timeout=300,
                           env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
        assert r.returncode == 0, (cfg, case, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
        line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("FEECASE ")][-1]
        got[case] = json.loads(line[8:])
    return got


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", CFGS)
def test_fee_outputs_equal_recorded(cfg):
    """every array of every case has the recorded shape and CRC-32; the cases exercise what they are named for"""
    with open(FIXTURE) as f:
        want = json.load(f)[cfg]
    got = _child(cfg)
    for case in CASES:
        g, w = got[case], want[case]
        print(cfg, case, {k: v for k, v in g.items() if not isinstance(v, dict)})
        assert g["n_unique"] > 2000 and g["n_hits"] > 500, (case, g["n_unique"], g["n_hits"])
        for k in w:
            assert g[k] == w[k], (cfg, case, k, g[k], w[k])
    if cfg != "ndlar":         # (no such pixel among ndlar's 3000 segments, recorded as n_wide 0: there one_class alone covers the form)
        assert got["quiet"]["n_wide"] > 0, "no pixel with windows wider than FEE_SPAN: the 256-thread list stayed empty"
    assert got["overflow"]["n_overflow"] > 0, "no pixel with more pairs than MAX_TRACKS_PER_PIXEL"
    assert got["quiet"]["n_overflow"] < got["overflow"]["n_overflow"]
    # the two instantiations agree with each other, not only each with its record
    for k in got["quiet"]:
        if k != "n_wide":
            assert got["quiet"][k] == got["one_class"][k], (cfg, k)
    # noise moves the results (the noisy cases are not the quiet one under another name)
    for noisy in ("table", "keyed"):
        assert got[noisy]["adc_list"] != got["quiet"]["adc_list"], noisy
    assert got["table"]["adc_list"] != got["keyed"]["adc_list"]


if __name__ == "__main__":
    sys.path[:0] = [PKG, TESTS]
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        print("FEECASE " + json.dumps(run_case(sys.argv[2], sys.argv[3])))
    elif len(sys.argv) in (2, 3) and sys.argv[1] == "--record":
        rec = {cfg: _child(cfg) for cfg in CFGS}
        path = sys.argv[2] if len(sys.argv) == 3 else FIXTURE
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print("recorded", path)
    else:
        raise SystemExit("usage: test_fee_setup_record.py --record [PATH] | --case CFG CASE")
