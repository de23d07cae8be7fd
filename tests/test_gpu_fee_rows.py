"""GPU: the FEE stage on hand-placed segments -- the shapes a grouped, clamped, register-resident row loop can get wrong and
that random tracks do not aim at.  pixel_adc_body requests the waveform rows of a pixel's slots in groups (several slots' loads
ahead of one wait, addresses clamped into the row, the window test at the add); that must not move any bit, so the expected
values are not tolerances but CRC-32s of the arrays' bytes, recorded with the library of the commit before the change.

Fixture: tests/golden/fee_rows.json, written by this file itself,

    python tests/test_gpu_fee_rows.py --record [PATH]

run on an MI355X with the library built from the parent commit (the one whose pixel_adc_body added each slot's row into LDS,
one load waited for per 64 ticks).  For every configuration and case it holds the shape and the CRC-32 (zlib) of unique_pix,
adc_list, adc_ticks_list, adc_digit, track_pixel_map, current_fractions and of the compact download's hit pixels, hit rows, hit
charges, track segments and fractions, plus the counters the assertions below read.

The segments (about 300, one event, one TPC, module0 and ndlar: M = 1 and 2) come in clusters three centimetres apart.  The
segments of a cluster lie on the same 2 mm line in the pixel plane and differ in drift depth only, so every pixel of the cluster
holds a pair of each of them, in segment order, at staggered drift times:
  slot counts   clusters of 1, 3, 4, 5, 8, 9, 49, 50, 51 and 60 segments within 300 ticks of drift: counts around any group size,
                MAX_TRACKS_PER_PIXEL = 50, and past it (overflow); the large ones carry enough charge for repeated hits, the
                single segment too little for one
  cut windows   a cluster next to the anode (its windows start before tick 0), one at the cathode, delayed so that its windows run
                past the last tick, and one of three whose middle segment arrives after the time axis ends (an empty window
                between two live slots)
  class border  a ladder of two-segment clusters, 300 .. 460 ticks apart in steps of 8: with windows of 100-160 ticks the spans
                of their pixels step through FEE_SPAN = 512, the border between the one-wave and the 256-thread form
Cases: default options, and fee_one_class (every pixel through the 256-thread form); they must agree on every array.
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
FIXTURE = os.path.join(TESTS, "golden", "fee_rows.json")
CFGS = ("module0", "ndlar")
CASES = ("default", "one_class")
FEE_SPAN = 512          # csrc/kernels_fee.hip
SLOT_COUNTS = (1, 3, 4, 5, 8, 9, 49, 50, 51, 60)
LADDER = tuple(range(300, 461, 8))
ARRAYS = ("unique_pix", "adc_list", "adc_ticks_list", "adc_digit", "track_pixel_map", "current_fractions")
COMPACT = ("hit_pixels", "track_segments", "hit_rows", "hit_charge", "fractions")


def _crc(a):
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": a.dtype.str, "crc32": zlib.crc32(a.tobytes()) & 0xFFFFFFFF}


def make_clusters():
    """the segments (edep-sim frame, like synth.make_segments) and, per cluster, (name, first segment, count)"""
    from larndsim_amd import consts
    from larndsim_amd.layout import segments_dtype
    det = consts.detector
    b = np.asarray(det.TPC_BORDERS)[0]
    (xlo, xhi), (ylo, yhi) = sorted(b[0]), sorted(b[1])
    z_anode, z_cathode = b[2][0], b[2][1]
    sgn = np.sign(z_cathode - z_anode)
    t_max = abs(z_cathode - z_anode) / det.V_DRIFT            # us of drift from the cathode
    t_axis = float(det.TIME_INTERVAL[1])
    n_col = int((xhi - xlo - 12.0) / 3.0)
    rows, clusters = [], []

    def cluster(name, drift_us, dedx, length=0.2, t0=None):
        """segments at drift times drift_us (us) on the cluster's line; t0: their event times"""
        i = len(clusters)
        xc, yc = xlo + 6.0 + 3.0 * (i % n_col), ylo + 6.0 + 3.0 * (i // n_col)
        assert yc < yhi - 6.0
        clusters.append((name, len(rows), len(drift_us)))
        for k, t in enumerate(drift_us):
            z = z_anode + sgn * t * det.V_DRIFT
            rows.append((xc - length / 2, yc, z, xc + length / 2, yc + 0.02, z + sgn * 0.01, dedx, 0.0 if t0 is None else t0[k]))

    for n in SLOT_COUNTS:
        step = min(40, 300 // max(n - 1, 1))
        cluster("slots%d" % n, [80.0 + k * step * det.TIME_SAMPLING for k in range(n)],
                dedx=0.15 if n == 1 else (6.0 if n >= 49 else 2.1), length=0.05 if n == 1 else 0.2)
    cluster("cut0", [0.4, 1.5], dedx=4.0)
    cluster("cutend", [t_max - 0.5, t_max - 3.5], dedx=4.0, t0=[t_axis - t_max + 2.5] * 2)       # (arrive at the axis' end + 2, - 1 us)
    cluster("empty", [100.0, 100.0, 102.0], dedx=4.0, t0=[0.0, t_axis - 100.0 + 30.0, 0.0])
    for d in LADDER:
        cluster("ladder%d" % d, [60.0, 60.0 + d * det.TIME_SAMPLING], dedx=4.0)
    r = np.array(rows)
    out = np.zeros(len(rows), dtype=segments_dtype)
    # edep-sim frame: drift (TPC z) axis is stored in "x", TPC x in "z" (synth.make_segments)
    out["z_start"], out["y_start"], out["x_start"] = r[:, 0], r[:, 1], r[:, 2]
    out["z_end"], out["y_end"], out["x_end"] = r[:, 3], r[:, 4], r[:, 5]
    for ax in "xyz":
        out[ax] = 0.5 * (out[ax + "_start"].astype(np.float64) + out[ax + "_end"])
    out["dx"] = np.sqrt(((r[:, 3:6] - r[:, 0:3]) ** 2).sum(axis=1))
    out["dEdx"] = r[:, 6]
    out["dE"] = out["dEdx"].astype(np.float64) * out["dx"]
    assert "t0" in out.dtype.names
    for f in ("t0", "t0_start", "t0_end"):
        if f in out.dtype.names:
            out[f] = r[:, 7]
    for f in ("traj_id", "file_traj_id"):
        if f in out.dtype.names:
            out[f] = np.arange(len(rows))
    if "segment_id" in out.dtype.names:
        out["segment_id"] = np.arange(len(rows))
    if "pdg_id" in out.dtype.names:
        out["pdg_id"] = 13
    return out, clusters


def run_case(cfg, case):
    """one case in this process: {array name: shape / dtype / crc32, what the case reached}"""
    import helpers as H
    from larndsim_amd import batching, consts, lib
    from larndsim_amd.chain import ChargeChain
    from larndsim_amd import synth
    H.load_cfg(cfg, noise_zero=True)
    seg, clusters = make_clusters()
    batching.swap_coordinates(seg)
    bid, order, table = batching.assign_batches(seg)
    assert (bid == 0).all() and (order == np.arange(len(seg))).all(), "one batch, segments in the order they were placed"
    ch = ChargeChain(synth.make_response("survey"))
    ch.upload(seg, bid)
    ch.quench_drift()
    if case == "one_class":
        lib.set_option("fee_one_class", 1, ch.ctx)
    st = ch.run(0, len(seg), want_fractions=True)
    out = ch.download(fractions=True)
    cpt = ch.download_compact()
    res = {k: _crc(out[k]) for k in ARRAYS}
    for k in COMPACT:
        res["compact_" + k] = _crc(cpt[k])
    # ---- what the case reached, from its own results ----
    M, NT = consts.sim.MAX_TRACKS_PER_PIXEL, len(consts.detector.TIME_TICKS)
    tpm = out["track_pixel_map"]
    n_slots = (tpm >= 0).sum(axis=1)
    hits = (out["adc_list"] != 0).sum(axis=1)
    # the cluster of a pixel's first slot (-1: a pixel without slots)
    owner = np.where(tpm[:, 0] >= 0, np.searchsorted([c[1] for c in clusters], tpm[:, 0], side="right") - 1, -1)
    name = [c[0] for c in clusters]
    res["n_unique"] = int(st.n_unique)
    res["n_overflow"] = int(st.n_overflow)
    res["n_hits"] = int(hits.sum())
    res["slot_counts"] = {name[i]: sorted(set(int(v) for v in n_slots[owner == i])) for i in range(len(SLOT_COUNTS))}
    res["pixels_of"] = {name[i]: int((owner == i).sum()) for i in range(len(clusters))}
    res["max_hits"] = int(hits.max())
    res["pixels_without_hit"] = int((hits == 0).sum())
    # a later hit right behind a reset: the smallest distance between successive hits of a pixel with three or more, in us
    tk = out["adc_ticks_list"]
    gaps = [np.diff(tk[u, :hits[u]]).min() for u in np.flatnonzero(hits >= 3)]
    res["min_hit_gap_us"] = float(min(gaps)) if gaps else -1.0
    # the ticks a pixel's summed waveform is non-zero over: inside its slots' windows, so a span of them is a lower bound of the
    # windows' span
    S = ch.pixel_waveforms(dense=True)
    nz = S != 0
    has = nz.any(axis=1)
    lo = np.where(has, nz.argmax(axis=1), NT)
    hi = np.where(has, NT - nz[:, ::-1].argmax(axis=1), 0)
    span = np.where(has, hi - lo, 0)
    res["cut_by_tick0"] = int((nz[:, 0] & (owner == name.index("cut0"))).sum())
    res["cut_by_last_tick"] = int((nz[:, NT - 1] & (owner == name.index("cutend"))).sum())
    t = ch.download_segments(seg.copy())["t"].astype(np.float64)
    e0 = clusters[name.index("empty")][1]
    res["empty_arrival_tick"] = float(t[e0 + 1] / consts.detector.TIME_SAMPLING)
    res["empty_slots"] = sorted(set(int(v) for v in n_slots[owner == name.index("empty")]))
    res["empty_middle_is_slot1"] = bool((tpm[owner == name.index("empty"), 1] == e0 + 1).all())
    res["spans_below_border"] = int(((span > FEE_SPAN - 64) & (span <= FEE_SPAN)).sum())
    res["spans_above_border"] = int(((span > FEE_SPAN) & (span <= FEE_SPAN + 64)).sum())
    res["first_hit_far_from_tick0"] = int(((hits > 0) & (lo > 500)).sum())
    res["n_time_ticks"], res["max_tracks"] = NT, M
    return res


def check_reached(cfg, g):
    """the case exercised what its clusters are named for"""
    M = g["max_tracks"]
    for n in SLOT_COUNTS:
        assert g["pixels_of"]["slots%d" % n] > 0, (cfg, n)
        assert g["slot_counts"]["slots%d" % n] == [min(n, M)], (cfg, n, g["slot_counts"])
    n_past = g["pixels_of"]["slots51"] + g["pixels_of"]["slots60"]
    assert g["n_overflow"] == n_past > 0, (cfg, g["n_overflow"], n_past)
    assert g["max_hits"] >= 3, (cfg, g["max_hits"])
    # hold 15 + busy 9 + reset 1 clock cycles of 0.1 us lie between a trigger and the first tick that can trigger again
    assert 0 < g["min_hit_gap_us"] <= 4.0, (cfg, g["min_hit_gap_us"])
    assert g["pixels_without_hit"] >= g["pixels_of"]["slots1"] > 0, (cfg, g["pixels_without_hit"])
    assert g["first_hit_far_from_tick0"] > 0, cfg
    assert g["cut_by_tick0"] > 0, cfg
    assert g["cut_by_last_tick"] > 0, cfg
    # (a row's window ends less than 200 ticks behind the segment's arrival: 100 past the axis, it is empty)
    assert g["empty_arrival_tick"] > g["n_time_ticks"] + 100, (cfg, g["empty_arrival_tick"])
    assert g["empty_slots"] == [3] and g["empty_middle_is_slot1"], (cfg, g["empty_slots"])
    assert g["spans_below_border"] > 0 and g["spans_above_border"] > 0, (cfg, g["spans_below_border"], g["spans_above_border"])
    assert g["n_hits"] > 50, (cfg, g["n_hits"])


def _child(cfg):
    """the cases of a configuration, each in a fresh process; stops at the first that fails"""
    got = {}
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", cfg, case], capture_output=True, timeout=300,
                           env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
        assert r.returncode == 0, (cfg, case, r.stdout.decode()[-1500:], r.stderr.decode()[-3000:])
        line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("FEEROWS ")][-1]
        got[case] = json.loads(line[8:])
    return got


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", CFGS)
def test_fee_rows_equal_recorded(cfg):
    """every array of both cases has the recorded shape and CRC-32, the cases agree, and the clusters reached their shapes"""
    with open(FIXTURE) as f:
        want = json.load(f)[cfg]
    got = _child(cfg)
    for case in CASES:
        g = got[case]
        print(cfg, case, {k: v for k, v in g.items() if not (isinstance(v, dict) and "crc32" in v)})
        check_reached(cfg, g)
        for k in want[case]:
            assert g[k] == want[case][k], (cfg, case, k, g[k], want[case][k])
    # the two forms agree with each other, not only each with its record
    for k in got["default"]:
        assert got["default"][k] == got["one_class"][k], (cfg, k)


if __name__ == "__main__":
    sys.path[:0] = [PKG, TESTS]
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        print("FEEROWS " + json.dumps(run_case(sys.argv[2], sys.argv[3])))
    elif len(sys.argv) in (2, 3) and sys.argv[1] == "--record":
        rec = {cfg: _child(cfg) for cfg in CFGS}
        for cfg in CFGS:
            for case in CASES:
                print(cfg, case, {k: v for k, v in rec[cfg][case].items() if not (isinstance(v, dict) and "crc32" in v)})
        path = sys.argv[2] if len(sys.argv) == 3 else FIXTURE
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print("recorded", path)
        for cfg in CFGS:
            for case in CASES:
                check_reached(cfg, rec[cfg][case])
        print("every case reached its shapes")
    else:
        raise SystemExit("usage: test_gpu_fee_rows.py --record [PATH] | --case CFG CASE")
