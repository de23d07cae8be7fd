"""CPU: pixel charge truth -- the numpy restatement of its definition (larndsim_amd/pixel_truth.py) on hand-made rows, the row
conversion of the driver's two datasets, and the driver's flag rules.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from larndsim_amd import pixel_truth as PT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_pixel_truth", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_restatement_clips_the_window_at_tick_0_and_at_nt():
    """a row that starts before tick 0 loses its first elements, one that runs past N_t its last; values exact in f64"""
    dt, NT, T = 0.5, 16, 8
    row = np.arange(1, T + 1, dtype=np.float32)                      # 1 .. 8
    r = PT.restate([row], [-3], [(0, T)], dt, NT)                    # elements 3.. land on ticks 0..4
    assert r["q_track"][0] == dt * (4 + 5 + 6 + 7 + 8)
    assert r["q_induced"] == r["q_track"][0] == r["q_abs"]
    r = PT.restate([row], [NT - 3], [(0, T)], dt, NT)                # elements 0..2 land on ticks 13..15
    assert r["q_track"][0] == dt * (1 + 2 + 3) == r["q_induced"]
    r = PT.restate([row], [2], [(2, 5)], dt, NT)                     # only the window's elements count
    assert r["q_track"][0] == dt * (3 + 4 + 5)
    r = PT.restate([row], [NT + 4], [(0, T)], dt, NT)                # wholly outside
    assert r["q_track"][0] == 0 and r["q_induced"] == 0 and r["q_abs"] == 0
    r = PT.restate([row], [-2], [(-5, T + 9)], dt, NT)               # a window wider than the row is the row
    assert r["q_track"][0] == dt * (3 + 4 + 5 + 6 + 7 + 8)


def test_restatement_empty_window_and_empty_pixel():
    dt, NT = 0.1, 32
    rows = np.ones((2, 10), dtype=np.float32)
    r = PT.restate(rows, [4, 4], [(3, 3), (0, 10)], dt, NT)          # slot 0: w0 == w1
    assert r["q_track"][0] == 0 and r["q_track"][1] == dt * 10
    assert r["q_induced"] == dt * 10 and r["q_abs"] == dt * 10
    r = PT.restate(np.zeros((0, 10), dtype=np.float32), [], np.zeros((0, 2), dtype=int), dt, NT)
    assert r["q_track"].shape == (0,) and r["q_induced"] == 0 and r["q_abs"] == 0 and r["n_hits"] == 0 and r["q_hits"] == 0


def test_restatement_opposite_signs_overlap():
    """two slots of opposite sign that overlap in part: |S| is taken after the sum, so q_abs lies between |q_induced| and the
    sum of the slots' own absolute charges"""
    dt, NT = 0.25, 64
    a = np.full(12, 2.0, dtype=np.float32)
    b = np.full(12, -1.5, dtype=np.float32)
    r = PT.restate([a, b], [10, 16], [(0, 12), (0, 12)], dt, NT)     # a: ticks 10..21, b: 16..27, overlap 16..21
    assert r["q_track"][0] == dt * 24 and r["q_track"][1] == dt * -18
    assert r["q_induced"] == dt * 6
    assert r["q_abs"] == dt * (6 * 2.0 + 6 * 0.5 + 6 * 1.5)
    assert r["q_abs"] > abs(r["q_induced"])
    assert r["q_abs"] < dt * (24 + 18)
    # a pixel that only saw induction: a bipolar row that sums to nothing
    bip = np.r_[np.full(5, 3.0), np.full(5, -3.0)].astype(np.float32)
    r = PT.restate([bip], [0], [(0, 10)], dt, NT)
    assert r["q_induced"] == 0 and r["q_abs"] == dt * 30


def test_restatement_reads_rows_as_f32_and_sums_in_slot_order():
    dt, NT = 1.0, 8
    rows = np.array([[1e8, 0.0], [1.0, 0.0], [-1e8, 0.0]])           # f64 in: narrowed to f32 first
    r = PT.restate(rows, [0, 0, 0], [(0, 2)] * 3, dt, NT)
    assert r["q_induced"] == 1.0                                     # (1e8 + 1) - 1e8 in f64, slot order
    tiny = np.array([[1.0 + 2.0 ** -30]])
    assert PT.restate(tiny, [0], [(0, 1)], dt, NT)["q_induced"] == 1.0


def test_hits_of_counts_the_filled_slots_and_sums_them_in_order():
    adc = np.zeros((3, 6))
    adc[0, :3] = [1e16, 1.0, -1e16]
    adc[2, :1] = [7.5]
    n, q = PT.hits_of(adc)
    assert n.tolist() == [3, 0, 1]
    assert q.tolist() == [(1e16 + 1.0) - 1e16, 0.0, 7.5]
    r = PT.restate(np.ones((1, 4), np.float32), [0], [(0, 4)], 1.0, 8, adc=adc[0])
    assert r["n_hits"] == 3 and r["q_hits"] == q[0]


def test_file_rows_map_batches_and_segments_and_count_over_the_file():
    px = np.zeros(3, dtype=PT.PIXEL_ROW)
    px["row"], px["pixel_id"], px["batch"] = [0, 2, 5], [11, 12, 13], [0, 0, 2]
    px["n_hits"], px["n_tracks"] = [1, 0, 2], [2, 0, 1]
    px["q_hits"], px["q_induced"], px["q_abs"] = [5.0, 0.0, 9.0], [4.0, 0.1, 8.0], [4.5, 0.3, 8.5]
    tr = np.zeros(3, dtype=PT.TRACK_ENTRY)
    tr["segment"], tr["q"] = [0, 3, 1], [1.0, 3.0, 8.0]
    seg_ids = np.arange(100, 120)
    rows, ent = PT.file_rows(dict(pixels=px, tracks=tr), event_of_batch=[7, 7, 9], first_segment_of_batch=[0, 4, 10],
                             segment_ids=seg_ids, track_base=40)
    assert rows.dtype == PT.FILE_PIXEL and ent.dtype == PT.FILE_TRACK
    assert rows["event_id"].tolist() == [7, 7, 9] and rows["pixel_id"].tolist() == [11, 12, 13]
    assert rows["track_begin"].tolist() == [40, 42, 42] and rows["track_count"].tolist() == [2, 0, 1]
    assert ent["segment_id"].tolist() == [100, 103, 111] and ent["q"].tolist() == [1.0, 3.0, 8.0]
    for k in ("n_hits", "q_hits", "q_induced", "q_abs"):
        assert np.array_equal(rows[k], px[k])
    with pytest.raises(ValueError, match="track entries"):
        PT.file_rows(dict(pixels=px, tracks=tr[:2]), [7, 7, 9], [0, 4, 10], seg_ids)


def test_cli_pixel_truth_flag_rules(monkeypatch):
    cli = _cli()
    base = ["--input_filename", "x.npy", "--output_filename", "y.npz"]
    a = cli._parse_args(base)
    assert a.pixel_truth is False and a.pixel_truth_min_charge is None
    a = cli._parse_args(base + ["--pixel_truth"])
    assert a.pixel_truth is True and a.pixel_truth_min_charge is None
    a = cli._parse_args(base + ["--pixel_truth", "--pixel_truth_min_charge", "250"])
    assert a.pixel_truth_min_charge == 250.0
    for bad in (["--pixel_truth_min_charge", "10"], ["--pixel_truth", "--pixel_truth_min_charge", "-1"],
                ["--pixel_truth", "--pixel_truth_min_charge", "inf"], ["--pixel_truth", "--pixel_truth_min_charge", "nan"]):
        with pytest.raises(SystemExit):
            cli._parse_args(base + bad)
    # more than one rank: refused before any rank is started, like --raw_arrays
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    with pytest.raises(SystemExit, match="--pixel_truth is not available with --n_gpus > 1"):
        cli.launch_ranks_if_asked(base + ["--pixel_truth", "--n_gpus", "2"])
    assert cli.launch_ranks_if_asked(base + ["--pixel_truth"]) is None          # one GPU, no launcher: nothing to start
    with pytest.raises(ValueError, match="--pixel_truth is not available with --n_gpus > 1"):
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", "0")
        cli.run_simulation("x.npy", "y.npz", n_gpus=2, pixel_truth=True)
