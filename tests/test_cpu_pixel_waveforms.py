"""CPU: pixel current waveforms -- the numpy statement of the zero suppression (larndsim_amd/pixel_waveforms.py) on hand-made
arrays, the row conversion of the driver's two datasets, the driver's flag rules and the ABI row size.  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

from larndsim_amd import pixel_waveforms as PW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py")


def _cli():
    spec = importlib.util.spec_from_file_location("sp_cli_pixel_waveforms", CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _spans(S, thr=0.0, pad=0):
    b, n = PW.spans_of(S, thr, pad)
    return list(zip(b.tolist(), n.tolist()))


def test_spans_of_empty_and_all_zero():
    for pad in (0, 1, 64):
        assert _spans(np.zeros(0), 0.0, pad) == []
        assert _spans(np.zeros(200), 0.0, pad) == []
        assert _spans(np.ones(200), 1.5, pad) == []


def test_spans_of_one_active_tick_and_its_padding():
    S = np.zeros(300)
    S[100] = -2.5                                                    # (|S| counts: the sign does not)
    assert _spans(S, 0.0, 0) == [(100, 1)]
    assert _spans(S, 0.0, 1) == [(99, 3)]
    assert _spans(S, 0.0, 64) == [(36, 129)]


def test_spans_of_clips_at_tick_0_and_at_the_last_tick():
    N = 150
    S = np.zeros(N)
    S[0], S[N - 1] = 1.0, 1.0
    assert _spans(S, 0.0, 0) == [(0, 1), (N - 1, 1)]
    assert _spans(S, 0.0, 1) == [(0, 2), (N - 2, 2)]
    assert _spans(S, 0.0, 64) == [(0, 65), (N - 65, 65)]
    S = np.zeros(100)
    S[0], S[99] = 1.0, 1.0                                           # the clipped neighbourhoods meet: 0..64 and 35..99
    assert _spans(S, 0.0, 64) == [(0, 100)]


@pytest.mark.parametrize("pad", [0, 1, 7, 63, 64])
def test_spans_of_touching_neighbourhoods_merge_and_a_gap_of_one_does_not(pad):
    a = 70
    S = np.zeros(400)
    S[a], S[a + 2 * pad + 1] = 1.0, 1.0                              # a + pad and a + pad + 1 are neighbours: one span
    assert _spans(S, 0.0, pad) == [(a - pad, 4 * pad + 2)]
    S = np.zeros(400)
    S[a], S[a + 2 * pad + 2] = 1.0, 1.0                              # tick a + pad + 1 belongs to neither
    assert _spans(S, 0.0, pad) == [(a - pad, 2 * pad + 1), (a + pad + 2, 2 * pad + 1)]


def test_spans_of_a_run_across_a_multiple_of_64():
    S = np.zeros(256)
    S[60:70] = 3.0
    S[127:129] = -1.0
    assert _spans(S, 0.0, 0) == [(60, 10), (127, 2)]
    assert _spans(S, 0.0, 2) == [(58, 14), (125, 6)]
    S[:] = 1.0
    assert _spans(S, 0.0, 0) == [(0, 256)] and _spans(S, 0.0, 64) == [(0, 256)]


def test_spans_of_threshold_is_strict():
    S = np.array([0.0, 0.5, 1.0, -1.0, 1.0 + 2.0 ** -40, -2.0, 0.0])
    assert _spans(S, 1.0, 0) == [(4, 2)]                             # |S| == thr is not active
    assert _spans(S, 0.0, 0) == [(1, 5)]                             # 0: exactly the non-zero ticks
    assert _spans(S.astype(np.float32), 1.0, 0) == [(5, 1)]          # (1 + 2^-40 is 1 in f32: compared as given)


def test_bad_arguments_are_refused():
    for thr, pad in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -1), (0.0, 65), (0.0, 1.5)):
        with pytest.raises(ValueError):
            PW.spans_of(np.zeros(8), thr, pad)


def test_expand_of_compact_is_s_on_the_kept_ticks_and_zero_elsewhere():
    rng = np.random.default_rng(12)
    U, N = 7, 200
    S = (rng.normal(size=(U, N)) * (rng.random((U, N)) < 0.08)).astype(np.float32)
    S[3] = 0                                                         # a pixel without a span
    S[5, :3], S[5, -2:] = 1.0, 2.0                                   # clipped at both ends
    meta = dict(row=np.arange(U), pixel_id=np.arange(U) + 1000, batch=np.array([0, 0, 0, 1, 1, 2, 2]), n_hits=np.array([1, 0, 2, 0, 1, 1, 0]))
    for thr, pad in ((0.0, 0), (0.0, 3), (0.7, 1), (0.7, 64)):
        c = PW.compact_of(S, meta, thr, pad)
        kept = np.stack([PW.kept_of(S[u], thr, pad) for u in range(U)])
        assert np.array_equal(PW.expand(c["spans"], c["samples"], U, N), np.where(kept, S, np.float32(0)))
        sp = c["spans"]
        assert c["n_ticks"] == N and sp.dtype == PW.SPAN_ROW and c["samples"].dtype == np.float32
        assert len(c["samples"]) == kept.sum() == sp["n_samples"].sum()
        assert np.array_equal(sp["sample_begin"], np.cumsum(sp["n_samples"]) - sp["n_samples"])      # tiles the samples
        order = np.lexsort((sp["t_begin"], sp["row"]))
        assert np.array_equal(order, np.arange(len(sp))) and 3 not in sp["row"]
        assert np.array_equal(sp["pixel_id"], sp["row"] + 1000) and np.array_equal(sp["batch"], meta["batch"][sp["row"]])
        h = PW.compact_of(S, meta, thr, pad, hits_only=True)
        assert np.array_equal(PW.expand(h["spans"], h["samples"], U, N), np.where(kept & (meta["n_hits"] > 0)[:, None], S, np.float32(0)))
    none = PW.compact_of(S, meta, 100.0, 64)
    assert len(none["spans"]) == 0 and len(none["samples"]) == 0 and none["n_ticks"] == N
    with pytest.raises(ValueError, match="does not fit"):
        PW.expand(c["spans"], c["samples"][:-1], U, N)


def test_file_rows_map_batches_to_events_and_count_samples_over_the_file():
    sp = np.zeros(3, dtype=PW.SPAN_ROW)
    sp["row"], sp["pixel_id"], sp["batch"] = [0, 0, 4], [11, 11, 13], [0, 0, 1]
    sp["t_begin"], sp["n_samples"], sp["sample_begin"] = [5, 90, 7], [3, 2, 4], [0, 3, 5]
    sam = np.arange(9, dtype=np.float32)
    rows, out = PW.file_rows(dict(spans=sp, samples=sam, n_ticks=128), event_of_batch=[7, 9], sample_base=1000)
    assert rows.dtype == PW.FILE_SPAN and out.dtype == np.float32 and np.array_equal(out, sam)
    assert rows["event_id"].tolist() == [7, 7, 9] and rows["pixel_id"].tolist() == [11, 11, 13]
    assert rows["t_begin"].tolist() == [5, 90, 7] and rows["n_samples"].tolist() == [3, 2, 4]
    assert rows["sample_begin"].tolist() == [1000, 1003, 1005]
    with pytest.raises(ValueError, match="samples"):
        PW.file_rows(dict(spans=sp, samples=sam[:8], n_ticks=128), [7, 9])
    rows, out = PW.file_rows(dict(spans=sp[:0], samples=sam[:0], n_ticks=128), [7, 9], 5)
    assert len(rows) == 0 and len(out) == 0


def test_cli_pixel_waveforms_flag_rules(monkeypatch):
    cli = _cli()
    base = ["--input_filename", "x.npy", "--output_filename", "y.npz"]
    a = cli._parse_args(base)
    assert a.pixel_waveforms is False and a.pixel_waveforms_threshold is None and a.pixel_waveforms_pad is None
    assert a.pixel_waveforms_hits_only is False
    a = cli._parse_args(base + ["--pixel_waveforms", "--pixel_waveforms_threshold", "2.5", "--pixel_waveforms_pad", "64",
                                "--pixel_waveforms_hits_only"])
    assert a.pixel_waveforms and a.pixel_waveforms_threshold == 2.5 and a.pixel_waveforms_pad == 64 and a.pixel_waveforms_hits_only
    on = ["--pixel_waveforms"]
    for bad in (["--pixel_waveforms_threshold", "1"], ["--pixel_waveforms_pad", "2"], ["--pixel_waveforms_hits_only"],
                on + ["--pixel_waveforms_threshold", "-1"], on + ["--pixel_waveforms_threshold", "inf"],
                on + ["--pixel_waveforms_threshold", "nan"], on + ["--pixel_waveforms_pad", "-1"],
                on + ["--pixel_waveforms_pad", "65"]):
        with pytest.raises(SystemExit):
            cli._parse_args(base + bad)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    with pytest.raises(SystemExit, match="--pixel_waveforms is not available with --n_gpus > 1"):
        cli.launch_ranks_if_asked(base + ["--pixel_waveforms", "--n_gpus", "2"])
    assert cli.launch_ranks_if_asked(base + ["--pixel_waveforms"]) is None
    with pytest.raises(ValueError, match="--pixel_waveforms is not available with --n_gpus > 1"):
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", "0")
        cli.run_simulation("x.npy", "y.npz", n_gpus=2, pixel_waveforms=True)


def test_abi_span_row_is_the_header_struct():
    """SPAN_ROW against LdsimPixelWaveSpan as include/ldsim.h declares it: the fields in order, 32 bytes"""
    assert PW.SPAN_ROW.itemsize == 32 and PW.SPAN_ROW.fields["sample_begin"][1] == 24
    text = open(os.path.join(REPO, "include", "ldsim.h")).read()
    body = re.search(r"typedef struct LdsimPixelWaveSpan \{(.*?)\} LdsimPixelWaveSpan;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        fields += [(n.strip(), "i4" if ctype == "int32_t" else "i8") for n in names.split(",")]
    assert fields == [(n, PW.SPAN_ROW.fields[n][0].str[1:]) for n in PW.SPAN_ROW.names]
    assert "int ldsim_chain_pixel_waveforms(" in text and "LDSIM_ENOMEM" in text
