"""CPU: host-side logic, ABI surface and fixtures (no compute calls into the HIP library)."""
import ctypes as C
import json
import os
import re
import tarfile

import numpy as np
import pytest

import helpers as H
from larndsim_amd import abi, batching, consts, layout, lib, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """larndsim/ of a larnd-sim tree's settings files (config.yaml, the YAML files it names for module0, 2x2, 2x2_no_modvar and
    ndlar, the SiPM impulse file they point to), unpacked from tests/golden/larndsim_tree.tar.gz (tests/golden/larndsim_tree.md)"""
    root = tmp_path_factory.mktemp("larndsim_tree")
    with tarfile.open(os.path.join(REPO, "tests", "golden", "larndsim_tree.tar.gz")) as t:
        t.extractall(root, **({"filter": "data"} if hasattr(tarfile, "data_filter") else {}))
    return str(root / "larndsim")


def test_library_loads_and_exports_every_declared_symbol():
    l = lib.load()
    hdr = open(os.path.join(REPO, "include", "ldsim.h")).read()
    declared = set(re.findall(r"\b(ldsim_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(l, name), f"{name} declared in include/ldsim.h but not exported"
    assert set(lib.EXPORTS) == declared
    assert l.ldsim_abi_version() == abi.ABI_VERSION == 8


def test_gform_census_slots_match_header():
    """abi.GFORM_CENSUS_SLOTS names the LDSIM_GC_* enumerators of include/ldsim.h in their order; LDSIM_GFORM_CENSUS_N closes it."""
    hdr = open(os.path.join(REPO, "include", "ldsim.h")).read()
    body = hdr[hdr.index("LDSIM_GC_PAIRS = 0"):hdr.index("LDSIM_GFORM_CENSUS_N\n")]
    names = re.findall(r"\bLDSIM_GC_([A-Z0-9_]+)\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert tuple(n.lower() for n in names) == abi.GFORM_CENSUS_SLOTS
    assert abi.GFORM_CENSUS_N == len(names) == 32 and len(set(names)) == 32


def test_graft_entry_build_succeeds():
    """The driver's build check: __graft_entry__.build() compiles the HIP library and the oracle and imports the package
    (an incremental make here).  It once asserted a stale ABI version after the header had moved on."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("graft_entry", os.path.join(REPO, "__graft_entry__.py"))
    ge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ge)
    ge.build()
    assert callable(ge.smoke)


def test_no_cpu_fallback_without_gpu():
    if lib.device_count() > 0:
        pytest.skip("GPU present")
    H.load_cfg("module0")
    with pytest.raises(lib.LdsimError, match="no HIP device|no CPU fallback"):
        lib.context()


def test_struct_layouts_match_header():
    # offsets of a few sentinel fields, computed from the C declaration order
    c = abi.LdsimConsts
    assert c.tpc_borders.offset == 13 * 8 + 8
    assert c.n_pixels.offset == c.tpc_borders.offset + 128 * 6 * 8
    assert C.sizeof(abi.LdsimTrackLayout) == 4 + 2 * 4 * layout.NFIELDS
    assert C.sizeof(abi.LdsimChainStats) == 5 * 8 + 4 * 4 + 5 * 8


def test_segments_dtype_is_the_edep_sim_schema():
    dt = layout.segments_dtype
    assert dt.itemsize == 152
    expect = dict(event_id=0, vertex_id=8, segment_id=24, z_end=28, n_electrons=56, t0_start=80, t0=96,
                  pixel_plane=112, dEdx=120, x=136, z=140, n_photons=144)
    for k, v in expect.items():
        assert dt.fields[k][1] == v, k
    lay = layout.make_layout(dt)
    assert lay.itemsize == 152 and lay.dtype[layout.FIELDS.index("n_electrons")] == layout.U4
    f8 = np.dtype([("dEdx", "f8"), ("dE", "f8"), ("n_electrons", "f8"), ("n_photons", "f8")])
    lay8 = layout.make_layout(f8)
    assert lay8.offset[layout.FIELDS.index("x")] == -1


@pytest.mark.parametrize("cfg,files", [
    ("module0", ("detector_properties/module0.yaml", "pixel_layouts/multi_tile_layout-2.3.16.yaml",
                 "simulation_properties/singles_sim.yaml")),
    ("2x2_no_modvar", ("detector_properties/2x2_no_modvar.yaml", "pixel_layouts/multi_tile_layout-2.4.16.yaml",
                       "simulation_properties/2x2_NuMI_sim_no_modvar.yaml")),
    ("ndlar", ("detector_properties/ndlar-module.yaml", "pixel_layouts/multi_tile_layout-3.0.40.yaml",
               "simulation_properties/NDLAr_LBNF_sim.yaml"))])
def test_yaml_loader_reproduces_reference_constants(cfg, files, ref):
    """Own YAML loader == snapshot written from the reference's loader (bit-identical floats)."""
    consts.load_properties(*(os.path.join(ref, f) for f in files))
    mine = json.loads(json.dumps(consts.snapshot_dict()))
    snap = json.load(open(os.path.join(REPO, "larnd-sim_amd", "larndsim_amd", "snapshots", cfg + ".json")))
    assert mine == snap


def test_snapshot_values_appendix_b():
    consts.load_snapshot("module0")
    d = consts.detector
    assert d.V_DRIFT == 0.1596452482154287 and d.N_PIXELS == (140, 280) and len(d.TIME_TICKS) == 2001
    assert d.TPC_BORDERS.shape == (2, 3, 2) and d.TIME_PADDING == 190 and d.TIME_WINDOW == 189.1
    consts.load_snapshot("ndlar")
    assert consts.detector.TPC_BORDERS.shape == (70, 3, 2) and consts.detector.RESPONSE_SAMPLING == 0.05
    assert consts.light.N_OP_CHANNEL == 0 and not consts.light.LIGHT_SIMULATED
    c = abi.pack_consts()
    assert c.n_tpc == 70 and c.n_time_ticks == 3201 and c.tpc_borders[69][2][0] == consts.detector.TPC_BORDERS[69][2][0]


def test_batching_matches_the_reference_batch_loop():
    consts.load_snapshot("2x2_no_modvar")
    seg = synth.make_segments(6000, seed=4, segs_per_event=1500, spill=True)
    # a few segments outside every TPC and one straddling two TPC groups
    seg["x_start"][:5] += 1000; seg["x_end"][:5] += 1000
    batching.swap_coordinates(seg)
    for tbs, bs in ((8, 10000), (2, 10000), (2, 400)):
        bid, order, table = batching.assign_batches(seg, tpc_batch_size=tbs, batch_size=bs)
        ref = np.full(len(seg), -1)
        k = 0
        for ev, mask in H.batch_sequence(seg, seg, "event_id", tbs, consts.detector.TPC_BORDERS):
            idx = np.flatnonzero(mask)
            for o in range(0, len(idx), bs):
                ref[idx[o:o + bs]] = k
                k += 1
        assert np.array_equal(ref, bid)
        assert len(table) == k and sum(t[3] for t in table) == (bid >= 0).sum()
        sb = bid[order]
        nsim = (bid >= 0).sum()
        assert (np.diff(sb[:nsim]) >= 0).all() and (sb[nsim:] == -1).all()


def test_shard_batches_balanced_and_contiguous():
    table = [(e, 0, 0, 5000 if e % 3 else 2000) for e in range(200)]
    for w in (1, 2, 4, 8):
        r = batching.shard_batches(table, w)
        assert (np.diff(r) >= 0).all() and r.max() == w - 1
        loads = np.bincount(r, weights=[t[3] for t in table], minlength=w)
        assert loads.max() / loads.mean() < 1.05


def test_chunk_ranges_cut_only_at_batch_boundaries():
    """One chain launch = whole batches: ranges tile [0, n), never split a batch, and reach the requested size."""
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 40, size=60)
    bid = np.repeat(np.arange(len(sizes)), sizes)
    for want in (1, 25, 100, 10_000):
        r = batching.chunk_ranges(bid, want)
        assert r[0][0] == 0 and r[-1][1] == len(bid)
        assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(e == len(bid) or bid[e] != bid[e - 1] for _, e in r)
        assert all(e - b >= want for b, e in r[:-1])
    assert batching.chunk_ranges(bid[:0], 10) == []


def test_load_pixel_table_reads_the_reference_format(tmp_path):
    """Pixel thresholds / gains files are what the reference's CudaDict.load reads (util/cuda_dict.py:82-88):
    an .npz with keys, values, default."""
    from larndsim_amd import fee
    f = tmp_path / "thr.npz"
    np.savez(f, keys=np.array([7, 3, 900001]), values=np.array([1.5e3, 2.5e3, 9.0]), default=np.array([4.2e3]))
    keys, values, default = fee.load_pixel_table(str(f))
    assert keys.dtype == np.int32 and values.dtype == np.float64
    assert keys.tolist() == [7, 3, 900001] and values.tolist() == [1.5e3, 2.5e3, 9.0] and default == 4.2e3
    np.savez(tmp_path / "dup.npz", keys=np.array([1, 1]), values=np.array([1.0, 2.0]), default=np.array([0.0]))
    with pytest.raises(ValueError, match="unique"):
        fee.load_pixel_table(str(tmp_path / "dup.npz"))
    np.savez(tmp_path / "len.npz", keys=np.array([1, 2]), values=np.array([1.0]), default=np.array([0.0]))
    with pytest.raises(ValueError, match="length"):
        fee.load_pixel_table(str(tmp_path / "len.npz"))


def test_oracle_rng_restatement_properties():
    """The oracle's restatement of numba.cuda.random (xoroshiro128p, SplitMix64 seeding, 2^64 jump, float32 Box-Muller):
    state 0 has both words equal to SplitMix64(seed); the jump is linear over GF(2) (jump(a ^ b) == jump(a) ^ jump(b));
    uniforms lie in [0, 1]; 2e5 normals have mean 0 and unit variance within 4 standard errors."""
    from oracle import oracle as O
    st = O.rng_create_states(4, 12345)
    z = (12345 + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    z ^= z >> 31
    assert int(st["s0"][0]) == int(st["s1"][0]) == z
    assert len({(int(a), int(b)) for a, b in zip(st["s0"], st["s1"])}) == 4
    a, b = O.rng_create_states(2, 1), O.rng_create_states(2, 2)
    x = np.zeros(2, dtype=O.RNG_DTYPE)
    x["s0"][0] = a["s0"][0] ^ b["s0"][0]; x["s1"][0] = a["s1"][0] ^ b["s1"][0]
    # one jump of the xor-ed state via the library: create_states jumps state 0 into state 1, reuse it through a manual copy
    lib = O.lib()
    import ctypes as C
    class R(C.Structure):
        _fields_ = [("s0", C.c_uint64), ("s1", C.c_uint64)]
    nxt = lib.o_rng_next
    nxt.restype = C.c_uint64
    r1 = R(int(a["s0"][0]), int(a["s1"][0])); r2 = R(int(b["s0"][0]), int(b["s1"][0])); r3 = R(int(x["s0"][0]), int(x["s1"][0]))
    for _ in range(50):      # the state update is linear: the xor of two streams' states is the state of the xor-ed seed state
        nxt(C.byref(r1)); nxt(C.byref(r2)); nxt(C.byref(r3))
        assert r3.s0 == r1.s0 ^ r2.s0 and r3.s1 == r1.s1 ^ r2.s1
    n = O.rng_normals(O.rng_create_states(1, 7), 0, 200_000).astype(np.float64)
    assert abs(n.mean()) < 4 / np.sqrt(len(n)) and abs(n.var() - 1) < 4 * np.sqrt(2 / len(n))
    assert np.isfinite(n).all() and np.abs(n).max() < 7


def test_synthetic_inputs_are_deterministic_and_in_schema():
    consts.load_snapshot("module0")
    a = synth.make_segments(3000, seed=20241016 + 2)
    b = synth.make_segments(3000, seed=20241016 + 2)
    assert a.dtype == layout.segments_dtype and a.tobytes() == b.tobytes()
    assert (a["dx"] >= 0.0099).all() and (a["dx"] <= 0.5001).all() and (a["dEdx"] >= 1).all()
    r = synth.make_response("survey")
    assert r.shape == (45, 45, 1950) and abs(r[0, 0].sum() * 0.1 - 1) < 1e-12
    assert (r[0, 0, :1600] == 0).all() and (synth.make_response("dense") != 0).all()
    lut = synth.make_lut()
    assert lut.shape == (14, 26, 8, 48) and np.allclose(lut["time_dist"].sum(-1), 1, atol=1e-5)


def test_cli_input_checks_like_the_reference(tmp_path):
    """cli/simulate_pixels.py:264-267 of the reference: missing input / existing output raise before any work."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sp_cli", os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(Exception, match="does not exist"):
        cli.run_simulation(str(tmp_path / "nope.npy"), str(tmp_path / "out.npz"))
    seg = synth.make_segments(10, seed=1, segs_per_event=10)
    np.save(tmp_path / "in.npy", seg)
    (tmp_path / "out.npz").write_bytes(b"x")
    with pytest.raises(Exception, match="already exists"):
        cli.run_simulation(str(tmp_path / "in.npy"), str(tmp_path / "out.npz"))
    with pytest.raises(KeyError):
        cli.run_simulation(str(tmp_path / "in.npy"), str(tmp_path / "out2.npz"), config="2x2_mod2mod_variation")
    # prepare_tracks: adds the columns the reference adds and swaps x<->z
    consts.load_snapshot("module0")
    old = np.zeros(3, dtype=[(n, layout.segments_dtype.fields[n][0]) for n in layout.segments_dtype.names
                             if n not in ("t0", "t0_start", "t0_end", "n_photons", "segment_id")])
    old["t"] = [1, 2, 3]; old["x"] = 5; old["z"] = 7
    new = cli.prepare_tracks(old)
    for f in ("t0", "t0_start", "t0_end", "n_photons", "segment_id"):
        assert f in new.dtype.names
    assert np.array_equal(new["t0"], [1, 2, 3]) and (new["t"] == 0).all() and (new["x"] == 7).all() and (new["z"] == 5).all()


def _load_cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sp_cli", os.path.join(REPO, "larnd-sim_amd", "cli", "simulate_pixels.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_event_times_into_truth_datasets():
    """cli/simulate_pixels.py:614-642: t_event is put in front of `vertices` (non-spill simulations: one time per distinct
    event id, repeated over the event's rows) and copied into `mc_hdr`; spill simulations leave `vertices` alone; a length
    mismatch is the reference's ValueError."""
    cli = _load_cli()
    H.load_cfg("module0")
    assert not consts.sim.IS_SPILL_SIM
    vt = np.zeros(5, dtype=[("event_id", "u4"), ("vertex_id", "u8"), ("x_vert", "f4")])
    vt["event_id"] = [0, 0, 2, 3, 3]
    vt["x_vert"] = np.arange(5)
    hdr = np.zeros(5, dtype=[("event_id", "u4"), ("reaction", "i4")])
    hdr["event_id"], hdr["reaction"] = vt["event_id"], np.arange(5) + 10
    times = np.array([1.5, 20.0, 300.0, 4000.0])
    truth = {"vertices": vt.copy(), "mc_hdr": hdr.copy(), "trajectories": np.zeros(2, dtype=[("event_id", "u4")])}
    cli.attach_event_times(truth, times, consts.sim)
    assert truth["vertices"].dtype.names[0] == "t_event" and truth["vertices"].dtype["t_event"] == np.float32
    assert np.array_equal(truth["vertices"]["t_event"], np.float32([1.5, 1.5, 300.0, 4000.0, 4000.0]))
    assert np.array_equal(truth["vertices"]["x_vert"], vt["x_vert"]) and np.array_equal(truth["vertices"]["vertex_id"], vt["vertex_id"])
    assert np.array_equal(truth["mc_hdr"]["t_event"], truth["vertices"]["t_event"]) and np.array_equal(truth["mc_hdr"]["reaction"], hdr["reaction"])
    assert truth["trajectories"].dtype.names == ("event_id",)
    with pytest.raises(ValueError, match="different number of vertices"):
        cli.attach_event_times({"vertices": vt.copy(), "mc_hdr": hdr[:3].copy()}, times, consts.sim)
    H.load_cfg("2x2_no_modvar")
    assert consts.sim.IS_SPILL_SIM
    truth = {"vertices": vt.copy(), "mc_hdr": hdr.copy()}
    cli.attach_event_times(truth, times, consts.sim)
    assert "t_event" not in truth["vertices"].dtype.names and "t_event" not in truth["mc_hdr"].dtype.names


def _random_packet_inputs(rng, n_pix, n_ev, spill):
    """Per-pixel ADC arrays as the chain hands them to the packet writer, shaped to reach every branch of the hit loop: slots
    that stop at the pedestal, several hits per pixel, pixels off the readout map, events past the 1 s clock reset, equal
    tick stamps in a row, trajectories with up to 12 segments on one pixel (numpy's pairwise summation starts at 9 terms)."""
    from larndsim_amd import packets
    d, sim = consts.detector, consts.sim
    A, M = sim.MAX_ADC_VALUES, sim.MAX_TRACKS_PER_PIXEL
    ped = packets._digitize0()
    n_tot = int(d.N_PIXELS[0]) * int(d.N_PIXELS[1]) * d.TPC_BORDERS.shape[0]
    upix = np.sort(rng.choice(n_tot, n_pix, replace=False)).astype(np.int64)
    ev_of_pix = np.sort(rng.integers(0, n_ev, n_pix))
    adc = np.full((n_pix, A), ped, dtype=np.float64)
    ticks = np.zeros((n_pix, A))
    nh = rng.choice([0, 1, 1, 1, 2, 3, A], n_pix)
    for u in range(n_pix):
        adc[u, :nh[u]] = rng.integers(int(ped) + 1, 255, nh[u])
        ticks[u, :nh[u]] = np.sort(rng.choice([12.3, 40.0, 40.0, 77.7, 150.2, 199.9], nh[u])) if rng.random() < 0.3 \
            else np.sort(rng.uniform(0, 200, nh[u]))
        if nh[u] > 1 and rng.random() < 0.1:
            adc[u, 1] = ped            # the loop stops here although a later slot is above the pedestal
    event_id_list = np.repeat(ev_of_pix[:, None], A, axis=1)
    frac = np.zeros((n_pix, A, M))
    seg_ids = np.full((n_pix, M), -1, dtype=np.int64)
    traj_ids = np.full((n_pix, M), -1, dtype=np.int64)
    for u in range(n_pix):
        k = int(rng.integers(1, min(M, 14) + 1))
        seg_ids[u, :k] = rng.choice(10_000, k, replace=False)
        traj_ids[u, :k] = rng.choice([3, 3, 3, 3, 8, 11, 40], k) if rng.random() < 0.5 else 5
        frac[u, :, :k] = rng.dirichlet(np.ones(k), A) * rng.choice([1.0, 1.0, 0.5], (A, 1))
    t0 = np.sort(rng.uniform(0, 50, n_ev)) + (np.arange(n_ev) * 1.2e6 / 3 if spill else 0)
    return dict(event_id_list=event_id_list, adc_list=adc, adc_ticks_list=ticks, unique_pix=upix, current_fractions=frac,
                track_ids=seg_ids, traj_ids=traj_ids, event_start_times=t0)


def test_packets_unequal_slot_widths_are_refused():
    """track_ids / traj_ids / current_fractions whose slot count is not MAX_TRACKS_PER_PIXEL: the reference's np.array over
    the per-packet lists is ragged (fee.py:271-276,297-300) and raises ValueError; so do build_packets and the loop checker."""
    from larndsim_amd import packets
    from packets_loop import build_packets_loop
    H.load_cfg("module0", noise_zero=False)
    rng = np.random.default_rng(5)
    inp = _random_packet_inputs(rng, 60, 3, False)
    w = 7
    for bad in (dict(inp, traj_ids=inp["traj_ids"][:, :-1]),
                dict(inp, track_ids=inp["track_ids"][:, :w], traj_ids=inp["traj_ids"][:, :w],
                     current_fractions=np.ascontiguousarray(inp["current_fractions"][:, :, :w]))):
        with pytest.raises(ValueError):
            packets.build_packets(**bad)
        with pytest.raises(ValueError):
            build_packets_loop(**bad)


@pytest.mark.parametrize("cfg,spill", [("module0", False), ("module0", True), ("2x2_no_modvar", True)])
def test_packets_array_form_equals_the_hit_loop(cfg, spill):
    """packets.build_packets (array operations; what the driver calls) against tests/packets_loop.py (the reference's
    loop restated hit by hit, pinned by the goldens): the same bytes, on the golden inputs and on random ones that walk every
    branch -- clock rollovers (events up to 4 s apart), pixels without a chip, a disabled channel, light triggers, module
    selection, trajectory sums of 9 and more terms."""
    from larndsim_amd import packets
    from packets_loop import build_packets_loop
    H.load_cfg(cfg, noise_zero=False)
    g = H.gold(f"packets_{cfg}.npz")
    n_ev = len(g["event_times"])
    bad = {str(g["bad_key"]): [int(g["bad_channel"])]} if str(g["bad_key"]) else None
    args = (g["event_id_list"], g["adc"], g["ticks"], g["unique_pix"], g["fractions"], g["segment_ids"], g["traj_ids"], g["event_times"])
    kw = dict(light_trigger_times=g["trig_times"], light_trigger_event_id=np.arange(n_ev), light_trigger_modules=np.ones(n_ev),
              bad_channels=bad)
    a, b = packets.build_packets(*args, **kw), build_packets_loop(*args, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) > 40
    rng = np.random.default_rng(77)
    n_big = 0
    for trial in range(6):
        inp = _random_packet_inputs(rng, 400, 12, spill)
        kw = {}
        if trial % 2 == 0:
            kw = dict(light_trigger_times=rng.uniform(0, 5, 12), light_trigger_event_id=rng.integers(0, 12, 12),
                      light_trigger_modules=np.ones(12))
        if trial % 3 == 1:
            kw["i_mod"] = 1
        a = packets.build_packets(**inp, **kw)
        if trial == 2 and len(a[0]):           # disable a channel that carries data
            first = a[0][a[0]["packet_type"] == 0][0]
            kw["bad_channels"] = {"%i-%i-%i" % (first["io_group"], first["io_channel"], first["chip_id"]): [int(first["channel_id"])]}
            a = packets.build_packets(**inp, **kw)
        b = build_packets_loop(**inp, **kw)
        assert len(a[0]) == len(b[0]) > 300, trial
        for name in a[0].dtype.names:
            assert np.array_equal(a[0][name], b[0][name]), (trial, name)
        for name in a[1].dtype.names:
            assert a[1][name].tobytes() == b[1][name].tobytes(), (trial, name)
        t = inp["traj_ids"]
        n_big += int(((t == 3).sum(axis=1) >= 9).sum() + ((t == 5).sum(axis=1) >= 9).sum())
        if spill:
            assert (inp["event_start_times"] / consts.detector.CLOCK_CYCLE > consts.detector.CLOCK_RESET_PERIOD).any()
    assert n_big > 0          # the pairwise-summation branch was reached


def _dense_to_compact_rows(event_id_list, adc_list, adc_ticks_list, unique_pix, current_fractions, track_ids, traj_ids):
    """the arguments of packets.build_packets_compact from the dense per-pixel arrays build_packets takes: every row, its hits = the
    slots the chain's scan wrote (here: up to the last slot above 0 -- the exporter's own stop rule is the builder's job), its filled
    track slots, the fractions of those slots"""
    U, A = adc_list.shape
    nh = np.where((adc_list != 0).any(axis=1), A - np.argmax((adc_list != 0)[:, ::-1], axis=1), 0).astype(np.int64)
    filled = track_ids != -1
    nt = filled.sum(axis=1).astype(np.int64)
    assert all((filled[u, :nt[u]]).all() for u in range(U)), "track slots fill from slot 0"
    hit_row = np.repeat(np.arange(U), nh)
    hit_slot = np.arange(int(nh.sum())) - np.repeat(np.cumsum(nh) - nh, nh)
    frac = [current_fractions[u, s, :nt[u]] for u, s in zip(hit_row, hit_slot)]
    return dict(row_event=event_id_list[:, 0], row_pixel=unique_pix, row_nh=nh, row_nt=nt,
                hit_adc=adc_list[hit_row, hit_slot].astype(np.int32), hit_tick=adc_ticks_list[hit_row, hit_slot],
                hit_frac=np.concatenate(frac) if frac else np.zeros(0),
                trk_segment=track_ids[filled], trk_traj=traj_ids[filled])


@pytest.mark.parametrize("cfg,spill", [("module0", False), ("module0", True), ("2x2_no_modvar", True)])
def test_native_packet_builder_equals_build_packets(cfg, spill):
    """ldsim_packets_build (csrc/packets.hip: the reference's hit loop in C on the chain's compact rows -- hits, filled track slots
    and per-hit fractions, no dense [pixel][30][50] array) against packets.build_packets on the dense form of the same rows: the
    same bytes, on the golden inputs (pinned to fee.export_to_hdf5) and on random ones that walk every branch -- clock rollovers,
    pixels without a chip, a disabled channel, light triggers, module selection, hit-less rows in front."""
    from larndsim_amd import packets
    H.load_cfg(cfg, noise_zero=False)
    g = H.gold(f"packets_{cfg}.npz")
    n_ev = len(g["event_times"])
    bad = {str(g["bad_key"]): [int(g["bad_channel"])]} if str(g["bad_key"]) else None
    args = (g["event_id_list"], g["adc"], g["ticks"], g["unique_pix"], g["fractions"], g["segment_ids"], g["traj_ids"])
    kw = dict(light_trigger_times=g["trig_times"], light_trigger_event_id=np.arange(n_ev), light_trigger_modules=np.ones(n_ev),
              bad_channels=bad)
    a = packets.build_packets(*args, g["event_times"], **kw)
    b = packets.build_packets_compact(**_dense_to_compact_rows(*args), event_start_times=g["event_times"], **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) > 40
    rng = np.random.default_rng(78)
    for trial in range(6):
        inp = _random_packet_inputs(rng, 400, 12, spill)
        if trial >= 3:                       # the export starts with rows that hold no hit (the exporter's row 0 all the same)
            inp["adc_list"][:3] = 0
        if trial >= 4:                       # negative and exactly-zero fractions in filled slots: the unused slots (0) sort between
            inp["current_fractions"][:, :, 0] *= -1.0
            inp["current_fractions"][:, :, 1] = 0.0
        kw = {}
        if trial % 2 == 0:
            kw = dict(light_trigger_times=rng.uniform(0, 5, 12), light_trigger_event_id=rng.integers(0, 12, 12),
                      light_trigger_modules=np.ones(12))
        if trial % 3 == 1:
            kw["i_mod"] = 1
        a = packets.build_packets(**inp, **kw)
        if trial == 2 and len(a[0]):
            first = a[0][a[0]["packet_type"] == 0][0]
            kw["bad_channels"] = {"%i-%i-%i" % (first["io_group"], first["io_channel"], first["chip_id"]): [int(first["channel_id"])]}
            a = packets.build_packets(**inp, **kw)
        est = inp.pop("event_start_times")
        b = packets.build_packets_compact(**_dense_to_compact_rows(**inp), event_start_times=est, **kw)
        assert len(a[0]) == len(b[0]) > 300, trial
        for name in a[0].dtype.names:
            assert np.array_equal(a[0][name], b[0][name]), (trial, name)
        for name in a[1].dtype.names:
            assert a[1][name].tobytes() == b[1][name].tobytes(), (trial, name)


@pytest.mark.parametrize("cfg", ["module0", "2x2_no_modvar"])
def test_packets_writer_golden(cfg):
    """packets.build_packets (larpix-control-free writer of the `packets` / `mc_packets_assn` datasets) against
    fee.export_to_hdf5 of the reference run under attribute-bag packet classes (oracle/gen_golden.py gen_packets): every
    packet in order with its io_group / io_channel / chip / channel / timestamp / dataword, the inserted timestamp, sync
    and trigger packets (module0: threshold trigger mode; 2x2: beam mode inserts none), rollover of the third event, a
    disabled channel, and the association rows."""
    from larndsim_amd import packets
    H.load_cfg(cfg, noise_zero=False)
    g = H.gold(f"packets_{cfg}.npz")
    bad = {str(g["bad_key"]): [int(g["bad_channel"])]} if str(g["bad_key"]) else None
    n_ev = len(g["event_times"])
    pk, assn = packets.build_packets(g["event_id_list"], g["adc"], g["ticks"], g["unique_pix"], g["fractions"],
                                     g["segment_ids"], g["traj_ids"], g["event_times"], light_trigger_times=g["trig_times"],
                                     light_trigger_event_id=np.arange(n_ev), light_trigger_modules=np.ones(n_ev),
                                     bad_channels=bad)
    rows = g["rows"]
    assert len(pk) == len(rows) and (rows["kind"] == 0).sum() > 40
    assert np.array_equal(pk["packet_type"], rows["kind"])
    assert np.array_equal(pk["io_group"], rows["io_group"])
    data = rows["kind"] == 0
    for f in ("io_channel", "chip_id", "channel_id", "dataword", "first_packet", "receipt_timestamp"):
        assert np.array_equal(pk[f][data].astype(np.int64), rows[f][data]), f
    assert np.array_equal(pk["timestamp"], rows["timestamp"].astype(np.uint64))        # floats truncate like the u8 dataset does
    sync_trig = (rows["kind"] == 6) | (rows["kind"] == 7)
    assert np.array_equal(pk["trigger_type"][sync_trig].astype(np.int64), rows["trigger_type"][sync_trig])
    if bad:
        k = tuple(int(x) for x in str(g["bad_key"]).split("-"))
        hit = (pk["io_group"] == k[0]) & (pk["io_channel"] == k[1]) & (pk["chip_id"] == k[2]) & \
              (pk["channel_id"] == int(g["bad_channel"])) & (pk["packet_type"] == 0)
        assert not hit.any()
    # data packets carry odd parity over their 64 bits
    w = (pk["chip_id"].astype(np.uint64) << 2) | (pk["channel_id"].astype(np.uint64) << 10) | \
        ((pk["timestamp"] & 0x7FFFFFFF) << 16) | (pk["first_packet"].astype(np.uint64) << 47) | \
        (pk["dataword"].astype(np.uint64) << 48) | (pk["parity"].astype(np.uint64) << 63)
    ones = np.array([bin(int(x)).count("1") for x in w[data]])
    assert (ones % 2 == 1).all()
    assert np.array_equal(assn["event_ids"], g["assn_event_ids"])
    assert np.array_equal(assn["segment_ids"], g["assn_segment_ids"])
    assert np.array_equal(assn["fraction"], g["assn_fraction"])
    assert np.array_equal(assn["file_traj_ids"], g["assn_file_traj_ids"])
    assert np.array_equal(assn["fraction_traj"], g["assn_fraction_traj"])
    assert packets.packets_dtype.itemsize == 36 and assn.dtype == packets.assn_dtype()
    # the driver's packets between events: fee.export_sync_to_hdf5 / export_timestamp_trigger_to_hdf5 (fee.py:361-497), for
    # all io groups and for one module's
    for i_mod in (-1, 1):
        for name, (pk2, as2) in (("sync", packets.build_sync_packets(g["sync_times"], i_mod)),
                                 ("tt", packets.build_timestamp_trigger_packets(g["event_times"], i_mod))):
            ref = g[f"{name}_rows_{i_mod}"]
            assert len(pk2) == len(ref) == len(as2) and len(ref) > 0
            assert np.array_equal(pk2["packet_type"], ref["kind"]) and np.array_equal(pk2["io_group"], ref["io_group"])
            assert np.array_equal(pk2["timestamp"], ref["timestamp"].astype(np.uint64))
            st = (ref["kind"] == 6) | (ref["kind"] == 7)
            assert np.array_equal(pk2["trigger_type"][st].astype(np.int64), ref["trigger_type"][st])
            assert (as2["event_ids"] == -1).all() and (as2["segment_ids"] == -1).all() and (as2["fraction"] == 0).all()


def test_config_keyword_resolution(ref):
    """config.get_config follows larndsim/config/config.py:40-69: bare names joined to their family's directory, names with
    '/' kept, lists element by element, other keys passed through; the module-variation decision and the per-module file
    lists follow cli/simulate_pixels.py:106-122, 355-372."""
    from larndsim_amd import config
    assert set(config.list_config_keys()) == {"module0", "2x2", "2x2_no_modvar", "ndlar"}   # built-in snapshots
    assert config.get_config("ndlar")["SNAPSHOT"] == "ndlar"
    with pytest.raises(KeyError, match="not in supported keywords"):
        config.get_config("2x2_mpvmpr")
    b = config.get_config("2x2")
    assert b["MOD2MOD_VARIATION"] is True and len(b["SNAPSHOT"]) == 4
    assert config.module_variation_active(b, 4, None, b["PIXEL_LAYOUT"], b["RESPONSE"], None)
    assert not config.module_variation_active(b, 1, None, b["PIXEL_LAYOUT"], b["RESPONSE"], None)      # one module
    assert not config.module_variation_active(b, 4, None, "a.yaml", ["r.npy"], "lut.npz")             # a single set of files
    assert not config.module_variation_active(b, 4, False, b["PIXEL_LAYOUT"], b["RESPONSE"], None)     # switched off by the flag
    assert config.module_files(b, b["PIXEL_LAYOUT"], "PIXEL_LAYOUT_ID", 4) == [b["PIXEL_LAYOUT"][i] for i in (0, 0, 1, 0)]
    assert config.module_files(b, ["a", "b", "c", "d"], "NO_SUCH_ID", 4) == ["a", "b", "c", "d"]
    with pytest.raises(KeyError, match="number of response files is incorrect"):
        config.module_files(b, ["a", "b", "c"], "NO_SUCH_ID", 4, "response files")
    assert config.single_file(["x"]) == "x" and config.single_file("x") == "x"
    with pytest.raises(KeyError, match="more than one"):
        config.single_file(["x", "y"], "response file")
    keys = set(config.list_config_keys(ref))
    assert {"module0", "2x2", "2x2_no_modvar", "2x2_mpvmpr", "ndlar"} <= keys
    c = config.get_config("2x2_no_modvar", ref)
    assert c["DET_PROPERTIES"] == os.path.join(ref, "detector_properties", "2x2_no_modvar.yaml")
    assert c["PIXEL_LAYOUT"] == os.path.join(ref, "pixel_layouts", "multi_tile_layout-2.4.16.yaml")
    assert c["RESPONSE"] == os.path.join(ref, "bin", "response_44.npy")
    assert c["LIGHT_LUT"].startswith("/global/cfs/")                   # has a '/': kept as written
    assert c["MOD2MOD_VARIATION"] is False and c["LIGHT_SIMULATED"] is True
    m = config.get_config("2x2", ref)
    assert m["PIXEL_LAYOUT"] == [os.path.join(ref, "pixel_layouts", f) for f in
                                 ("multi_tile_layout-2.4.16.yaml", "multi_tile_layout-2.5.16.yaml")]
    assert m["PIXEL_LAYOUT_ID"] == [0, 0, 1, 0] and m["MOD2MOD_VARIATION"] is True
    # per-module loading through the package's own YAML loader == the per-module snapshots written from the reference's
    layouts = config.module_files(m, m["PIXEL_LAYOUT"], "PIXEL_LAYOUT_ID", 4)
    assert consts.get_n_modules(m["DET_PROPERTIES"]) == [1, 2, 3, 4]
    for i_mod in (1, 2, 3, 4):
        consts.load_properties(m["DET_PROPERTIES"], layouts, m["SIM_PROPERTIES"], i_module=i_mod)
        mine = json.loads(json.dumps(consts.snapshot_dict()))
        snap = json.load(open(os.path.join(REPO, "larnd-sim_amd", "larndsim_amd", "snapshots", f"2x2_mod{i_mod}.json")))
        assert mine == snap, i_mod
    assert consts.detector.RESPONSE_SAMPLING == 0.05 and consts.sim.MAX_MC_TRUTH_IDS == 50
    with pytest.raises(KeyError):
        config.get_config("2x2_mod2mod_variation", ref)               # the reference CLI's default keyword is not in its own map
    # the resolved files load through the package's own YAML loader
    consts.load_properties(c["DET_PROPERTIES"], c["PIXEL_LAYOUT"], c["SIM_PROPERTIES"])
    assert consts.detector.TPC_BORDERS.shape == (8, 3, 2) and len(consts.detector.PIXEL_CONNECTION_DICT) == 4900


@pytest.mark.parametrize("cfg", ["module0", "2x2_no_modvar"])
def test_light_output_datasets_golden(cfg):
    """light_trig rows, light_wvfm and light_wvfm_mc_assn rows against what the reference's exporters (light_sim.py:621-757)
    left in an in-memory h5py sink after their appending calls (oracle/gen_golden.py gen_light_export)."""
    import helpers as H
    from larndsim_amd import consts, light_sim
    H.load_cfg(cfg)
    consts.sim.MAX_MC_TRUTH_IDS = 3
    g = H.gold(f"light_export_{cfg}.npz")
    assert int(g["light_trig_mode"]) == consts.light.LIGHT_TRIG_MODE
    trig, wv, assn = [], [], []
    for i in range(2):
        c = {k: g[f"call{i}_{k}"] for k in ("event_id", "start_times", "trigger_idx", "op_channel_idx", "waveforms",
                                              "true_track_id", "true_photons", "event_times", "i_trig")}
        if consts.light.LIGHT_TRIG_MODE == 0:
            trig.append(light_sim.build_light_trig(c["event_id"], c["start_times"], c["trigger_idx"], c["op_channel_idx"],
                                                   c["event_times"]))
        wv.append(c["waveforms"])
        assn.append(light_sim.zero_suppress_waveform_truth(c["true_track_id"].astype('i8'), c["true_photons"],
                                                           c["event_id"][0], int(c["i_trig"]), -1))
    if consts.light.LIGHT_TRIG_MODE == 1:
        lev = g["trig1_event_id"]
        trig.append(light_sim.build_light_trig(lev, np.full(3, 0), np.full(3, 0), consts.light.TPC_TO_OP_CHANNEL[:].ravel(),
                                               g["trig1_event_times"]))
    trig = np.concatenate(trig); assn = np.concatenate(assn)
    assert trig.dtype["op_channel"].shape == g["light_trig_op_channel"].shape[1:]
    assert np.array_equal(trig["op_channel"], g["light_trig_op_channel"])
    assert np.array_equal(trig["ts_s"], g["light_trig_ts_s"]) and np.array_equal(trig["ts_sync"], g["light_trig_ts_sync"])
    assert trig["ts_sync"].dtype == np.uint64
    assert np.array_equal(np.concatenate(wv), g["light_wvfm"])
    assert str(assn.dtype.descr) == str(g["assn_dtype"])
    for f in assn.dtype.names:
        assert np.array_equal(assn[f], g["assn_" + f]), f
    assert len(assn) > 100 and len(np.unique(assn["trigger_id"])) > 2


def test_sum_light_wrapper_keeps_its_arguments_only_for_the_same_channel_array(monkeypatch):
    """ChargeChain.sum_light without truth slots (trigger mode 1) keeps the channel array's pointer and the fixed arguments of the
    library call between batches.  No GPU: the library call is replaced by a recorder.  The same array object re-uses them (changes
    of its contents are the library's business: it compares against its copy); another object, another tick cap or another light
    window refreshes them; an array that had to be converted is never kept; truth slots take the general path."""
    from larndsim_amd import chain
    H.load_cfg("ndlar")
    synth.set_synthetic_light(48)
    calls = []

    class FakeLib:
        def ldsim_dev_sum_light(self, ctx, b, e, opc, n_det, tid, mt, t_start, n_ticks):
            calls.append((b.value, e.value, C.cast(opc, C.c_void_p).value, n_det.value, tid is None or not bool(tid), mt.value,
                          t_start.value, n_ticks.value))
            return 0

    fake = FakeLib()
    monkeypatch.setattr(lib, "load", lambda: fake)
    monkeypatch.setattr(lib, "consts_generation", lambda: 7)
    ch = chain.ChargeChain.__new__(chain.ChargeChain)
    ch.ctx, ch._generation, ch.n = None, 7, 0
    opc = consts.light.TPC_TO_OP_CHANNEL[:].ravel().astype(np.int32)
    n_ticks_full = int((consts.light.LIGHT_WINDOW[1] + consts.light.LIGHT_WINDOW[0]) / consts.light.LIGHT_TICK_SIZE)
    assert consts.sim.MAX_MC_TRUTH_IDS == 0 and consts.light.LIGHT_TRIG_MODE != 0
    assert ch.sum_light(0, 200, opc) == (n_ticks_full, 0)
    first = ch._sum_light_fast
    assert ch.sum_light(200, 450, opc) == (n_ticks_full, 0) and ch._sum_light_fast is first
    assert calls[0][2] == calls[1][2] == opc.ctypes.data and calls[1][:2] == (200, 450) and calls[1][3] == len(opc)
    assert ch._light_shape == (len(opc), n_ticks_full, 0) and lib.context_light_shape() == ch._light_shape
    # another array object (same contents), another tick cap: refreshed
    opc2 = opc.copy()
    ch.sum_light(0, 10, opc2)
    assert ch._sum_light_fast is not first and calls[-1][2] == opc2.ctypes.data
    second = ch._sum_light_fast
    assert ch.sum_light(0, 10, opc2, max_ticks=5000) == (5000, 0) and ch._sum_light_fast is not second and calls[-1][7] == 5000
    # an int64 list is converted for the call and not kept
    kept = ch._sum_light_fast
    ch.sum_light(0, 10, opc.astype(np.int64))
    assert ch._sum_light_fast is kept and calls[-1][3] == len(opc)
    # a changed light window changes the tick count of the next call
    w = consts.light.LIGHT_WINDOW
    try:
        consts.light.LIGHT_WINDOW = (w[0], w[1] + 1)
        n2, _ = ch.sum_light(0, 10, opc2, max_ticks=int(5e4))
        assert n2 == n_ticks_full + int(1 / consts.light.LIGHT_TICK_SIZE) and calls[-1][7] == n2
    finally:
        consts.light.LIGHT_WINDOW = w
    # truth slots: the general path (ids made for the range)
    n_before = len(calls)
    ch.sum_light(5, 9, opc2, max_truth=3)
    assert len(calls) == n_before + 1 and calls[-1][5] == 3 and calls[-1][4] is False


def test_expand_compact_lead_rows_equal_padding_each_batch():
    """chain.expand_compact(lead_rows=True) hands the exporter, for a batch whose first unique pixel holds no hit, that hit-less row in
    front of the batch's hit pixels: the same rows as expanding without it and padding every batch's slices afterwards (what the
    driver did before, copying the fraction array once more); the default form is unchanged."""
    from larndsim_amd import chain, packets
    H.load_cfg("module0")
    A = consts.sim.MAX_ADC_VALUES
    rng = np.random.default_rng(1)
    n = 60
    batch = np.sort(rng.integers(0, 8, n))
    nh, nt = rng.integers(1, min(4, A) + 1, n), rng.integers(1, 5, n)
    starts = np.r_[True, batch[1:] != batch[:-1]]
    first = np.zeros(n, bool)
    first[starts] = rng.random(int(starts.sum())) < 0.5
    assert first.any() and (~first[starts]).any()
    hp = np.zeros((n, 5), np.int64)
    hp[:, 0], hp[:, 1], hp[:, 2], hp[:, 3], hp[:, 4] = np.arange(n) * 3, rng.integers(0, 1000, n), batch, nh, nt | (first.astype(int) << 8)
    n_hits = int(nh.sum())
    hit_rows = np.zeros(n_hits, dtype=[('slot', 'i4'), ('tick', 'f8'), ('adc', 'f8')])
    hit_rows['slot'] = np.concatenate([np.arange(k) for k in nh])
    hit_rows['tick'], hit_rows['adc'] = rng.random(n_hits) * 100, rng.integers(70, 200, n_hits)
    c = dict(hit_pixels=hp, hit_rows=hit_rows, hit_charge=rng.random(n_hits) * 1e4, track_segments=rng.integers(0, 500, int(nt.sum())),
             has_fractions=True, fractions=rng.random(int(np.repeat(nt, nh).sum())))
    old, new = chain.expand_compact(c), chain.expand_compact(c, lead_rows=True)
    assert np.array_equal(old["row"], hp[:, 0]) and np.array_equal(old["first_of_batch"], first)
    ped = packets._digitize0()
    fill = dict(track_pixel_map=-1, adc_digit=ped, adc_ticks_list=0, current_fractions=0, adc_list=0)
    for k in ("track_pixel_map", "adc_digit", "adc_ticks_list", "current_fractions", "adc_list", "unique_pix", "batch"):
        blocks = []
        for bb in np.unique(batch):
            blk = old[k][old["batch"] == bb]
            if not old["first_of_batch"][old["batch"] == bb][0]:
                v = fill.get(k, blk[0])
                blk = np.concatenate([np.full((1,) + blk.shape[1:], v, dtype=blk.dtype), blk])
            blocks.append(blk)
        ref = np.concatenate(blocks)
        assert ref.shape == new[k].shape and np.array_equal(ref, new[k]), k
    assert len(new["batch"]) == n + int((starts & ~first).sum())
    assert new["first_of_batch"][np.r_[True, new["batch"][1:] != new["batch"][:-1]]].all()
    assert (new["row"][new["row"] >= 0] == hp[:, 0]).all() and (new["row"] == -1).sum() == len(new["batch"]) - n


def test_a_second_thread_cannot_claim_the_process_ctx_while_a_chain_lives():
    """lib.claim_chain (what ChargeChain.__init__ calls first): the process-wide ctx serves one thread at a time.  A chain object
    made on another thread while the first thread's chain is alive is refused; after the first is dropped, or its thread has ended,
    the claim passes (VERDICT r03 item 5 -- the C-level guard, LDSIM_ESTATE on concurrent entry, has its test on the GPU)."""
    import gc
    import threading
    from larndsim_amd import lib

    class Chain:
        pass
    lib._chain_owner = None
    a = Chain()
    lib.claim_chain(a)
    lib.claim_chain(Chain())                  # same thread: chains follow each other as before
    lib.claim_chain(a)
    seen = []

    def other(expect_refusal):
        try:
            lib.claim_chain(Chain())
            seen.append("claimed")
        except lib.LdsimError as e:
            seen.append(str(e))
        assert ("still alive" in seen[-1]) == expect_refusal

    t = threading.Thread(target=other, args=(True,)); t.start(); t.join()
    assert "still alive" in seen[-1]
    del a
    gc.collect()
    t = threading.Thread(target=other, args=(False,)); t.start(); t.join()
    assert seen[-1] == "claimed"
    # the thread that claimed last has ended: its claim does not outlive it
    lib.claim_chain(Chain())
    lib._chain_owner = None


def test_crc32_parts_equals_zlib():
    """ldsim_crc32_parts (csrc/crc32.hip: slicing-by-8 per 4 MiB piece on host threads, pieces joined with the GF(2) zero-append
    operator) against zlib.crc32 over ragged part lists, on 1, 3 and all threads."""
    import zlib
    from larndsim_amd import lib
    rng = np.random.default_rng(11)
    for sizes in ([], [0], [1], [7, 0, 9], [5, 4 << 20, (4 << 20) + 3, 123457], [(9 << 20) + 1]):
        parts = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
        ref = zlib.crc32(b"".join(p.tobytes() for p in parts))
        for nt in (1, 3, 0):
            assert lib.crc32_parts(parts, nt) == ref, (sizes, nt)
    assert lib.crc32_parts([b"123456789"]) == 0xCBF43926          # the check value of CRC-32/ISO-HDLC


@pytest.mark.parametrize("zip64_at", [None, 64])
def test_npz_stream_reads_back_like_savez(tmp_path, monkeypatch, zip64_at):
    """The driver's output writer (larndsim_amd/npz_stream.py): members written from ragged pieces read back through numpy.load
    as the joined arrays, zipfile's own CRC check passes, and with the ZIP64 threshold lowered every ZIP64 record is exercised."""
    import zipfile
    from larndsim_amd import npz_stream
    from larndsim_amd.packets import packets_dtype
    if zip64_at is not None:
        monkeypatch.setattr(npz_stream, "_ZIP64_AT", zip64_at)
    rng = np.random.default_rng(0)
    fn = str(tmp_path / "a.npz")
    pk = [np.frombuffer(rng.bytes(36 * n), dtype=packets_dtype) for n in (5, 0, 17)]
    al = np.zeros(7, dtype=np.dtype([("a", "u1"), ("b", "f8"), ("c", "i4", (3,))], align=True))
    al["b"] = rng.random(7)
    wv = [rng.random((3, 4, 5)), rng.random((0, 4, 5)), rng.random((2, 4, 5))]
    with npz_stream.NpzStream(fn) as z:
        z.write("packets", pk)
        z.write("light_wvfm/light_wvfm_mod0", wv)
        z.write("scalar", [np.float64(3.5)])
        z.write("al", [al, al[:0], al[::2]])
        z.write("empty", [np.zeros((0, 3), dtype="i2")])
        with pytest.raises(ValueError, match="differ"):
            z.write("bad", [np.zeros(3), np.zeros(3, dtype="f4")])
    assert zipfile.ZipFile(fn).testzip() is None
    with np.load(fn) as f:
        assert f.files == ["packets", "light_wvfm/light_wvfm_mod0", "scalar", "al", "empty"]
        assert np.array_equal(f["packets"], np.concatenate(pk)) and f["packets"].dtype == packets_dtype
        assert np.array_equal(f["light_wvfm/light_wvfm_mod0"], np.concatenate(wv))
        assert f["scalar"] == 3.5 and f["scalar"].shape == ()
        assert np.array_equal(f["al"], np.concatenate([al, al[::2]])) and f["al"].dtype == al.dtype
        assert f["empty"].shape == (0, 3) and f["empty"].dtype == np.dtype("i2")
