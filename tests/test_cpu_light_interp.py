"""CPU: the numpy twin of the trilinear LUT interpolation (larndsim_amd/lightLUT.py: interpolation_corners,
interpolated_light_incidence) against its definition -- u = f - 0.5 per axis, corners clamp(floor(u)) and clamp(floor(u) + 1),
corner c = 4 dx + 2 dy + dz with weight (wx[dx] * wy[dy]) * wz[dz], sums in corner order; t0 over the lit corners only."""
import numpy as np
import pytest

import helpers as H
import light_interp_cases as LC
from larndsim_amd import consts, lightLUT
from oracle import oracle as O

EPS = np.finfo(np.float64).eps


@pytest.fixture(autouse=True)
def _module0():
    H.load_cfg("module0")
    yield
    H.load_cfg("module0")


def _fractions(n, vox_div, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 3)) * np.array(vox_div)


@pytest.mark.parametrize("vox_div", [(14, 26, 8), (2, 1, 3), (1, 1, 5)])
def test_weights_are_a_partition_of_unity(vox_div):
    """Each segment's eight weights are >= 0 and sum to 1 within 4 f64 ulp, inside the table, in the clamp region and outside the
    padded borders; the corner indices stay inside the table."""
    f = _fractions(4000, vox_div, 1, -0.3, 1.3)
    for itpc in (0, 1):
        x, y, z = LC.position(f[:, 0], f[:, 1], f[:, 2], itpc, vox_div)
        idx, w = lightLUT.interpolation_corners(x, y, z, itpc, vox_div)
        assert idx.shape == (4000, 8, 3) and w.shape == (4000, 8)
        assert (w >= 0).all()
        s = w[:, 0]
        for c in range(1, 8):
            s = s + w[:, c]
        assert (np.abs(s - 1.0) <= 4 * EPS).all(), np.abs(s - 1.0).max() / EPS
        assert (idx >= 0).all() and (idx < np.array(vox_div)).all()


def test_voxel_centres_reproduce_the_nearest_voxel():
    """At exact voxel centres one weight is 1 within 1e-12 (on the voxel itself) and the incidence equals the oracle's
    nearest-voxel one within 1 f4 ulp."""
    vox_div = (5, 7, 4)
    lut = LC.small_lut(vox_div, 48, 3)
    ijk = np.stack(np.meshgrid(*(np.arange(m) for m in vox_div), indexing="ij"), axis=-1).reshape(-1, 3)
    itpc = (np.arange(len(ijk)) % 2).astype(np.int32)
    pos = [LC.position(i + 0.5, j + 0.5, k + 0.5, t, vox_div) for (i, j, k), t in zip(ijk, itpc)]
    x, y, z = (np.array(v) for v in zip(*pos))
    idx, w = lightLUT.interpolation_corners(x, y, z, itpc, vox_div)
    top = w.argmax(axis=1)
    assert (np.abs(w.max(axis=1) - 1.0) <= 1e-12).all() and (np.sort(w, axis=1)[:, :7] <= 1e-12).all()
    assert np.array_equal(idx[np.arange(len(ijk)), top], ijk)
    r = LC.records(x, y, z, itpc, 4)
    nph, t0d, vox = lightLUT.interpolated_light_incidence(r, lut)
    onph, ot0, ovox = O.light_incidence(r, lut)
    assert np.array_equal(vox, ovox) and np.array_equal(vox, ijk)
    assert (onph > 0).sum() == len(ijk) * 48
    assert LC.ulp_close(nph, onph) and LC.ulp_close(t0d, ot0)


def test_linear_field_is_reproduced():
    """vis = a + b i + c j + d k per channel (coefficients in 1/64ths: the f4 table holds the field exactly), positions inside the
    hull of the voxel centres: the corners and weights reproduce the linear function of (fx - 0.5, fy - 0.5, fz - 0.5) to 1e-12
    relative, and the incidence is that value rounded to f4 (efficiency and photons 1)."""
    vox_div, ndet = (6, 5, 4), 96
    rng = np.random.default_rng(7)
    coef = rng.integers(32, 128, (4, ndet)) / 64.0
    i, j, k = np.meshgrid(*(np.arange(m, dtype=np.float64) for m in vox_div), indexing="ij")
    lut = LC.small_lut(vox_div, ndet, 8)
    field = coef[0] + i[..., None] * coef[1] + j[..., None] * coef[2] + k[..., None] * coef[3]
    lut["vis"] = field
    assert np.array_equal(lut["vis"].astype(np.float64), field)
    f = 0.5 + rng.uniform(0, 1, (500, 3)) * (np.array(vox_div) - 1)
    x, y, z = LC.position(f[:, 0], f[:, 1], f[:, 2], 0, vox_div)
    idx, w = lightLUT.interpolation_corners(x, y, z, 0, vox_div)
    got = np.zeros((500, ndet))
    for c in range(8):
        got += w[:, c, None] * lut["vis"][idx[:, c, 0], idx[:, c, 1], idx[:, c, 2]].astype(np.float64)
    u = f - 0.5
    exp = coef[0] + u[:, 0, None] * coef[1] + u[:, 1, None] * coef[2] + u[:, 2, None] * coef[3]
    assert np.abs(got / exp - 1).max() <= 1e-12
    consts.light.OP_CHANNEL_EFFICIENCY = np.ones(96)
    r = LC.records(x, y, z, np.zeros(500, dtype=np.int32), 9)
    r["n_photons"] = 1.0
    nph, _, _ = lightLUT.interpolated_light_incidence(r, lut)
    own = np.asarray(consts.light.OP_CHANNEL_TO_TPC) == 0
    assert own.sum() == 48 and (nph[:, ~own] == 0).all()
    assert np.array_equal(nph[:, own], got[:, own].astype(np.float32))          # the same sums in the same order
    assert LC.ulp_close(nph[:, own], exp[:, own].astype(np.float32))


def test_one_axis_table_is_np_interp_with_constant_ends():
    """On a (1, 1, nz) table the result is np.interp over the voxel centres along z, constant beyond the outermost centres."""
    vox_div, ndet = (1, 1, 6), 96
    lut = LC.small_lut(vox_div, ndet, 11)
    rng = np.random.default_rng(12)
    f = np.stack([rng.uniform(0, 1, 400), rng.uniform(0, 1, 400), rng.uniform(-0.2, 6.2, 400)], axis=1)
    f[:6, 2] = [0.0, 0.25, 0.5, 5.5, 5.75, 6.0]
    x, y, z = LC.position(f[:, 0], f[:, 1], f[:, 2], 0, vox_div)
    consts.light.OP_CHANNEL_EFFICIENCY = np.ones(96)
    r = LC.records(x, y, z, np.zeros(400, dtype=np.int32), 13)
    r["n_photons"] = 1.0
    nph, _, vox = lightLUT.interpolated_light_incidence(r, lut)
    centres = np.arange(6) + 0.5
    vis = lut["vis"][0, 0].astype(np.float64)
    for ch in range(48):                                              # TPC 0's channels
        exp = np.interp(f[:, 2], centres, vis[:, ch % ndet])
        np.testing.assert_allclose(nph[:, ch], exp, rtol=3e-7, atol=0)
    assert np.array_equal(nph[0, :48], vis[0, :48].astype(np.float32)) and np.array_equal(nph[1, :48], nph[0, :48])
    assert np.array_equal(nph[5, :48], vis[5, :48].astype(np.float32)) and np.array_equal(nph[4, :48], nph[5, :48])
    assert (vox[:, :2] == 0).all()


def test_x_mirror_between_the_tpcs_of_a_module_and_y_flip():
    """TPC 0 (even) counts x voxels from x_min, TPC 1 (odd) from x_max.  A position in the even TPC and its x-mirror in the odd
    one pick the same corners with equal weights; the same x in both picks mirrored x indices with the two x weights swapped.
    The y index runs against y: the corner with dy = 0 is the one at the larger y."""
    vox_div = (14, 26, 8)
    nx, ny, nz = vox_div
    f = _fractions(300, vox_div, 21)
    x0, y0, z0 = LC.position(f[:, 0], f[:, 1], f[:, 2], 0, vox_div)
    x_min, x_max = LC.padded_borders(0)[:2]
    assert LC.padded_borders(1)[:4] == LC.padded_borders(0)[:4]      # the two TPCs share their x and y borders
    _, _, z1 = LC.position(f[:, 0], f[:, 1], f[:, 2], 1, vox_div)
    idx0, w0 = lightLUT.interpolation_corners(x0, y0, z0, 0, vox_div)
    idx1, w1 = lightLUT.interpolation_corners(x_min + x_max - x0, y0, z1, 1, vox_div)
    assert np.array_equal(idx0, idx1)
    np.testing.assert_allclose(w1, w0, rtol=0, atol=1e-11)
    idx2, w2 = lightLUT.interpolation_corners(x0, y0, z1, 1, vox_div)
    swap = [4, 5, 6, 7, 0, 1, 2, 3]                                    # dx <-> 1 - dx
    # away from the clamp region (there both x corners are one voxel, mirrored or not)
    inner = (f[:, 0] > 0.5 + 1e-9) & (f[:, 0] < nx - 0.5 - 1e-9) & (np.abs(f[:, 0] - 0.5 - np.round(f[:, 0] - 0.5)) > 1e-9)
    assert inner.sum() > 200
    assert np.array_equal(idx2[inner][:, swap, 0], nx - 1 - idx0[inner][:, :, 0])
    assert np.array_equal(idx2[inner][:, swap, 1:], idx0[inner][:, :, 1:])
    np.testing.assert_allclose(w2[inner][:, swap], w0[inner], rtol=0, atol=1e-11)
    # y: a quarter of a voxel below the centre of row j (smaller y): corners j (dy = 0, weight 0.75) and j + 1 (0.25)
    y_min, y_max = LC.padded_borders(0)[2:4]
    j = 9
    y = y_max - (j + 0.75) / ny * (y_max - y_min)
    idx, w = lightLUT.interpolation_corners(x0[:1], [y], z0[:1], 0, vox_div)
    dy = (np.arange(8) >> 1) & 1
    assert np.array_equal(idx[0, :, 1], j + dy)
    wy = np.array([w[0, dy == 0].sum(), w[0, dy == 1].sum()])
    np.testing.assert_allclose(wy, [0.75, 0.25], rtol=0, atol=1e-12)
    assert lightLUT.interpolation_corners(x0[:1], [y + 0.1], z0[:1], 0, vox_div)[1][0, dy == 0].sum() > wy[0]


def test_t0_skips_dark_corners():
    """t0 is the weight-renormalised mean over the corners with visibility > 0; with all eight dark it is the nearest voxel's t0
    and n_photons_det is 0."""
    vox_div, ndet = (3, 3, 3), 96
    lut = LC.small_lut(vox_div, ndet, 31)
    rng = np.random.default_rng(32)
    dark = rng.random(lut["vis"].shape) < 0.4
    lut["vis"][dark] = 0.0
    lut["vis"][:2, :2, :2, 5] = 0.0                        # channel 5: all eight corners of the first cell dark
    lut["vis"][:2, :2, :2, 6] = 0.0                        # channel 6: one lit corner
    lut["vis"][1, 0, 1, 6] = 3e-3
    f = 0.5 + rng.uniform(0.05, 0.95, (200, 3))          # inside the first cell of voxel centres: corners (0|1, 0|1, 0|1)
    x, y, z = LC.position(f[:, 0], f[:, 1], f[:, 2], 0, vox_div)
    r = LC.records(x, y, z, np.zeros(200, dtype=np.int32), 33)
    assert consts.light.LIGHT_TRIG_MODE == 0
    nph, t0d, vox = lightLUT.interpolated_light_incidence(r, lut)
    idx, w = lightLUT.interpolation_corners(x, y, z, 0, vox_div)
    assert (idx.min(axis=1) == 0).all() and (idx.max(axis=1) == 1).all()
    vis = lut["vis"].astype(np.float64)
    t0 = lut["t0"].astype(np.float64)
    mus = 1e-6 * 1e9
    seen_partial = 0
    for ch in range(96):
        v = np.stack([vis[idx[:, c, 0], idx[:, c, 1], idx[:, c, 2], ch] for c in range(8)], axis=1)
        t = np.stack([t0[idx[:, c, 0], idx[:, c, 1], idx[:, c, 2], ch] for c in range(8)], axis=1)
        lit = v > 0
        S = (w * lit).sum(axis=1)
        near = t0[vox[:, 0], vox[:, 1], vox[:, 2], ch]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(S > 0, (w * lit * t).sum(axis=1) / S, near)
        exp = (mean + r["t0"] * mus) / mus
        np.testing.assert_allclose(t0d[:, ch], exp, rtol=3e-7, atol=0)
        seen_partial += int(((lit.sum(axis=1) > 0) & (lit.sum(axis=1) < 8)).sum())
        # the mean lies between the lit corners' times, whatever the dark ones hold
        some = lit.any(axis=1)
        lo, hi = np.where(lit, t, np.inf).min(axis=1), np.where(lit, t, -np.inf).max(axis=1)
        assert ((mean[some] >= lo[some] - 1e-9) & (mean[some] <= hi[some] + 1e-9)).all()
    assert seen_partial > 1000
    # all dark: nearest voxel's t0, no photons -- also on a channel of the segment's own TPC
    exp5 = (t0[vox[:, 0], vox[:, 1], vox[:, 2], 5] + r["t0"] * mus) / mus
    assert np.array_equal(t0d[:, 5], exp5.astype(np.float32)) and (nph[:, 5] == 0).all()
    # one lit corner: its t0 whatever its weight, and photons from its share alone
    exp6 = (t0[1, 0, 1, 6] * np.ones(200) + r["t0"] * mus) / mus
    np.testing.assert_allclose(t0d[:, 6], exp6, rtol=3e-7, atol=0)
    c_lit = 4 * 1 + 2 * 0 + 1
    exp_n = consts.light.OP_CHANNEL_EFFICIENCY[6] * (w[:, c_lit] * vis[1, 0, 1, 6]) * r["n_photons"]
    np.testing.assert_allclose(nph[:, 6], exp_n, rtol=3e-7, atol=0)


def test_segments_outside_every_tpc_keep_zeros():
    vox_div = (3, 4, 2)
    lut = LC.small_lut(vox_div, 8, 41)
    r = LC.mixed_segments(70, vox_div, 42)
    out = r["pixel_plane"] == consts.detector.DEFAULT_PLANE_INDEX
    assert 0 < out.sum() < 70
    nph, t0d, vox = lightLUT.interpolated_light_incidence(r, lut)
    assert (nph[out] == 0).all() and (t0d[out] == 0).all() and (vox[out] == 0).all()
    assert (nph[~out] > 0).any(axis=1).all()
