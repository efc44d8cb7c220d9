"""GPU: the tile flush of the throwers (k_throw.h, flush_tile): cells walked by additions instead of a division per cell,
32-bit byte offsets from a workgroup-uniform base, and the one-rounding fixed-point conversion of a cell's charge
(wayne_amd/csrc/flush_math.h; its arithmetic alone: tests/test_flush_math.py).

  * Tile shapes through psf_apply (the int32 frame path): tiles of 1 to 16 columns on frames of side 2, 3 and 17, a tile
    shrunk to more than 512 columns (wider than the workgroup: a step of no whole row), tile widths 511, 512 and 513
    (a step of one row and -1, 0, +1 columns), a ragged last workgroup.  Split mode, fast and exact samplers, the exact
    frame against oracle/split_oracle.c within helpers.split_moved_bound; every electron counted, none off the frame.
  * Addresses and the conversion on an exposure: with a flat cube f0 = 1.25, f1 = f2 = f3 = 0 every product
    n x flat x 2^28 is an integer, so the accumulators must be 1.25 x those of the same run without the flat, exactly,
    in every read plane, the frame's last row and column and the last read included.
  * The conversion's slow path: one cell of more than 2^23 electrons.
"""
import math
import types

import numpy as np
import pytest

import helpers
from wayne_amd import _lib, calibration, detector, engine, grism, synthetic
from wayne_amd.exposure_generator import ExposureGenerator

pytestmark = pytest.mark.gpu

R16, TILE, REACH_MAX = 4.63, 9216, 48       # kLaneR16, kLaneTile, kLaneReachMax (k_narrow.h)


def lane_tile(x, y, smax, N):
    """(tw, th) of the tile of one k_lane workgroup (k_narrow.h, lane_body): the bins' box +- margin, clipped to
    [1, N), shrunk to kLaneTile cells from the rows first."""
    m = math.ceil(np.float32(R16) * np.float32(smax) + np.float32(1.0))
    assert m <= REACH_MAX
    ix, iy = np.floor(x).astype(int), np.floor(y).astype(int)
    x0, x1 = max(ix.min() - m, 1), min(ix.max() + m + 1, N)
    y0, y1 = max(iy.min() - m, 1), min(iy.max() + m + 1, N)
    tw, th = max(x1 - x0, 0), max(y1 - y0, 0)
    while tw * th > TILE and th > 1:
        th = max(th - 2, 1)
    while tw * th > TILE and tw > 1:
        tw = max(tw - 2, 1)
    return tw, th


def frames_against_the_oracle(ctx, counts, x, y, ratio, sl, sh, N, seed, exp=0, sub=0):
    """psf_apply in split mode, fast and exact samplers, both held to the oracle's frame on the same counters.
    Returns (fast frame, oracle frame), N x N."""
    from oracle import clib
    counts = np.asarray(counts, dtype=np.int32)
    want = clib.psf_split_oracle(counts, x, y, ratio, sl, sh, N, seed, exp, sub).astype(np.int64)
    total = int(want.sum())
    got = {}
    for exact in (False, True):
        f = ctx.psf_apply(counts, x, y, ratio, sl, sh, N, N, seed, rng_mode=_lib.RNG_SPLIT, exposure=exp, subsample=sub,
                          exact_samplers=exact)
        f = np.asarray(f).astype(np.int64).reshape(N, N)
        got[exact] = f
        assert f.min() >= 0 and f.sum() <= counts.sum()
        assert f[0].sum() == 0 and f[:, 0].sum() == 0            # (pyparallel_menu.c:93: 0 < pos)
        moved = int(np.abs(f.reshape(-1) - want).sum() + abs(int(f.sum()) - total)) // 2
        bound = helpers.split_moved_bound(counts, total, exact=exact)
        print("N %d exact %s: %d electrons, %d moved (bound %.1f)" % (N, exact, total, moved, bound))
        if exact:
            assert abs(int(f.sum()) - total) <= 2 + total // 100000
            assert moved <= bound, "%d of %d electrons moved" % (moved, total)
    # the fast samplers draw other electrons from the same law: the same total to a few sqrt(total) where electrons
    # can leave the frame, the same total exactly where they cannot
    assert abs(int(got[False].sum()) - total) <= 6 * math.sqrt(max(int(counts.sum()) - total, 0)) + 2 + total // 100000
    return got[False], want.reshape(N, N)


@pytest.mark.parametrize("N", [2, 3, 17])
def test_small_frames_tiles_of_1_to_16_columns(gpu_ctx, N):
    # bins all over a frame smaller than any margin: k_lane's and k_narrow's tiles are the frame without row and
    # column 0 -- 1, 2 and 16 columns -- and k_narrow's are narrower still where its bins sit near the left edge
    rng = np.random.default_rng(100 + N)
    W = 512 + 70                                                  # a ragged second workgroup
    counts = rng.integers(1400, 1600, W).astype(np.int32)
    x = rng.uniform(0.2, N - 0.2, W)
    y = rng.uniform(0.2, N - 0.2, W)
    ratio, sl, sh = np.full(W, 0.2), np.full(W, 0.7), np.full(W, 2.0)
    assert lane_tile(x[:512], y[:512], 2.0, N) == (N - 1, N - 1)
    f, want = frames_against_the_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 300 + N, 1, 2)
    assert f[1:, 1:].sum() == f.sum() > 0
    if N == 2:
        assert f[1, 1] == f.sum()                                 # the one pixel that keeps electrons


def test_a_tile_wider_than_the_workgroup(gpu_ctx):
    # 512 all-wide bins in a row 600 px long on a 700^2 frame: the box +- 25 px is 651 x 51 cells, shrunk from the rows
    # to 651 x 13 -- more columns than the workgroup has threads (q = 0: no step reaches the next row without a wrap)
    W, N = 512, 700
    rng = np.random.default_rng(7)
    counts = rng.integers(1400, 1600, W).astype(np.int32)
    x = 50.3 + 600.0 * np.arange(W) / (W - 1)
    y = np.full(W, 350.4)
    ratio, sl, sh = np.ones(W), np.full(W, 0.7), np.full(W, 5.0)
    tw, th = lane_tile(x, y, 5.0, N)
    assert tw == 651 and th == 13 and tw > 512
    f, want = frames_against_the_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 41, 0, 3)
    assert f.sum() == counts.sum() == want.sum()                  # (far from every edge: every electron counted)


@pytest.mark.parametrize("width", [511, 512, 513])
def test_tile_width_about_the_workgroup_size(gpu_ctx, width):
    # a trace whose first workgroup's tile is `width` columns wide (sigma_h = 6.5: margin 32), 40 more bins for a ragged
    # second workgroup, narrow and wide electrons (k_lane and k_narrow in one grid)
    W, N = 512 + 40, 700
    span = width - 65
    rng = np.random.default_rng(width)
    counts = rng.integers(1400, 1600, W).astype(np.int32)
    x = 100.3 + span * np.arange(W) / 511.0
    y = 350.7 + 0.0007 * np.arange(W)
    ratio, sl, sh = np.full(W, 0.2), np.full(W, 0.7), np.full(W, 6.5)
    tw, th = lane_tile(x[:512], y[:512], 6.5, N)
    assert tw == width and th == 18 - 2 * (width == 513)          # (66 rows shrunk two at a time to kLaneTile cells)
    f, want = frames_against_the_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 43, 2, width)
    assert f.sum() == counts.sum() == want.sum()


def test_a_bin_for_k_throw_beside_the_others(gpu_ctx):
    # bins beyond a lane's 4096 electrons go to k_throw, whose workgroups size their tiles from their slice of the trace
    W, N = 600, 256
    rng = np.random.default_rng(12)
    counts = rng.integers(1400, 1600, W).astype(np.int32)
    counts[::50] = 30000
    x = 90.3 + 0.1 * np.arange(W)
    y = 128.7 + 0.0007 * np.arange(W)
    ratio, sl, sh = np.full(W, 0.9), np.full(W, 0.7), np.full(W, 5.5)
    f, want = frames_against_the_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 44, 1, 1)
    assert f.sum() == counts.sum() == want.sum()


# ---- exposures: the int64 accumulators ----

_dyadic = {}


def dyadic_calibration():
    """The synthetic calibration set with the flat cube f0 = 1.25, f1 = f2 = f3 = 0 (its own object: its own engines)."""
    if not _dyadic:
        cal = calibration.CalibrationSet.synthetic(11)
        for g in list(cal.flat):
            cube = np.zeros_like(cal.flat[g])
            cube[0] = 1.25
            cal.flat[g] = cube
        _dyadic["cal"] = cal
    return _dyadic["cal"]


def tiny_visit(E):
    cal = dyadic_calibration()
    return synthetic.Visit("tiny", detector.WFC3_IR(), grism.G141(cal), cal, n_exposures=1, E=E)


def accumulators(eng, eg, kw, mode, **more):
    ctx = eng.ctx
    ctx.upload(0, eg.build_descriptor(eng, rng_mode=mode, out_dtype=np.float64, **dict(kw, **more)))
    ctx.run_front(0)
    counts, x, y, acc = ctx.debug_fetch(0, acc=True)
    ctx.run_back(0)
    return counts, x, y, acc


ROUTES = [("k_thrower", _lib.RNG_SPLIT, {}),
          ("k_lane batches + k_narrow", _lib.RNG_SPLIT, {"fuse_thrower": 0, "batch": 3}),
          ("k_throw", _lib.RNG_PHILOX, {})]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_dyadic_flat_scales_every_accumulator_exactly(route):
    _, mode, knobs = route
    v = tiny_visit(3e6)                  # ~800 electrons per bin and sub-sample: multinomial bins and lanes' electrons
    eng = engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    eg = ExposureGenerator(v.detector, v.grism, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=v.calibration, seed=v.seed,
                           exposure_index=0)
    N, R = eng.N, eng.R
    kw = v.frame_kwargs(0, cosmic_rate=None)
    # where the spectrum lies with the visit's own pointing; then the pointing that runs the trace off the frame's
    # right edge and ends the scan in its last row
    counts, x, y, _ = accumulators(eng, eg, kw, mode)
    lit = counts > 0
    assert lit.any()
    kw["x_ref"] += (N - 0.5) - x[lit].max() + 3.0
    kw["y_ref"] += (N - 0.5) - y[lit].max()
    for name, value in knobs.items():
        _lib.set_knob_all(name, value)
    counts, x, y, plain = accumulators(eng, eg, kw, mode, add_flat=False)
    counts_f, _, _, flat = accumulators(eng, eg, kw, mode, add_flat=True)
    np.testing.assert_array_equal(counts, counts_f)
    assert plain.shape == flat.shape == (R, N + 10, N + 10)
    # the last row, the last column and the last read take electrons; the border takes none
    assert plain[:, N + 4, 5:N + 5].sum() > 0 and plain[:, 5:N + 5, N + 4].sum() > 0 and plain[R - 1].sum() > 0
    inner = np.zeros(plain.shape[1:], bool)
    inner[5:N + 5, 5:N + 5] = True
    assert not plain[:, ~inner].any() and not flat[:, ~inner].any()
    # whole electrons without the flat, 1.25 x as many with it: exact in fp64 (n 5 2^26 is far below 2^53)
    assert np.array_equal(plain, np.round(plain)) and 0 < plain.sum() <= counts.sum()
    np.testing.assert_array_equal(flat, 1.25 * plain)


def test_a_cell_beyond_the_fast_conversion():
    # One bin of ~1.2e7 narrow electrons per sub-sample at a pixel's centre, sigma_l = 0.06 px (the pixel's edges are
    # 8 sigma away: every electron stays), staring: the cell's charge n x 1.25 is beyond 2^23, the guard of the
    # one-rounding conversion, and its wave converts the way deposit_global does.
    cal = dyadic_calibration()
    gr = grism.G141(cal)
    gr.psf_ratio_poly = types.SimpleNamespace(coeffs=np.zeros(4))                       # no wide electrons
    gr.psf_sigmal_poly = types.SimpleNamespace(coeffs=np.array([0.0, 0.0, 0.0, 0.06]))
    gr.psf_sigmah_poly = types.SimpleNamespace(coeffs=np.array([0.0, 0.0, 0.0, 1.0]))
    v = synthetic.Visit("tiny", detector.WFC3_IR(), gr, cal, n_exposures=1, E=3e7)
    eng = engine.Engine(0, gr, v.detector, cal, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    try:
        eg = ExposureGenerator(v.detector, gr, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=cal, seed=v.seed, exposure_index=0)
        N, R = eng.N, eng.R
        kw = v.frame_kwargs(0, cosmic_rate=None, scan_speed=0.0, x_jitter=0.0, y_jitter=0.0, add_stellar_noise=False,
                            planet_signal=None, scale_factor=1.0)
        # the visit's spectrum: which bin sits mid-frame, and how many electrons a unit of its flux gives
        counts, x, y, _ = accumulators(eng, eg, kw, _lib.RNG_SPLIT, add_flat=False)
        w0 = int(np.argmin(np.abs(x[0] - N / 2.0)))
        assert counts[:, w0].min() > 1000
        i0 = int(np.argmin(np.abs(v.wl - eg_wavelength(v, gr, w0))))
        flux = np.zeros_like(v.stellar_flux)
        flux[i0] = v.stellar_flux[i0] * 1.2e7 / counts[:, w0].mean()
        kw["stellar_flux"] = flux
        kw["x_ref"] += 0.5 - (x[0, w0] - math.floor(x[0, w0]))
        kw["y_ref"] += 0.5 - (y[0, w0] - math.floor(y[0, w0]))
        counts, x, y, plain = accumulators(eng, eg, kw, _lib.RNG_SPLIT, add_flat=False)
        _, _, _, flat = accumulators(eng, eg, kw, _lib.RNG_SPLIT, add_flat=True)
        n = counts[:, w0].astype(np.int64)
        assert counts.sum() == n.sum() and n.min() > 2 ** 23 and n.max() < 2 ** 24
        fx, fy = x[:, w0] - np.floor(x[:, w0]), y[:, w0] - np.floor(y[:, w0])
        assert np.abs(fx - 0.5).max() < 0.1 and np.abs(fy - 0.5).max() < 0.1
        px, py = int(math.floor(x[0, w0])), int(math.floor(y[0, w0]))
        assert 0 < px < N and 0 < py < N
        per_read = np.zeros(R, np.int64)
        np.add.at(per_read, eg._host_vectors["read"], n)
        print("electrons per sub-sample", n, "per read", per_read)
        np.testing.assert_array_equal(plain[:, py + 5, px + 5], per_read.astype(np.float64))
        assert plain.sum() == n.sum()                              # nothing anywhere else
        np.testing.assert_array_equal(flat[:, py + 5, px + 5], 1.25 * per_read)
        assert flat.sum() == 1.25 * n.sum()
    finally:
        eng.close()


def eg_wavelength(v, gr, w):
    """Wavelength of bin w of the descriptor's spectrum: the visit's grid cropped to the grism's limits."""
    from wayne_amd import tools
    i0, i1 = tools.crop_spectrum_ind(gr.wl_limits[0], gr.wl_limits[1], v.wl.copy())
    return v.wl[i0:i1][w]
