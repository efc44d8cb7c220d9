"""GPU: an exposure's run with nothing in front of k_prep_sub (the default) against the launch as it was, k_prep_wl_run
in front of every run (knob prep_wl_per_run = 1).

By default the per-wavelength arrays are worked out when a source's grid is uploaded and kept while grid and grism stay
the same (plan::WlCache), the trace coefficients of the sub-samples are worked out on the host (plan::trace_table) and
the status block is never cleared on the device: the runs of a slot are numbered and a flag counts when its word equals
the number of the run looked at.  With the knob the device does all three per run, which is the reference here: counts,
positions and reads must be equal bit for bit (np.array_equal) -- that holds the host's trace coefficients to the device's.
"""
import numpy as np
import pytest

import helpers
from wayne_amd import _lib, engine

pytestmark = pytest.mark.gpu


def new_engine(v):
    return engine.Engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def launches_of(ctx, name, call):
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = call()
        n = ctx.profile_get()[name]["launches"]
    finally:
        ctx.profile_enable(False)
    return out, n


def test_counts_positions_and_reads_equal_the_per_run_kernels():
    v = helpers.make_visit("small256")
    pg = helpers.product_generator(v, 0)
    eng = new_engine(v)
    try:
        ctx = eng.ctx
        desc = pg.build_descriptor(eng, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **v.frame_kwargs(0))
        got = {}
        for knob in (0, 1, 0):
            ctx.set_knob("prep_wl_per_run", knob)

            def once():
                ctx.upload(0, desc)
                ctx.run_front(0)
                counts, x, y = ctx.debug_fetch(0)[:3]
                ctx.run_back(0)
                return counts.copy(), x.copy(), y.copy(), ctx.download(0).copy()
            out, n = launches_of(ctx, "k_prep_wl", once)
            got.setdefault(knob, []).append((out, n))
        (a, n_a), (a2, n_a2) = got[0]
        (b, n_b), = got[1]
        assert a[0].shape == (v.K, desc._keep[0].size) and a[0].sum() > 1e6
        for i, what in enumerate(("counts", "x", "y", "reads")):
            assert np.array_equal(a[i], b[i]), "%s: %d values differ" % (what, int((a[i] != b[i]).sum()))
            assert np.array_equal(a[i], a2[i]), what
        # the first upload of the grid launches k_prep_wl once; the per-run form launches it with the run; a later upload
        # of the same grid launches nothing
        assert (n_a, n_b, n_a2) == (1, 1, 0), (n_a, n_b, n_a2)
    finally:
        eng.close()


def test_another_grid_of_the_same_length_then_another_length():
    v = helpers.make_visit("small256")
    pg = helpers.product_generator(v, 0)
    kw = v.frame_kwargs(0)
    kw_shift = dict(kw, wl=v.wl + 1e-7)
    kw_half = dict(kw, wl=v.wl[::2], stellar_flux=v.stellar_flux[::2] * 2.0, planet_signal=kw["planet_signal"][:, ::2])
    used = new_engine(v)
    try:
        descs = [pg.build_descriptor(used, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **k) for k in (kw, kw_shift, kw_half)]
        W = [d._keep[0].size for d in descs]
        assert W[0] == W[1] and W[2] < W[0] and not np.array_equal(descs[0]._keep[0], descs[1]._keep[0])
        seen = [used.ctx.synthesize(d).copy() for d in descs]
        for i in (1, 2):
            fresh = new_engine(v)
            try:
                want = fresh.ctx.synthesize(descs[i])
                assert np.array_equal(seen[i], want), "upload %d: %d pixels differ" % (i, int((seen[i] != want).sum()))
            finally:
                fresh.close()
        assert not np.array_equal(seen[0], seen[1])
    finally:
        used.close()


def test_a_new_grism_between_two_uploads_of_the_same_grid():
    v = helpers.make_visit("small256")
    pg = helpers.product_generator(v, 0)
    kw = v.frame_kwargs(0, cosmic_rate=None)
    g = v.grism
    sens_wl, sens_val = v.calibration.sensitivity(g.name)

    def set_grism(eng):
        wmin, wmax = v.calibration.flat_wl.get(g.name, (0.0, 1.0))
        eng.ctx.set_grism(g.trace_coeff, g.wl_solution, np.asarray(g.psf_ratio_poly.coeffs) * 0.8, np.asarray(g.psf_sigmal_poly.coeffs) * 1.2,
                          g.psf_sigmah_poly.coeffs, sens_wl, np.asarray(sens_val) * 1.5, wmin, wmax)
    swapped, fresh = new_engine(v), new_engine(v)
    try:
        desc = pg.build_descriptor(swapped, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **kw)
        first = swapped.ctx.synthesize(desc).copy()
        set_grism(swapped)
        set_grism(fresh)
        a = swapped.ctx.synthesize(desc)
        b = fresh.ctx.synthesize(desc)
        assert np.array_equal(a, b), "%d pixels differ" % int((a != b).sum())
        assert not np.array_equal(a, first)
        # ... and a slot uploaded BEFORE the grism changed and run after it takes the new grism too, as it always did
        swapped.ctx.upload(1, desc)
        fresh.ctx.upload(1, desc)
        set_grism(swapped)
        swapped.ctx.run(1)
        fresh.ctx.run(1)
        assert np.array_equal(swapped.ctx.download(1), fresh.ctx.download(1))
    finally:
        swapped.close()
        fresh.close()


@pytest.mark.parametrize("fetch_between", [False, True])
def test_the_status_word_across_runs_nobody_looked_at(fetch_between):
    v = helpers.make_visit("small256")
    pg = helpers.product_generator(v, 0)
    eng = new_engine(v)
    try:
        ctx = eng.ctx
        desc = pg.build_descriptor(eng, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **v.frame_kwargs(0))
        ctx.upload(0, desc)
        ctx.run(0)
        want = ctx.download(0).copy()
        assert ctx.status(0) == 0 and ctx.reruns == 0

        def run(flagged):
            ctx.set_knob("lane_reach", 5 if flagged else None)    # (5: the run meets a bin beyond its launch sequence)
            ctx.run(0)
        # flagged, then clean: the slot's last run is clean -- nothing is run again
        ctx.upload(0, desc)
        run(True)
        if fetch_between:
            ctx.fetch_async(0)
        run(False)
        assert ctx.status(0) == 0
        n0 = ctx.reruns
        ctx.synchronize()
        assert ctx.reruns == n0 and ctx.status(0) == 0
        assert np.array_equal(ctx.download(0), want)
        # clean, then flagged: bit 1, and the run is repeated when somebody looks
        ctx.upload(0, desc)
        run(False)
        if fetch_between:
            ctx.fetch_async(0)
        run(True)
        assert ctx.status(0) == 2
        if fetch_between:
            # the reads fetched are those of the CLEAN run, and so is the status block that came with them
            got = ctx.wait(0)
            assert ctx.reruns == n0
            assert np.array_equal(got, want)
            assert ctx.status(0) == 2
        ctx.synchronize()
        assert ctx.reruns == n0 + 1 and ctx.status(0) == 0
        assert np.array_equal(ctx.download(0), want)
    finally:
        eng.close()
