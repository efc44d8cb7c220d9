"""GPU: contaminating field stars (wayne_exposure_set_sources) on the small synthetic visits.

A contaminant's part of an exposure is the front half of the single-source exposure with the offset positions, its own
spectrum, no depth, no cosmic rays and seed = wayne_source_seed(seed, tag): the accumulators of T + C1 + C2 are the
integer sums of those of T, C1 and C2 run alone.  Tolerances (stated per test):
  * accumulated electrons without the flat: exact (int64 accumulators, integer electrons);
  * with the flat: each source is planned and launched exactly as it would be alone, so its tile flushes are the same
    ones -- still exact; the bound of test_exposure_gpu.py (flushes * 2^-29 e- per pixel) is the stated allowance;
  * counts against the oracle: exact without stellar noise; with it, < 1e-5 of the bins may differ (a 1-ulp log()
    difference on a decision boundary of the fp64 Poisson sampler, as in test_exposure_gpu.py);
  * positions against the oracle's SpectrumTrace: 1e-9 px.
"""
import numpy as np
import pytest

import helpers
from oracle import wayne_oracle as wo
from wayne_amd import _lib
from wayne_amd.sources import Contaminant

pytestmark = pytest.mark.gpu

DET_OFF = dict(add_stellar_noise=False, sky_background=0.0, cosmic_rate=None, add_dark=False, add_read_noise=False)
MODES = [_lib.RNG_SPLIT, _lib.RNG_PHILOX]


def prepare(name, rng_mode=_lib.RNG_SPLIT, i=0, contaminants=None, **over):
    v = helpers.make_visit(name, n_exposures=i + 1)
    kw = v.frame_kwargs(i, **over)
    pg = helpers.product_generator(v, i)
    pg.prepare(rng_mode=rng_mode, out_dtype=np.float64, contaminants=contaminants, **kw)
    eng, desc, _ = pg._prepared
    pg._prepared = None
    return v, kw, pg, eng, desc


def target_spectrum(desc):
    return desc._keep[0], desc._keep[1]      # (make_desc keeps the cropped wl and flux first)


def contaminant(desc, tag, dx, dy, ratio=0.3, tilt=0.0):
    wl, fl = target_spectrum(desc)
    return Contaminant(dx, dy, wl.copy(), fl * ratio * (1.0 + tilt * (wl - wl.mean())), tag)


def single(pg, desc, c):
    """The single-source exposure of contaminant c: offset positions, its spectrum, no depth, no cosmic rays, the
    derived seed; everything else the exposure's."""
    h = pg._host_vectors
    return _lib.make_desc(_lib.source_seed(desc.seed, c.tag), desc.exposure_index, desc.flags, desc.sub_scale, c.wl, c.flux,
                          None, h["x_ref"] + c.dx, h["y_ref"] + c.dy, h["dur"], h["read"], pg._read_dt, replay_seed=h["seeds"],
                          rng_mode=desc.rng_mode, threads_compat=desc.threads_compat, sky_ct_s=desc.sky_ct_s,
                          cosmic_rate=-1.0, scale_factor=desc.scale_factor, noise_mean=desc.noise_mean,
                          noise_std=desc.noise_std)


def front(ctx, desc, sources=None, slot=0):
    """upload (+ sources), front half -> accumulators; then the back half so that the slot ends clean."""
    ctx.upload(slot, desc)
    if sources is not None:
        ctx.set_sources(slot, sources)
    ctx.run_front(slot)
    acc = ctx.debug_fetch(slot, acc=True)[3]
    ctx.run_back(slot)
    return acc, ctx.download(slot).copy()


@pytest.mark.parametrize("mode", MODES)
def test_no_sources_leaves_the_exposure_as_it_was(mode):
    v, kw, pg, eng, desc = prepare("small256", mode)
    ctx = eng.ctx
    ctx.upload(0, desc)
    ctx.run(0)
    plain = ctx.download(0).copy()
    ctx.upload(0, desc)
    ctx.set_sources(0, [])
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), plain)
    # a slot that ran with a contaminant far from the target (its accumulators outside the target's boxes) and is then
    # uploaded again without: nothing of the contaminant is left in it
    far = contaminant(desc, 1, -90.0, 70.0, ratio=1.0)
    ctx.upload(5, desc)
    ctx.set_sources(5, [far])
    ctx.run(5)
    with_far = ctx.download(5).copy()
    assert np.abs(with_far - plain).max() > 100
    ctx.upload(5, desc)
    ctx.run(5)
    np.testing.assert_array_equal(ctx.download(5), plain)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("flat", [False, True])
def test_sources_add_exactly_and_commute(mode, flat):
    v, kw, pg, eng, desc = prepare("small256", mode, **dict(DET_OFF, add_flat=flat, add_stellar_noise=True))
    ctx = eng.ctx
    c1 = contaminant(desc, 1, 25.0, -30.0, ratio=0.5)
    c2 = contaminant(desc, 2, -40.0, 12.0, ratio=0.2, tilt=1.0)
    r0 = ctx.reruns
    acc_t, _ = front(ctx, desc)
    acc_1, _ = front(ctx, single(pg, desc, c1))
    acc_2, _ = front(ctx, single(pg, desc, c2))
    acc_all, reads_12 = front(ctx, desc, [c1, c2])
    _, reads_21 = front(ctx, desc, [c2, c1])
    assert ctx.reruns == r0
    assert acc_1.sum() > 1e4 and acc_2.sum() > 1e4
    if flat:
        flushes = 4096.0 * v.K * 3
        np.testing.assert_allclose(acc_all, acc_t + acc_1 + acc_2, rtol=0, atol=flushes * 2.0 ** -29)
    else:
        np.testing.assert_array_equal(acc_all, acc_t + acc_1 + acc_2)
    np.testing.assert_array_equal(reads_12, reads_21)


@pytest.mark.parametrize("noise", [False, True])
def test_each_source_against_the_oracle(noise):
    over = dict(DET_OFF, add_stellar_noise=noise, add_flat=False, x_jitter=0.0, y_jitter=0.0)
    v, kw, pg, eng, desc = prepare("tiny", _lib.RNG_SPLIT, **over)
    near = contaminant(desc, 1, 6.0, -9.0, ratio=0.4)
    far = contaminant(desc, 3, 300.0, -260.0, ratio=0.8, tilt=0.5)    # across the field: other trace coefficients
    ctx = eng.ctx
    ctx.upload(0, desc)
    ctx.set_sources(0, [near, far])
    ctx.run_front(0)
    got = [ctx.debug_fetch_source(0, i) for i in (1, 2)]
    ctx.run_back(0)
    ctx.synchronize()
    eo = helpers.oracle_generator(v)
    N = pg.detector.light_sensitive_size(v.SUBARRAY)
    for c, (counts, x, y) in zip((near, far), got):
        kc = dict(kw, x_ref=kw["x_ref"] + c.dx, y_ref=kw["y_ref"] + c.dy, wl=c.wl, stellar_flux=c.flux,
                  planet_signal=np.zeros((v.K, c.wl.size)))
        orec = {}
        draws = wo.PhiloxDraws(_lib.source_seed(v.seed, c.tag), 0, N)
        eo.scanning_frame(threads=2, draws=draws, thrower="oracle", record=orec, **helpers.oracle_kwargs(kc))
        want = np.stack(orec["counts"])
        if noise:
            assert (counts != want).mean() < 1e-5
        else:
            np.testing.assert_array_equal(counts, want)
        assert counts.sum() > 1000
        np.testing.assert_allclose(x, np.stack(orec["x"]), rtol=0, atol=1e-9)
        np.testing.assert_allclose(y, np.stack(orec["y"]), rtol=0, atol=1e-9)
    # the far source's spectrum is not the near one's shifted by the difference of the offsets: the field-dependent
    # trace and dispersion place its bins elsewhere
    shift = got[1][1] - got[0][1] - (far.dx - near.dx)
    assert np.abs(shift).max() > 1e-3


@pytest.mark.parametrize("mode", MODES)
def test_accumulators_stay_inside_the_boxes(mode):
    v, kw, pg, eng, desc = prepare("small256", mode, **DET_OFF)
    ctx = eng.ctx
    far = contaminant(desc, 1, -100.0, 80.0, ratio=0.6)
    partly = contaminant(desc, 2, 150.0, -5.0, ratio=0.6)        # the trace runs off the right edge
    off = contaminant(desc, 3, 900.0, 900.0, ratio=0.6)          # nowhere on the sub-array
    ctx.upload(0, desc)
    ctx.run(0)
    plain = ctx.download(0).copy()
    ctx.upload(2, desc)
    ctx.set_sources(2, [far, partly, off])
    ctx.run_front(2)
    acc = ctx.debug_fetch(2, acc=True)[3]
    counts = [ctx.debug_fetch_source(2, i)[0].sum() for i in range(4)]
    use_box, boxes, _ = ctx.debug_boxes(2)
    assert use_box
    for r in range(acc.shape[0]):
        x0, x1, y0, y1 = boxes[r]
        inside = np.zeros(acc[r].shape, dtype=bool)
        inside[y0:y1, x0:x1] = True
        assert not acc[r][~inside].any(), r
    # on the frame: every electron of the target and the far source, part of the partly-off one, none of the last
    on = acc.sum()
    assert counts[3] > 0 and on < sum(counts[:3])
    assert on > counts[0] * 0.5 + counts[1] * 0.5
    ctx.run_back(2)
    ctx.synchronize()
    # the next exposure in the slot is clean
    ctx.upload(2, desc)
    ctx.run(2)
    np.testing.assert_array_equal(ctx.download(2), plain)


def test_a_contaminant_has_streams_of_its_own():
    v, kw, pg, eng, desc = prepare("small256", _lib.RNG_SPLIT, **dict(DET_OFF, add_stellar_noise=True, add_flat=False,
                                                                        planet_signal=None))
    ctx = eng.ctx
    wl, fl = target_spectrum(desc)
    twin = Contaminant(0.0, 0.0, wl.copy(), fl.copy(), 1)
    acc_t, _ = front(ctx, desc)
    acc_all, _ = front(ctx, desc, [twin])
    ctx.upload(0, desc)
    ctx.set_sources(0, [twin])
    ctx.run_front(0)
    ct, cc = ctx.debug_fetch_source(0, 0)[0], ctx.debug_fetch_source(0, 1)[0]
    ctx.run_back(0)
    ctx.synchronize()
    assert not np.array_equal(acc_all, 2 * acc_t)
    assert not np.array_equal(ct, cc)
    # expected counts (noise off) as the mean of the two draws' law; per-bin deviations uncorrelated: |r| < 0.1
    # (n = K x W ~ 3000 bins: the standard error of r is ~0.02)
    _, _, pg2, eng2, desc2 = prepare("small256", _lib.RNG_SPLIT, **dict(DET_OFF, add_flat=False, planet_signal=None))
    ctx.upload(0, desc2)
    ctx.run_front(0)
    lam = ctx.debug_fetch(0)[0].astype(float)
    ctx.run_back(0)
    ctx.synchronize()
    m = lam > 20
    r = np.corrcoef((ct - lam)[m], (cc - lam)[m])[0, 1]
    assert m.sum() > 500 and abs(r) < 0.1, r


def test_the_rerun_repeats_every_source():
    v, kw, pg, eng, desc = prepare("small256", _lib.RNG_SPLIT)
    ctx = eng.ctx
    cs = [contaminant(desc, 1, 25.0, -30.0, ratio=0.5), contaminant(desc, 2, -40.0, 12.0, ratio=0.2, tilt=1.0)]
    ctx.upload(0, desc)
    ctx.set_sources(0, cs)
    ctx.run(0)
    want = ctx.download(0).copy()
    n0 = ctx.reruns
    ctx.set_knob("lane_reach", 5)
    try:
        ctx.upload(0, desc)
        ctx.set_sources(0, cs)
        ctx.run(0)
        got = ctx.download(0).copy()
    finally:
        ctx.set_knob("lane_reach", None)
    assert ctx.reruns == n0 + 1
    np.testing.assert_array_equal(got, want)


def test_replay_mode_refuses_contaminants():
    v, kw, pg, eng, desc = prepare("tiny", _lib.RNG_REPLAY)
    ctx = eng.ctx
    ctx.upload(0, desc)
    ctx.run(0)
    plain = ctx.download(0).copy()
    ctx.upload(0, desc)
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_sources(0, [contaminant(desc, 1, 5.0, 5.0)])
    assert e.value.status == _lib.E_INVALID
    ctx.run(0)                              # the slot still runs, without the contaminant
    np.testing.assert_array_equal(ctx.download(0), plain)


def test_bad_lists_are_refused_and_the_slot_stays_usable():
    v, kw, pg, eng, desc = prepare("tiny", _lib.RNG_SPLIT)
    ctx = eng.ctx
    ctx.upload(0, desc)
    ctx.run(0)
    plain = ctx.download(0).copy()
    ctx.upload(0, desc)
    good = contaminant(desc, 1, 5.0, 5.0)
    bad_lists = [[good, contaminant(desc, 1, 8.0, 0.0)],                 # duplicate tag
                 [contaminant(desc, 2, 0.0, 0.0)] * 9]                    # more than 8
    for bad in bad_lists:
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_sources(0, bad)
        assert e.value.status == _lib.E_INVALID
    nan = contaminant(desc, 1, 5.0, 5.0)
    nan.dx = float("nan")
    for c in (nan,):
        with pytest.raises(_lib.WayneError):
            ctx.set_sources(0, [c])
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), plain)


@pytest.mark.parametrize("mode", MODES)
def test_a_contaminant_dilutes_the_depth_on_its_rows_only(mode):
    # all noise sources off; depth d on every bin in transit, 0 out of it; the white-light depth recovered from the
    # frames' electron totals is d N_T / (N_T + N_C) when the contaminant shares the target's rows, d when the
    # target's rows are extracted apart from it (to within the fraction of electrons thrown off the frame)
    d = 0.01
    base = dict(DET_OFF, add_flat=False)
    v, kw, pg, eng, desc_out = prepare("small256", mode, **dict(base, planet_signal=None))
    _, _, _, _, desc_in = prepare("small256", mode, **dict(base, planet_signal=np.full((v.K, v.wl.size), d)))
    ctx = eng.ctx

    def totals(desc, c, rows=None):
        ctx.upload(0, desc)
        ctx.set_sources(0, [c])
        ctx.run_front(0)
        acc = ctx.debug_fetch(0, acc=True)[3]
        n_t, n_c = (ctx.debug_fetch_source(0, i)[0].sum() for i in (0, 1))
        ctx.run_back(0)
        ctx.synchronize()
        tot = acc.sum() if rows is None else acc[:, rows[0]:rows[1], :].sum()
        return tot, float(n_t), float(n_c), acc.sum()

    same_rows = contaminant(desc_out, 1, -60.0, 0.0, ratio=0.5)
    f_out, nt_out, nc, on_out = totals(desc_out, same_rows)
    f_in, nt_in, _, _ = totals(desc_in, same_rows)
    off = 1.0 - on_out / (nt_out + nc)
    assert off < 0.3
    want = d * nt_out / (nt_out + nc)
    assert abs((1.0 - f_in / f_out) - want) <= d * off + 1e-4, (1.0 - f_in / f_out, want)
    assert abs(want - d) > 0.2 * d                       # the dilution is there to be seen
    # the contaminant on rows of its own: extract the target's rows only
    ctx.upload(0, desc_out)
    ctx.run_front(0)
    acc_t = ctx.debug_fetch(0, acc=True)[3]
    ctx.run_back(0)
    ctx.synchronize()
    ys = np.nonzero(acc_t.sum(axis=(0, 2)))[0]
    rows = (int(ys.min()), int(ys.max()) + 1)
    apart = contaminant(desc_out, 1, 0.0, float(rows[1] - rows[0] + 40), ratio=0.5)
    f_out, nt_out, _, _ = totals(desc_out, apart, rows)
    f_in, _, _, _ = totals(desc_in, apart, rows)
    assert abs((1.0 - f_in / f_out) - d) <= d * off + 1e-4
