"""GPU: wavelength-binned, flat-fielded channels of the device-side extraction (wayne_exposure_set_channels;
k_extract_bins and k_extract_bins_finish).

The oracle in every case is the law restated in numpy (tests/channel_law.py) applied to the reads of the SAME slot, with
the sky level that slot's column extraction formed: channels may differ from it by the order of their float64 sums,
1e-9 of M_p[b] per channel (derived in tests/channel_law.py).  Host side: tests/test_channels.py."""
import collections
import os
import shutil

import numpy as np
import pytest

import channel_law
import extraction_law as law
import helpers
from wayne_amd import _lib, engine, extraction, run_visit
from wayne_amd.visit import VisitRunner

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "fixtures", "mini_visit")
_visits, _planes, _flats = {}, {}, {}
Run = collections.namedtuple("Run", "reads spectra sky channels rejected plan")
WIDE = {"G141": (1.0, 1.8), "G102": (0.7, 1.25)}          # beyond the first order at both ends


def visit(name, n=6):
    if (name, n) not in _visits:
        _visits[(name, n)] = helpers.make_visit(name, n_exposures=n)
    return _visits[(name, n)]


def planes(v):
    if v.name not in _planes:
        _planes[v.name] = law.Planes(v)
    return _planes[v.name]


def flat_of(v):
    if v.name not in _flats:
        _flats[v.name] = channel_law.Flat(v)
    return _flats[v.name]


def engine_of(v):
    return engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def descriptor(v, i, ex, out_dtype=np.float32, **over):
    gen = helpers.product_generator(v, i)
    return gen.build_descriptor(engine_of(v), out_dtype=out_dtype, extraction=ex, **v.frame_kwargs(i, **over)), gen


def fetch(ctx, slot, plan):
    reads = ctx.download(slot)
    spectra, sky = ctx.download_spectra(slot)
    return Run(reads, spectra, sky, ctx.channels(slot) if ctx.has_channels(slot) else None,
               ctx.rejected(slot) if ctx.has_crrej(slot) else None, plan)


def extracted(v, i, ex, out_dtype=np.float32, slot=0, **over):
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(slot, desc)
    ctx.run(slot)
    return fetch(ctx, slot, gen.extraction_plan)


def hand_made(v, plan, out_dtype=np.float32, slot=0, **over):
    """Exposure 0 of `v` extracted with `plan` (an Extraction with channels and a row solution of the test's own)."""
    return extracted(v, 0, plan, out_dtype, slot, **over)


def oracle_of(run, v):
    plan = run.plan
    cr = (plan.crrej.k, plan.crrej.read_noise) if plan.crrej is not None else None
    return channel_law.restate(run.reads, planes(v), plan.row_windows, plan.bg_cols, plan.channels.edges_um,
                               plan.row_solution[0], plan.row_solution[1], plan.steps,
                               flat_of(v) if plan.channels.flat else None, cr, sky=run.sky)


def assert_is_the_law(run, v, what):
    want = oracle_of(run, v)
    channel_law.assert_parity(run.channels, want, what)
    return want


def busy_rate(v, per_interval=30.0):
    dt = np.diff(np.concatenate([[0.0], np.asarray(v.read_times, dtype=float)]))
    N = v.detector.light_sensitive_size(v.SUBARRAY)
    return per_interval * 1024.0 ** 2 / (N * N * dt.min())


def parity_case(name, i, out_dtype, flat, crrej=False, n_channels=20):
    v = visit(name)
    lo, hi = WIDE[v.grism.name]
    ch = extraction.Channels.linear(lo, hi, n_channels).with_flat(flat)
    over = {}
    if name.startswith("tiny"):
        ex = extraction.ExtractionOptions(margin=40, channels=ch, crrej=crrej or None)
    else:
        ex = extraction.ExtractionOptions(channels=ch, crrej=crrej or None)
    if crrej:
        over = dict(cosmic_rate=busy_rate(v, 3.0))
    run = extracted(v, i, ex, out_dtype, **over)
    R, S = v.NSAMP - 1, planes(v).S
    what = "%s[%d] %s flat %d crrej %d" % (name, i, np.dtype(out_dtype).name, flat, crrej)
    assert run.channels.shape == (R + 1, n_channels) and run.channels.dtype == np.float64
    u_lo, u_hi = run.plan.hull
    if name.startswith("tiny"):
        # the frame cuts the first order: the hull ends with the frame (a second strip of at most 10 columns), channels lie wholly
        # and partly outside it, and the windows are clamped at both borders
        assert S == 74 and u_lo < 10 and u_hi == S and (u_hi - u_lo) % 64 <= 10
        assert run.plan.row_windows[:, 0].min() == 5 and run.plan.row_windows[:, 1].max() == S - 5
    if name == "small256":
        rows = run.plan.row_windows[R, 1] - run.plan.row_windows[R, 0]
        assert rows > 2 * 32 and rows % 32 != 0                      # several chunks and a remainder
    if name == "cfg4":
        rows = run.plan.row_windows[R, 1] - run.plan.row_windows[R, 0]
        assert S == 1024 and rows > 20 * 32 and 128 < u_hi - u_lo <= 192      # three 64-column strips
    if crrej:
        assert run.rejected.sum() > 0
    want = assert_is_the_law(run, v, what)
    assert np.abs(want.channels).max() > (100.0 if name.startswith("tiny") else 1000.0)      # (tiny: 3e4 electrons in all)
    if crrej:
        plain = channel_law.restate(run.reads, planes(v), run.plan.row_windows, run.plan.bg_cols, ch.edges_um,
                                    run.plan.row_solution[0], run.plan.row_solution[1], run.plan.steps,
                                    flat_of(v) if flat else None, None, sky=run.sky)
        assert np.abs(plain.channels - want.channels).max() > 1000.0   # the rejection matters to the channels
    return run, want


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "noflat"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("name,i", [("tiny", 0), ("tiny_g102", 0), ("small256", 1), ("stare256", 0)],
                         ids=["tiny", "tiny_g102", "small256", "stare256"])
def test_channels_are_the_law_applied_to_the_slots_reads(name, i, out_dtype, flat):
    parity_case(name, i, out_dtype, flat)


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "noflat"])
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
def test_channels_of_a_rejecting_extraction_are_the_law(out_dtype, flat):
    parity_case("small256", 1, out_dtype, flat, crrej=True)


def test_channels_on_the_full_array():
    parity_case("cfg4", 0, np.float32, True)


def test_the_flat_matters_and_is_the_cubes():
    on, _ = parity_case("small256", 1, np.float32, True)
    off, _ = parity_case("small256", 1, np.float32, False)
    assert on.reads.tobytes() == off.reads.tobytes() and on.spectra.tobytes() == off.spectra.tobytes()
    big = np.abs(off.channels) > 1e4
    assert big.any() and (np.abs(on.channels[big] / off.channels[big] - 1.0) > 1e-4).any()


def constant_solution(S, a, b):
    return np.full(S, a), np.full(S, b)


def small_plan(S, channels, sol, windows=None, steps=extraction.ALL, bg=(6, 26), crrej=None):
    windows = windows or [(100, 140), (110, 150), (120, 167), (20, 246)]
    return extraction.Extraction(windows, bg, steps, crrej, channels, sol)


def test_hand_made_plans():
    v = visit("small256")
    S = 266
    # lambda = 1.0 + 0.005 u: column u0 is at 1.0 + 0.005 u0
    sol = constant_solution(S, 1.0, 0.005)

    def at(u):
        return 1.0 + 0.005 * u

    cases = {
        "one channel": (extraction.Channels([at(60.25), at(200.5)]), sol, None),
        "256 channels": (extraction.Channels.linear(at(40.0), at(232.0), 256), sol, None),        # each 0.75 px wide
        "narrower than a pixel": (extraction.Channels([at(100.2), at(100.6), at(100.7), at(103.0)]), sol, None),
        "left and right of the frame": (extraction.Channels([at(-50.0), at(-10.0), at(100.0), at(120.0), at(300.0), at(340.0)]),
                                        sol, None),
        "one-row window": (extraction.Channels.linear(at(50.0), at(210.0), 7), sol, [(100, 101), (7, 8), (S - 6, S - 5), (130, 131)]),
    }
    # an edge exactly on a pixel boundary: powers of two make (e - a) / b exact
    cases["edges on pixel boundaries"] = (extraction.Channels([64 * 0.0078125, 96 * 0.0078125, 128 * 0.0078125]),
                                          constant_solution(S, 0.0, 0.0078125), None)
    # a wl_a ramp so steep that a channel's columns move by 3 px over a 32-row chunk
    rows = np.arange(S, dtype=np.float64)
    cases["steep ramp"] = (extraction.Channels.linear(at(90.0), at(170.0), 16), (1.0 + 0.005 * (3.0 / 32.0) * (rows - 130.0), np.full(S, 0.005)), None)
    for what, (ch, solution, windows) in cases.items():
        run = hand_made(v, small_plan(S, ch.with_flat(what not in ("one channel", "edges on pixel boundaries")), solution, windows))
        want = assert_is_the_law(run, v, what)
        if what == "left and right of the frame":
            assert (run.channels[:, 0] == 0.0).all() and (run.channels[:, 4] == 0.0).all()
            assert (run.channels[:, 2] != 0.0).all()
        if what == "edges on pixel boundaries":
            # ... where the channel (flat off) is the device's own column spectra, summed
            for b, (c0, c1) in enumerate(((64, 96), (96, 128))):
                col = run.spectra[:, c0:c1].sum(axis=1)
                assert (np.abs(run.channels[:, b] - col) <= law.REL * want.M[:, b]).all(), what
        if what == "steep ramp":
            ua = (ch.edges_um[0] - solution[0][[100, 131]]) / 0.005
            assert abs(ua[1] - ua[0]) > 2.0


def test_integer_edges_give_the_devices_own_column_sums():
    v = visit("small256")
    S = 266
    sol = constant_solution(S, 0.5, 0.0078125)
    edges = 0.5 + 0.0078125 * np.array([30.0, 31.0, 40.0, 100.0, 180.0, 250.0])
    for steps in (extraction.ALL, extraction.ALL & ~extraction.SKY):
        run = hand_made(v, small_plan(S, extraction.Channels(edges, flat=False), sol, steps=steps))
        want = assert_is_the_law(run, v, "integer edges, steps %d" % steps)
        cols = [30, 31, 40, 100, 180, 250]
        for b in range(5):
            col = run.spectra[:, cols[b]:cols[b + 1]].sum(axis=1)
            assert (np.abs(run.channels[:, b] - col) <= law.REL * want.M[:, b]).all(), (steps, b)


def test_steps_off():
    v = visit("small256")
    ch = extraction.Channels.linear(1.1, 1.7, 20)
    for steps in (extraction.ALL & ~extraction.LAST_READ, extraction.ALL & ~extraction.SKY, extraction.GAIN):
        plan = extraction.ExtractionOptions(steps=steps, channels=ch)
        run = extracted(v, 1, plan)
        assert_is_the_law(run, v, "steps %d" % steps)
        if not steps & extraction.LAST_READ:
            assert (run.channels[-1] == 0.0).all() and (run.channels[:-1] != 0.0).any()
        if not steps & extraction.SKY:
            assert (run.sky == 0.0).all()


def test_hull_at_the_cap_and_beyond():
    v = visit("cfg4", 1)
    ctx = engine_of(v).ctx
    S = 1024
    px = 2.0 ** -10                                                  # (exact: an edge falls on a pixel boundary)
    sol = constant_solution(S, 1.0, px)
    windows = [(300, 320)] * 15 + [(290, 331)]
    cap = extraction.MAX_HULL
    assert cap == _lib.MAX_CHANNEL_HULL == 384
    at_cap = extraction.Extraction(windows, channels=extraction.Channels.linear(1.0 + px * 300.0, 1.0 + px * (300.0 + cap), 9),
                                   row_solution=sol)
    assert at_cap.hull == (300, 300 + cap)
    run = extracted(v, 0, at_cap)
    assert_is_the_law(run, v, "hull at the cap")
    never = run.spectra.copy()
    # one column beyond: refused by the Python mirror and by the library, and the slot extracts without channels
    beyond = extraction.Channels.linear(1.0 + px * 300.0, 1.0 + px * (300.5 + cap), 9)
    with pytest.raises(ValueError):
        extraction.Extraction(windows, channels=beyond, row_solution=sol)
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_channels(0, beyond, sol)
    assert e.value.status == _lib.E_INVALID and not ctx.has_channels(0)
    ctx.run(0)
    got, _ = ctx.download_spectra(0)
    assert got.tobytes() == never.tobytes()
    with pytest.raises(_lib.WayneError) as e:
        ctx.channels(0)
    assert e.value.status == _lib.E_STATE


def test_the_planned_solution_is_where_the_device_puts_the_bins():
    v = visit("small256")
    gen = helpers.product_generator(v, 1)
    record = {}
    kw = v.frame_kwargs(1, x_jitter=0.0, y_jitter=0.0)
    gen.scanning_frame(record=record, **kw)
    sub_scale, S = 507 - 128, 266
    wl_a, wl_b = extraction.row_solution(v.grism, kw["x_ref"], kw["y_ref"], sub_scale, S)
    i0, i1 = extraction.tools.crop_spectrum_ind(v.grism.wl_limits[0], v.grism.wl_limits[1], v.wl)
    wl = v.wl[i0:i1]
    x, y = np.asarray(record["x"], dtype=np.float64), np.asarray(record["y"], dtype=np.float64)
    x, y = x.reshape(-1, wl.size), y.reshape(-1, wl.size)
    first = (wl >= v.grism.min_lambda) & (wl <= v.grism.max_lambda)
    row = np.floor(y).astype(int) + 5
    ok = first[None, :] & (row >= 0) & (row < S)
    lam = wl_a[np.clip(row, 0, S - 1)] + wl_b[np.clip(row, 0, S - 1)] * (x + 5.0)
    err = np.abs(lam - wl[None, :])[ok] * 1e4
    print("planned row solution against the device's %d bins: worst %.3f A (allowed 1)" % (ok.sum(), err.max()))
    assert ok.sum() > 1000 and err.max() <= 1.0
    assert np.ptp(y[:, first]) > 20.0                                # the star did move


def test_the_same_exposure_gives_the_same_bytes():
    v = visit("small256")
    ctx = engine_of(v).ctx
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(channels=ch))
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    a, b = fetch(ctx, 0, gen.extraction_plan), fetch(ctx, 1, gen.extraction_plan)
    assert a.channels.tobytes() == b.channels.tobytes() and np.abs(a.channels).max() > 1000.0
    assert a.spectra.tobytes() == b.spectra.tobytes()
    for slot, i in ((0, 0), (1, 2), (2, 0)):                         # other exposures, with other plans, in between
        other, _ = descriptor(v, i, extraction.ExtractionOptions(margin=3 + slot, channels=extraction.Channels.linear(1.2, 1.6, 5 + slot)))
        ctx.upload(slot, other)
        ctx.run(slot)
    ctx.synchronize()
    ctx.upload(3, desc)
    ctx.run(3)
    assert fetch(ctx, 3, gen.extraction_plan).channels.tobytes() == a.channels.tobytes()
    ctx.run(3)                                                       # a second run re-bins, it does not add
    assert fetch(ctx, 3, gen.extraction_plan).channels.tobytes() == a.channels.tobytes()
    # the delivery path (pinned copy) brings the same bytes
    ctx.fetch_spectra_async(3)
    spectra, sky = ctx.wait_spectra(3)
    assert ctx.channels(3).tobytes() == a.channels.tobytes() and spectra.tobytes() == a.spectra.tobytes()


def test_the_second_run_rebins():
    # a lane_reach so low that the first run meets a bin beyond it: status bit 1, and the exposure is run again with
    # k_throw -- its channels are those of the second run's reads
    v = visit("small256")
    ctx = engine_of(v).ctx
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    desc, gen = descriptor(v, 1, extraction.ExtractionOptions(channels=ch))
    before = ctx.reruns
    _lib.set_knob_all("lane_reach", "5")
    try:
        ctx.upload(0, desc)
        ctx.run(0)
        ctx.fetch_spectra_async(0)
        spectra, sky = ctx.wait_spectra(0)
        spectra, sky, channels = spectra.copy(), sky.copy(), ctx.channels(0)
        reads = ctx.download(0)
    finally:
        _lib.set_knob_all("lane_reach", None)
    assert ctx.reruns == before + 1
    run = Run(reads, spectra, sky, channels, None, gen.extraction_plan)
    assert_is_the_law(run, v, "after the second run")
    _lib.set_knob_all("lane_reach", "5")
    try:
        ctx.upload(1, desc)
        ctx.run(1)
        again = fetch(ctx, 1, gen.extraction_plan)                   # (the blocking calls take the same second run)
    finally:
        _lib.set_knob_all("lane_reach", None)
    assert again.channels.tobytes() == channels.tobytes()


def test_nothing_else_moves():
    v = visit("small256")
    ctx = engine_of(v).ctx
    over = dict(cosmic_rate=busy_rate(v, 3.0))
    ch = extraction.Channels.linear(1.05, 1.75, 23)
    for crrej in (None, True):
        plain, gen = descriptor(v, 1, extraction.ExtractionOptions(crrej=crrej), **over)
        binned, gen_b = descriptor(v, 1, extraction.ExtractionOptions(crrej=crrej, channels=ch), **over)
        ctx.upload(0, plain)
        ctx.run(0)
        never = fetch(ctx, 0, gen.extraction_plan)
        assert never.channels is None
        with pytest.raises(_lib.WayneError) as e:
            ctx.channels(0)
        assert e.value.status == _lib.E_STATE
        ctx.upload(1, binned)
        assert ctx.has_channels(1) and ctx.has_crrej(1) == bool(crrej)
        ctx.run(1)
        got = fetch(ctx, 1, gen_b.extraction_plan)
        assert got.channels is not None
        for a, b in ((got.reads, never.reads), (got.spectra, never.spectra), (got.sky, never.sky)):
            assert a.tobytes() == b.tobytes()
        if crrej:
            assert got.rejected.tobytes() == never.rejected.tobytes() and got.rejected.sum() > 0
        # the pinned delivery: the same spectra block in front of the channels
        ctx.fetch_spectra_async(1)
        spectra, sky = ctx.wait_spectra(1)
        assert spectra.tobytes() == never.spectra.tobytes() and sky.tobytes() == never.sky.tobytes()
        if crrej:
            assert ctx.rejected(1).tobytes() == never.rejected.tobytes()
        assert ctx.channels(1).tobytes() == got.channels.tobytes()
        # set_crrej keeps the channels; set_channels(None), a fresh upload and set_extraction clear them
        ctx.set_crrej(1, extraction.CosmicRejection() if crrej else None)
        assert ctx.has_channels(1)
        ctx.run(1)
        assert fetch(ctx, 1, gen_b.extraction_plan).channels.tobytes() == got.channels.tobytes()
        ctx.set_channels(1, None)
        assert not ctx.has_channels(1)
        ctx.upload(2, binned)
        ctx.set_extraction(2, gen.extraction_plan)
        assert not ctx.has_channels(2)
        ctx.upload(3, binned)
        ctx.upload(3, plain)
        for slot in (1, 2, 3):
            ctx.run(slot)
            got = fetch(ctx, slot, gen.extraction_plan)
            assert got.channels is None and got.spectra.tobytes() == never.spectra.tobytes()
            with pytest.raises(_lib.WayneError) as e:
                ctx.channels(slot)
            assert e.value.status == _lib.E_STATE


def test_refusals_leave_the_slot_extracting_without_channels():
    v = visit("small256")
    ctx = engine_of(v).ctx
    S = 266
    nothing, _ = descriptor(v, 1, None)
    ctx.upload(0, nothing)
    good, sol = extraction.Channels.linear(1.1, 1.7, 20), constant_solution(S, 0.9, 0.0046)
    with pytest.raises(_lib.WayneError) as e:                        # no extraction on the slot
        ctx.set_channels(0, good, sol)
    assert e.value.status == _lib.E_STATE
    with pytest.raises(_lib.WayneError) as e:                        # a slot that was never uploaded
        ctx.set_channels(202, good, sol)
    assert e.value.status == _lib.E_STATE
    plain, gen = descriptor(v, 1, True)
    ctx.upload(1, plain)
    ctx.run(1)
    never, never_sky = ctx.download_spectra(1)
    lo, hi = gen.extraction_plan.mask_rows
    nan, inf = float("nan"), float("inf")

    def raw(n, edges, wl_a, wl_b, flags):
        """set_channels past the Python mirror"""
        d = _lib.ChannelsDesc()
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (edges, wl_a, wl_b)]
        d.n_channels = n
        d.edges_um, d.wl_a, d.wl_b = (a.ctypes.data_as(_lib._dp) for a in keep)
        d.flags = flags
        return ctx._L.wayne_exposure_set_channels(ctx._h, 0, _lib.C.byref(d))

    e20 = np.linspace(1.1, 1.7, 21)
    a, b = sol

    def changed(arr, y, value):
        out = arr.copy()
        out[y] = value
        return out

    bad = [(0, e20, a, b, 1), (257, np.linspace(1.1, 1.7, 258), a, b, 1), (20, changed(e20, 3, nan), a, b, 1),
           (20, changed(e20, 20, inf), a, b, 1), (20, changed(e20, 4, e20[3]), a, b, 1), (20, e20[::-1], a, b, 1),
           (20, e20, changed(a, lo, nan), b, 1), (20, e20, changed(a, hi - 1, inf), b, 1), (20, e20, a, changed(b, lo + 1, 0.0), 1),
           (20, e20, a, changed(b, lo + 1, -0.0046), 1), (20, e20, a, changed(b, hi - 1, nan), 1), (20, e20, a, changed(b, lo, inf), 1),
           (20, e20, a, b, 2), (20, e20, a, b, 0x80000001)]          # (a hull beyond the cap: test_hull_at_the_cap_and_beyond)
    for n, (nch, edges, wl_a, wl_b, flags) in enumerate(bad):
        ctx.upload(0, plain)
        ctx.set_channels(0, good, sol)
        assert raw(nch, edges, wl_a, wl_b, flags) == _lib.E_INVALID, n
    # bad values on rows outside every formed window are not looked at
    ctx.upload(0, plain)
    assert raw(20, e20, changed(a, lo - 1, nan), changed(b, hi, -1.0), 1) == 0
    assert raw(20, e20, a, changed(b, lo, nan), 1) == _lib.E_INVALID
    ctx.run(0)                                                       # ... and the slot extracts, without channels
    got, got_sky = ctx.download_spectra(0)
    assert got.tobytes() == never.tobytes() and got_sky.tobytes() == never_sky.tobytes()
    pc = _lib._dp()
    assert ctx._L.wayne_exposure_channels(ctx._h, 0, _lib.C.byref(pc)) == _lib.E_STATE      # (past the Python guard)
    with pytest.raises(_lib.WayneError) as e:
        ctx.channels(0)
    assert e.value.status == _lib.E_STATE
    # the channels exist once the spectra have been fetched
    ctx.upload(0, plain)
    ctx.set_channels(0, good, sol)
    ctx.run(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.channels(0)
    assert e.value.status == _lib.E_STATE
    ctx.download_spectra(0)
    assert ctx.channels(0).shape == (v.NSAMP, 20)


def test_frames_visits_and_observations_carry_the_channels():
    v = visit("tiny")
    ch = extraction.Channels.linear(1.0, 1.8, 12)
    exp = helpers.product_generator(v, 0).scanning_frame(extraction=True, channels=ch, **v.frame_kwargs(0))
    assert exp.channels.shape == (4, 12) and exp.extraction.channels is ch and np.abs(exp.channels).max() > 100.0
    plain = helpers.product_generator(v, 0).scanning_frame(extraction=True, **v.frame_kwargs(0))
    assert not hasattr(plain, "channels") and plain.spectra.tobytes() == exp.spectra.tobytes()
    run = Run(np.stack([r[0] for r in exp.reads]), exp.spectra, exp.sky, exp.channels, None, exp.extraction)
    assert_is_the_law(run, v, "scanning_frame(channels=)")

    runner = VisitRunner(v)
    spectra, sky = runner.run_spectra(range(3), extraction=extraction.ExtractionOptions(channels=ch))
    assert runner.channels.shape == (3, 4, 12) and runner.channels.dtype == np.float64
    assert spectra[0].tobytes() == exp.spectra.tobytes() and runner.channels[0].tobytes() == exp.channels.tobytes()
    runner.run_spectra(range(2))
    assert runner.channels is None

    s = visit("stare256")
    kw = s.frame_kwargs(0)
    for drop in ("scan_speed", "sample_rate", "ssv_generator"):
        kw.pop(drop, None)
    stare = helpers.product_generator(s, 0).staring_frame(extraction=True, channels=extraction.Channels.linear(1.1, 1.7, 20), **kw)
    assert stare.channels.shape == (4, 20) and np.abs(stare.channels).max() > 1000.0


def test_cli_writes_the_channels_and_they_are_the_frames(tmp_path):
    work = str(tmp_path / "visit")
    shutil.copytree(MINI, work)
    yml = os.path.join(work, "params.yml")
    out, plain = str(tmp_path / "channels.npz"), str(tmp_path / "plain.npz")
    obs = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", out, "--channels", "1.1:1.7:20"])
    z = np.load(out)
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start"]
    assert sorted(z.files) == sorted(base + ["channels", "channel_edges_um", "channel_flat", "wl_a", "wl_b"])
    n, NP, S = z["spectra"].shape
    assert z["channels"].shape == (3, NP, 20) and z["wl_a"].shape == (3, S) and z["wl_b"].shape == (3, S)
    assert bool(z["channel_flat"]) and z["channel_edges_um"].tobytes() == np.linspace(1.1, 1.7, 21).tobytes()
    np.testing.assert_array_equal(z["channels"], obs.spectra_result["channels"])
    assert np.abs(z["channels"]).max() > 1000.0
    # Observation.frame_options["channels"] through the frame API: the same exposure, the same bytes
    obs2 = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", plain])
    assert sorted(np.load(plain).files) == sorted(base) and "channels" not in obs2.spectra_result
    obs2.frame_options["channels"] = extraction.Channels.linear(1.1, 1.7, 20)
    obs2.spectra_out, obs2.spectra_only = None, False
    frame = obs2._generate_exposure(obs2.exp_start_times[1], 2, write_fits=False)
    assert frame.channels.tobytes() == z["channels"][1].tobytes() and frame.spectra.tobytes() == z["spectra"][1].tobytes()
    noflat = str(tmp_path / "noflat.npz")
    run_visit.run(["-p", yml, "--max-exposures", "2", "--spectra-only", noflat, "--channels", "1.1:1.7:20", "--no-channel-flat"])
    zn = np.load(noflat)
    assert not bool(zn["channel_flat"]) and zn["channels"].tobytes() != z["channels"][:2].tobytes()
    assert zn["spectra"].tobytes() == z["spectra"][:2].tobytes()
