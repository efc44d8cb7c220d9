"""GPU: 16-bit unsigned reads (WAYNE_F_OUT_U16, out_dtype=np.uint16, --uint16-reads).

The law: a uint16 read is the float32 read of the same k_ramp instantiation -- the same arithmetic, the same Philox
counters -- quantised in the kernel's store,

    q = v is NaN ? 0 : (uint16) min(max(rintf(v), 0), 65535)          (round half to even, saturating)

so for the same visit, exposure and seeds it equals np.clip(np.rint(f32), 0, 65535).astype(np.uint16) of the float32
reads with ZERO differences: derived, not measured (results do not depend on what ran before: tests/test_soak_gpu.py).
Against the oracle, independently of the float path: half a count of rounding plus the float32-read tolerance T1 of
DESIGN.md section 6 (0.02 DN + 2e-7 relative).  Host side of the mode: tests/test_uint16_reads.py."""
import os
import shutil

import numpy as np
import pytest

import helpers
from oracle import wayne_oracle as wo
from wayne_amd import _lib, calibration, detector, engine, fitsio, grism, run_visit, synthetic, traps as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "fixtures", "mini_visit")
OFF = dict(add_stellar_noise=False, sky_background=0.0, cosmic_rate=None, add_dark=False, add_read_noise=False)
U16 = "unsigned short"


def quantised(f32):
    assert f32.dtype == np.float32 and np.isfinite(f32).all()
    return np.clip(np.rint(f32), 0, 65535).astype(np.uint16)


def engine_of(v):
    return engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def frames(v, out_dtype, staring=False, i=0, want_variant=None, **opts):
    """The reads of exposure i as one array, and the k_ramp instantiation that made them."""
    pg = helpers.product_generator(v, i)
    kw = v.frame_kwargs(i, **opts.pop("over", {}))
    if staring:
        kw = {k: kw[k] for k in kw if k not in ("scan_speed", "sample_rate", "ssv_generator")}
        exp = pg.staring_frame(out_dtype=out_dtype, **opts, **kw)
    else:
        exp = pg.scanning_frame(out_dtype=out_dtype, **opts, **kw)
    reads = np.stack([r[0] for r in exp.reads])
    assert reads.dtype == np.dtype(out_dtype)
    variant = engine_of(v).ctx.ramp_variant(0)
    if want_variant is not None:
        assert variant == want_variant % (U16 if np.dtype(out_dtype) == np.uint16 else "float"), variant
    return reads


_special = {}


def sky_visit(kind):
    """tiny128 over a master sky that sends the host's sky plan (host_plan.h plan_sky) to one of its other samplers:
    `pieces` -- hot pixels (x 50) in the sub-array's part of the plane, so that a pixel's remainder above its level
    exceeds the 16 electrons one sequential search draws (tests/test_extremes_gpu.py hot_sky_visit, here inside the
    128 x 128 crop); `direct` is reached with the ordinary plane and a rate no 256-entry alias table holds."""
    if kind not in _special:
        cal = calibration.CalibrationSet.synthetic(11)
        if kind == "pieces":
            cal.sky["G141"][450:565:9, 450:565:7] *= np.float32(50.0)
        _special[kind] = cal
    cal = _special[kind]
    return synthetic.Visit("tiny128", detector.WFC3_IR(), grism.G141(cal), cal, n_exposures=1)


def direct_rate(v):
    """A sky rate whose per-read mean is ~200 electrons on the typical pixel: 200 + 8 sqrt(200) + 8 > 255, no table."""
    dt = np.diff(np.concatenate([[0.0], v.read_times])).max()
    sky = v.calibration.sky[v.grism.name]
    return 200.0 / (dt * float(np.median(sky[sky > 0])))


LAW_CASES = {
    #                  visit        staring  options of the frame                          instantiation (%s = reads' type)
    "tiny_S74":       ("tiny",      False,   {},                                           None),
    "tiny128":        ("tiny128",   False,   {},                                           "k_ramp<%s, true, 1, false, true>"),
    "tiny128_exact":  ("tiny128",   False,   dict(exact_samplers=True),                    "k_ramp_wide<%s, false, 1, false>"),
    "stare256":       ("stare256",  True,    {},                                           None),
    "small256_allon": ("small256",  False,   {},                                           "k_ramp<%s, true, 1, false, true>"),
    "sky_direct":     ("direct",    False,   {},                                           "k_ramp_wide<%s, true, 0, false>"),
    "sky_pieces":     ("pieces",    False,   dict(over=dict(sky_background=20.0)),         "k_ramp<%s, true, 2, false, false>"),
    "noise_stage":    ("tiny128",   False,   dict(over=dict(noise_mean=1.5, noise_std=0.5)), "k_ramp_wide<%s, true, 1, true>"),
    "charge_traps":   ("tiny128",   False,   dict(charge_traps=T.ChargeTraps()),           "k_ramp_trap<%s, true, 1, false, true>"),
}


@pytest.mark.parametrize("case", list(LAW_CASES))
def test_uint16_reads_are_the_quantised_float32_reads_bit_for_bit(case):
    name, staring, opts, variant = LAW_CASES[case]
    if name in ("direct", "pieces"):
        v = sky_visit(name)
        if name == "direct":
            opts = dict(over=dict(sky_background=direct_rate(v)))
    else:
        v = helpers.make_visit(name)
    f32 = frames(v, np.float32, staring, want_variant=variant, **dict(opts))
    u16 = frames(v, np.uint16, staring, want_variant=variant, **dict(opts))
    S = v.detector.full_size(v.SUBARRAY)
    assert u16.shape == f32.shape == (v.NSAMP, S, S)
    if case == "tiny_S74":
        assert S * S == 5476                                    # a partial last workgroup and a partial last wave
    want = quantised(f32)
    assert int((u16 != want).sum()) == 0
    # the comparison is not a trivial one: many levels (the smallest case, 64 x 64 without a bias file, spans ~35 DN),
    # values that needed rounding, and the star's charge in the last read
    assert len(np.unique(want)) > 16 and float((f32 != np.rint(f32)).mean()) > 0.5
    assert float(f32[-1].sum(dtype=np.float64)) > float(f32[0].sum(dtype=np.float64))
    # plane 0 (the zero read) and the reference-pixel border went through the same store
    np.testing.assert_array_equal(u16[0], want[0])
    np.testing.assert_array_equal(u16[:, :5, :], want[:, :5, :])


def test_low_saturation_is_exercised():
    # no bias: the reference pixels are read noise around zero (sigma 6 DN), half of them negative
    v = helpers.make_visit("tiny128")
    over = dict(add_initial_bias=False, add_read_noise=True)
    f32 = frames(v, np.float32, over=over)
    u16 = frames(v, np.uint16, over=over)
    low = f32 < -0.5
    assert int(low.sum()) > 100
    assert (u16[low] == 0).all()
    assert int((u16 != quantised(f32)).sum()) == 0


def test_high_saturation_is_exercised():
    over = dict(clip_values_det_limits=False, add_non_linear=False)
    E = 3e7
    for _ in range(5):                                          # raised until the ramp passes the ADC's range
        v = helpers.make_visit("small256", E=E)
        f32 = frames(v, np.float32, over=over)
        if int((f32 > 65535.5).sum()) > 100:
            break
        E *= 4.0
    high = f32 > 65535.5
    assert int(high.sum()) > 100
    u16 = frames(v, np.uint16, over=over)
    assert (u16[high] == 65535).all()
    assert int((u16 != quantised(f32)).sum()) == 0
    # with the detector's own limit on, the float limit of 78000 DN (+ zero read + read noise) lands on 65535 too
    # (four times the flux again, so that the ramp passes that limit as well)
    v = helpers.make_visit("small256", E=4.0 * E)
    over = dict(clip_values_det_limits=True, add_non_linear=False)
    f32 = frames(v, np.float32, over=over)
    u16 = frames(v, np.uint16, over=over)
    at_limit = f32 >= 77000.0
    assert int(at_limit.sum()) > 100
    assert (u16[at_limit] == 65535).all()
    assert int((u16 != quantised(f32)).sum()) == 0


def test_uint16_reads_against_the_oracle():
    # deterministic configuration (tests/test_modes_gpu.py): replay thrower, no random stage -- the oracle's float64
    # reads, clipped to the ADC's range, against the device's uint16 ones: half a count of rounding + T1
    v = helpers.make_visit("tiny128")
    kw = v.frame_kwargs(0, **OFF)
    pg = helpers.product_generator(v, 0)
    eo = helpers.oracle_generator(v)
    N = v.detector.light_sensitive_size(v.SUBARRAY)
    exp = pg.scanning_frame(threads=2, rng_mode=_lib.RNG_REPLAY, out_dtype=np.uint16, **kw)
    got = np.stack([r[0] for r in exp.reads])
    assert got.dtype == np.uint16
    want = np.stack(eo.scanning_frame(threads=2, draws=wo.PhiloxDraws(v.seed, 0, N), thrower="oracle",
                                      **helpers.oracle_kwargs(kw)))
    assert want.shape == got.shape and want[-1].max() - want[0].max() > 20.0      # the spectrum is on the frame, far above the bound
    d = np.abs(got.astype(np.float64) - np.clip(want, 0.0, 65535.0))
    print("uint16 vs oracle: max |d| = %.4f, bound 0.52 + 2e-7 |oracle|" % d.max())
    assert (d <= 0.5 + 0.02 + 2e-7 * np.abs(want)).all()


def test_delivery_on_alternating_slots_and_per_upload_buffer_sizing():
    v = helpers.make_visit("tiny128", n_exposures=3)
    eng = engine_of(v)
    ctx = eng.ctx
    S = v.detector.full_size(v.SUBARRAY)

    def desc(i, out_dtype):
        return helpers.product_generator(v, i).build_descriptor(eng, out_dtype=out_dtype, **v.frame_kwargs(i))

    want = [ctx.synthesize(desc(i, np.uint16)).copy() for i in range(3)]
    want32 = ctx.synthesize(desc(0, np.float32)).copy()
    assert all(w.dtype == np.uint16 and w.shape == (v.NSAMP, S, S) for w in want)
    assert (want[0] != want[1]).any()
    # upload / run / fetch_async on two alternating slots, each collected one exposure later
    got, pending = {}, None
    for i in range(3):
        slot = i % 2
        ctx.upload(slot, desc(i, np.uint16))
        ctx.run(slot)
        ctx.fetch_async(slot)
        if pending is not None:
            got[pending[0]] = np.array(ctx.wait(pending[1]))
        pending = (i, slot)
    view = ctx.wait(pending[1])
    assert view.dtype == np.uint16 and view.shape == (v.NSAMP, S, S)
    got[pending[0]] = np.array(view)
    np.testing.assert_array_equal(ctx.download(pending[1]), got[pending[0]])
    for i in range(3):
        np.testing.assert_array_equal(got[i], want[i])
    # one slot as uint16, float32, uint16 again: the dtype and the size follow the upload
    for out_dtype, ref in ((np.uint16, want[0]), (np.float32, want32), (np.uint16, want[0])):
        ctx.upload(2, desc(0, out_dtype))
        ctx.run(2)
        a = ctx.download(2)
        ctx.fetch_async(2)
        b = np.array(ctx.wait(2))
        assert a.dtype == b.dtype == np.dtype(out_dtype)
        np.testing.assert_array_equal(a, ref)
        np.testing.assert_array_equal(b, ref)
    # both read types at once: refused at upload, and the context goes on working
    d = desc(0, np.uint16)
    d.flags |= _lib.F_OUT_F64
    with pytest.raises(_lib.WayneError) as e:
        ctx.upload(2, d)
    assert e.value.status == _lib.E_INVALID and "OUT_U16" in str(e.value)
    np.testing.assert_array_equal(ctx.synthesize(desc(1, np.uint16)), want[1])


def test_an_exposure_run_a_second_time_gives_the_same_uint16_frame():
    # status bit 1 (a bin beyond the launch sequence's reach; knob lane_reach as in tests/test_soak_gpu.py): the general
    # sequence runs when the batch is synchronised, into the same uint16 buffer
    v = helpers.make_visit("small256")
    eng = engine_of(v)
    ctx = eng.ctx
    desc = helpers.product_generator(v, 0).build_descriptor(eng, out_dtype=np.uint16, **v.frame_kwargs(0))
    ctx.upload(0, desc)
    ctx.run_checked(0)
    want = ctx.download(0).copy()
    assert want.dtype == np.uint16 and want[-1].max() > 5000
    _lib.set_knob_all("lane_reach", "5")
    try:
        n0 = ctx.reruns
        ctx.upload(4, desc)
        ctx.run(4)
        ctx.synchronize()
        assert ctx.reruns == n0 + 1 and ctx.status(4) == 0
        via_sync = ctx.download(4).copy()
        assert ctx.reruns == n0 + 1
        ctx.upload(5, desc)
        ctx.run_checked(5)
        assert ctx.reruns == n0 + 2
        via_checked = ctx.download(5).copy()
    finally:
        _lib.set_knob_all("lane_reach", None)
    np.testing.assert_array_equal(via_sync, want)
    np.testing.assert_array_equal(via_checked, want)


def visit_files(outdir, names):
    out = {}
    for n in names:
        h = fitsio.read(os.path.join(outdir, n))
        cards = [c for c in h[0].header.cards if c[0] not in ("DATE", "SIM-TIME")]
        out[n] = (cards, [x for x in h if x.name == "SCI"], os.path.getsize(os.path.join(outdir, n)))
    return out


def test_a_visit_with_uint16_reads(tmp_path):
    names = ["0001_raw.fits", "0002_raw.fits"]
    seen = {}
    for streams in (2, 1):
        engine.close_all()
        _lib.set_knob_all("streams", streams)
        work = str(tmp_path / ("visit%d" % streams))
        shutil.copytree(MINI, work)
        yml = os.path.join(work, "params.yml")
        obs = run_visit.run(["-p", yml, "--max-exposures", "2"])
        floats = visit_files(obs.outdir, names)
        stamp = {n: os.stat(os.path.join(obs.outdir, n)).st_mtime_ns for n in names}
        # the float files are not this visit's once it asks for uint16 reads: both regenerated
        obs = run_visit.run(["-p", yml, "--max-exposures", "2", "--uint16-reads", "--resume"])
        assert obs.skipped == []
        ints = visit_files(obs.outdir, names)
        for n in names:
            assert os.stat(os.path.join(obs.outdir, n)).st_mtime_ns != stamp[n]
            cards_f, sci_f, size_f = floats[n]
            cards_i, sci_i, size_i = ints[n]
            assert cards_i == cards_f                                     # the primary header but for DATE / SIM-TIME
            assert len(sci_i) == len(sci_f) == 4 and size_f - size_i >= 4 * 138 * 138 * 6 - 4 * 2880     # 2 bytes a sample, not 8
            for a, b in zip(sci_i, sci_f):
                assert (a.header["BITPIX"], a.header["BSCALE"], a.header["BZERO"]) == (16, 1, 32768)
                assert b.header["BITPIX"] == -64 and a.header["SAMPNUM"] == b.header["SAMPNUM"]
                assert a.data.dtype == np.uint16 and a.data.shape == (138, 138)
                # (the default float32 reads go into the float64 images exactly)
                np.testing.assert_array_equal(a.data, np.clip(np.rint(b.data), 0, 65535).astype(np.uint16))
        if streams == 2:
            stamp = {n: os.stat(os.path.join(obs.outdir, n)).st_mtime_ns for n in names}
            obs = run_visit.run(["-p", yml, "--max-exposures", "2", "--uint16-reads", "--resume"])
            assert obs.skipped == [0, 1]
            assert all(os.stat(os.path.join(obs.outdir, n)).st_mtime_ns == stamp[n] for n in names)
            # ... and back: the uint16 files are not a float visit's
            obs = run_visit.run(["-p", yml, "--max-exposures", "2", "--resume"])
            assert obs.skipped == []
        seen[streams] = ints
    engine.close_all()
    for n in names:                                                       # whichever stream carried the exposures
        assert seen[1][n][0] == seen[2][n][0]
        for a, b in zip(seen[1][n][1], seen[2][n][1]):
            np.testing.assert_array_equal(a.data, b.data)
