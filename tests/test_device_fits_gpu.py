"""GPU: device-side FITS words (wayne_exposure_set_fits, k_fits_words, --device-fits).

The law (tests/fits_words_law.py, tolerance 0): the payload of a slot is, plane by plane and the last read first, the
big-endian FITS words of the slot's own reads, each plane padded with zeros to the 2880-byte block.  Everything here
compares bytes with `==`: the payload against the law applied to the reads the same slot delivers, and the files of a
visit written from pinned memory against the files the host path writes.  Host side: tests/test_device_fits.py."""
import os
import shutil

import numpy as np
import pytest
import yaml

import fits_words_law as law
import helpers
from fits_words_law import clock_free
from wayne_amd import _lib, engine, fitsio, run_visit, visit as wv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
DTYPES = (np.float32, np.float64, np.uint16)


def engine_of(v):
    return engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def descriptor(v, eng, out_dtype, i=0, staring=False, **opts):
    pg = helpers.product_generator(v, i)
    kw = v.frame_kwargs(i)
    if staring:
        kw = {k: kw[k] for k in kw if k not in ("scan_speed", "sample_rate", "ssv_generator")}
        return pg.prepare(staring=True, out_dtype=out_dtype, **opts, **kw)._prepared[1]
    return pg.build_descriptor(eng, out_dtype=out_dtype, **opts, **kw)


PARITY = {"tiny": False, "tiny_g102": False, "tiny128": False, "small256": False, "stare256": True}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", list(PARITY))
def test_payload_is_the_law_on_the_slots_own_reads(name, dtype):
    v = helpers.make_visit(name)
    eng = engine_of(v)
    ctx = eng.ctx
    S = v.detector.full_size(v.SUBARRAY)
    R = v.NSAMP - 1
    # the slot first with another sample type, of another word size: this run's planes and padding then land on the
    # stale words of another stride
    other = np.float32 if np.dtype(dtype) == np.uint16 else np.uint16
    slot = 6
    # (... and before that once with the type itself, so that the buffer has its size already and the other type's words
    # are not lost to a fresh allocation)
    ctx.upload(slot, descriptor(v, eng, dtype, staring=PARITY[name], device_fits=True))
    ctx.run_checked(slot)
    ctx.upload(slot, descriptor(v, eng, other, staring=PARITY[name], device_fits=True))
    assert ctx.has_fits(slot)
    ctx.run_checked(slot)
    stale = ctx.download_fits(slot)
    assert stale.size == (R + 1) * law.layout(S, R, other)[1]
    ctx.upload(slot, descriptor(v, eng, dtype, staring=PARITY[name], device_fits=True))
    assert ctx.fits_layout_of(slot) == law.layout(S, R, dtype) == _lib.fits_layout(S, R, dtype)
    ctx.run_checked(slot)
    reads = ctx.download(slot)
    got = ctx.download_fits(slot)
    assert reads.dtype == np.dtype(dtype) and reads.shape == (R + 1, S, S) and np.isfinite(reads.astype(np.float64)).all()
    want = law.payload(reads)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d bytes differ, the first at %d" % (bad.size, want.size, bad[0])
    # what the comparison covers: padding bytes, a star in the last read that the zero read does not hold (so the order
    # of the planes matters), and at S = 74 a half vector of uint16 samples and a partial last workgroup
    plane_bytes, stride, _ = law.layout(S, R, dtype)
    assert stride > plane_bytes and float(reads[-1].astype(np.float64).sum()) != float(reads[0].astype(np.float64).sum())
    if name == "tiny":
        assert S * S == 5476 and S * S % 8 == 4
    last, pad = law.plane_of(got, 0, S, dtype)
    np.testing.assert_array_equal(last, reads[-1].astype(last.dtype))
    assert not pad.any()


def test_a_second_run_delivers_its_own_words():
    # status bit 1 (a bin beyond the launch sequence's reach; knob lane_reach as in tests/test_uint16_reads_gpu.py):
    # wait_fits runs the exposure again with the general sequence and fetches the payload -- and the reads fetched
    # beside it -- a second time
    v = helpers.make_visit("small256")
    eng = engine_of(v)
    ctx = eng.ctx
    desc = descriptor(v, eng, np.float32, device_fits=True)
    ctx.upload(0, desc)
    ctx.run_checked(0)
    want_reads = ctx.download(0).copy()
    _lib.set_knob_all("lane_reach", "5")
    try:
        n0 = ctx.reruns
        ctx.upload(4, desc)
        ctx.run(4)
        ctx.fetch_async(4)
        ctx.fetch_fits_async(4)
        payload = ctx.wait_fits(4)
        assert ctx.reruns == n0 + 1
        reads = ctx.wait(4)
        assert ctx.reruns == n0 + 1 and ctx.status(4) == 0
        assert payload.dtype == np.uint8 and (payload == law.payload(reads)).all()
        np.testing.assert_array_equal(reads, want_reads)
        # without the reads: the payload alone
        ctx.upload(5, desc)
        ctx.run(5)
        ctx.fetch_fits_async(5)
        alone = ctx.wait_fits(5)
        assert ctx.reruns == n0 + 2
        assert (alone == law.payload(want_reads)).all()
    finally:
        _lib.set_knob_all("lane_reach", None)


def raw_files(out_dir):
    names = sorted(n for n in os.listdir(out_dir) if n.endswith("_raw.fits"))
    return {n: clock_free(open(os.path.join(out_dir, n), "rb").read()) for n in names}


def same_files(a, b, n):
    assert sorted(a) == sorted(b) == ["%04d_raw.fits" % (i + 1) for i in range(n)]
    for name in a:
        assert len(a[name]) == len(b[name]) and a[name] == b[name], name        # every header, every data section


VISIT_CASES = {
    "float32": dict(out_dtype=np.float32),
    "uint16": dict(out_dtype=np.uint16),
    "extraction": dict(out_dtype=np.float32, extraction=True),
}


@pytest.mark.parametrize("case", list(VISIT_CASES))
def test_a_visit_writes_the_same_files_from_pinned_memory(tmp_path, monkeypatch, case):
    opts = dict(VISIT_CASES[case])
    extraction = opts.pop("extraction", None)
    n = 6
    v = helpers.make_visit("tiny128", n_exposures=n)

    def run(out, device_fits):
        spectra = {}
        runner = wv.VisitRunner(v, 0, out_dir=str(tmp_path / out), device_fits=device_fits, **opts)
        kw = {}
        if extraction is not None:
            kw = dict(extraction=extraction, on_spectra=lambda i, sp, sk: spectra.__setitem__(i, (sp.copy(), sk.copy())))
        assert runner.run(range(n), **kw) == {}
        return raw_files(str(tmp_path / out)), spectra

    monkeypatch.setenv("WAYNE_FITS_THREADS", "4")
    want, want_spectra = run("host", False)
    assert len(want) == n and len(set(want.values())) == n
    for streams in (2, 1):
        for threads in (1, 4):
            monkeypatch.setenv("WAYNE_FITS_THREADS", str(threads))      # (read when the run makes its writer pool)
            _lib.set_knob_all("streams", streams)
            got, got_spectra = run("dev_s%d_t%d" % (streams, threads), True)
            same_files(got, want, n)
            assert sorted(got_spectra) == sorted(want_spectra)
            for i in want_spectra:
                np.testing.assert_array_equal(got_spectra[i][0], want_spectra[i][0])
                np.testing.assert_array_equal(got_spectra[i][1], want_spectra[i][1])
    # keep=True and on_reads still get the reads (they are then fetched beside the payload)
    _lib.set_knob_all("streams", None)
    seen = {}
    runner = wv.VisitRunner(v, 0, out_dir=str(tmp_path / "kept"), device_fits=True, **opts)
    kw = dict(extraction=extraction) if extraction is not None else {}
    kept = runner.run(range(2), keep=True, on_reads=lambda i, r: seen.__setitem__(i, r.copy()), **kw)
    for i in range(2):
        reads = kept[i][0] if extraction is not None else kept[i]
        np.testing.assert_array_equal(reads, seen[i])
        sci = [h for h in fitsio.read(os.path.join(str(tmp_path / "kept"), "%04d_raw.fits" % (i + 1))) if h.name == "SCI"]
        np.testing.assert_array_equal(np.asarray(sci[0].data), reads[-1].astype(sci[0].data.dtype))
    same_files(raw_files(str(tmp_path / "kept")), {k: want[k] for k in sorted(want)[:2]}, 2)


def mini_observation(out_dir, n, device_fits, traps=None):
    cfg = yaml.safe_load(open(os.path.join(MINI, "params.yml")))
    if traps is not None:
        cfg["charge_traps"] = traps
    obs = run_visit.build_observation(cfg, base_dir=MINI)
    obs.outdir = out_dir
    obs.exp_start_times = obs.exp_start_times[:n]
    if device_fits:
        obs.frame_options["device_fits"] = True
    return obs


def test_a_carried_trap_history_writes_the_same_files(tmp_path, monkeypatch):
    traps = {"history": "carried", "slow": {"initial": 200.0, "orbit_fill": 100.0}, "fast": {"initial": 30.0}}
    n = 6
    monkeypatch.setenv("WAYNE_FITS_THREADS", "4")
    host = mini_observation(str(tmp_path / "host"), n, False, traps)
    host.run_observation()
    want = raw_files(host.outdir)
    state = host.trap_state.copy()
    for streams, threads in ((2, 1), (1, 4)):
        monkeypatch.setenv("WAYNE_FITS_THREADS", str(threads))
        _lib.set_knob_all("streams", streams)
        dev = mini_observation(str(tmp_path / ("dev%d" % streams)), n, True, traps)
        dev.run_observation()
        same_files(raw_files(dev.outdir), want, n)
        np.testing.assert_array_equal(dev.trap_state.view(np.uint32), state.view(np.uint32))
    engine.close_all()


def test_cli_writes_the_same_files_and_resumes(tmp_path):
    n = 4
    names = ["%04d_raw.fits" % (i + 1) for i in range(n)]
    outs = {}
    for flag in ((), ("--device-fits",)):
        work = str(tmp_path / ("visit%d" % len(flag)))
        shutil.copytree(MINI, work)
        yml = os.path.join(work, "params.yml")
        obs = run_visit.run(["-p", yml, "--max-exposures", str(n)] + list(flag))
        outs[flag] = (obs.outdir, yml)
    host, dev = raw_files(outs[()][0]), raw_files(outs[("--device-fits",)][0])
    same_files(dev, host, n)
    # the direct image is the host path's either way
    assert open(os.path.join(outs[()][0], "0000_flt.fits"), "rb").read()[2880:] == \
        open(os.path.join(outs[("--device-fits",)][0], "0000_flt.fits"), "rb").read()[2880:]
    # --resume: the files are the host path's, so a whole one is recognised and only the deleted one is made again
    out, yml = outs[("--device-fits",)]
    stamp = {m: os.stat(os.path.join(out, m)).st_mtime_ns for m in names}
    os.remove(os.path.join(out, names[2]))
    obs = run_visit.run(["-p", yml, "--max-exposures", str(n), "--device-fits", "--resume"])
    assert obs.skipped == [0, 1, 3]
    for m in names:
        assert (os.stat(os.path.join(out, m)).st_mtime_ns == stamp[m]) == (m != names[2])
    same_files(raw_files(out), host, n)
    engine.close_all()


def test_off_means_off():
    v = helpers.make_visit("tiny128")
    eng = engine_of(v)
    ctx = eng.ctx
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        ctx.upload(2, descriptor(v, eng, np.float32, device_fits=True))
        ctx.run_checked(2)
        assert ctx.fits_profile()["launches"] == 1
        # the same slot again, uploaded without the option: no k_fits_words, nothing to fetch
        ctx.upload(2, descriptor(v, eng, np.float32))
        assert not ctx.has_fits(2)
        ctx.run_checked(2)
        assert ctx.fits_profile()["launches"] == 1
        for call in (ctx.fetch_fits_async, ctx.wait_fits, ctx.download_fits):
            with pytest.raises(_lib.WayneError) as e:
                call(2)
            assert e.value.status == _lib.E_STATE
        # a slot that was never uploaded
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_fits(200)
        assert e.value.status == _lib.E_STATE
        # set_fits(on=False) clears it too, and the reads are those of a slot that never had it
        ctx.upload(3, descriptor(v, eng, np.float32, device_fits=True))
        ctx.set_fits(3, False)
        ctx.run_checked(3)
        assert ctx.fits_profile()["launches"] == 1
        np.testing.assert_array_equal(ctx.download(3), ctx.download(2))
    finally:
        ctx.profile_enable(False)
