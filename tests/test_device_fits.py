"""CPU: the host half of the device-side FITS words (--device-fits) -- the layout function against tests/fits_words_law.py,
the Exposure's stored-words path against its array path byte for byte, the lease of fits_delivery.FitsDelivery against a
fake context, the refusal beside --spectra-only and the digest guard of a descriptor without the option.
The device side: tests/test_device_fits_gpu.py."""
import os
import threading

import numpy as np
import pytest
import yaml

import fits_words_law as law
from fits_words_law import clock_free
from wayne_amd import _lib, calibration, detector, exposure, fits_delivery, fitsio, grism, run_visit, visit
from wayne_amd.exposure_generator import ExposureGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
# visit.descriptor_digest of the mini visit's first descriptor, as tests/test_traps_cpu.py records it
DIGEST_TODAY = "ada2f5427249538616a40b32d67ff4f78fd7aab0"
DTYPES = (np.float32, np.float64, np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_function_equals_the_law(dtype):
    for S in (74, 138, 266, 1024, 522):
        for R in (1, 2, 15):
            got = _lib.fits_layout(S, R, dtype)
            assert got == law.layout(S, R, dtype), (S, R, dtype)
            plane_bytes, stride, bitpix = got
            assert stride % 2880 == 0 and stride % 64 == 0 and 0 <= stride - plane_bytes < 2880
            # the flag word of a descriptor names the type the same way; its other bits do not matter
            assert _lib.fits_layout(S, R, _lib.OUT_FLAGS[np.dtype(dtype)] | _lib.F_ADD_DARK | _lib.F_EXACT_SAMPLERS) == got
    assert law.layout(74, 3, np.uint16)[0] % 16 == 8          # the half vector of every sub-array side
    assert law.layout(1024, 15, np.uint16)[0] % 16 == 0       # ... and none at 1024


def test_layout_function_refuses_what_has_no_layout():
    for S, R, flags in ((74, 3, _lib.F_OUT_F64 | _lib.F_OUT_U16), (75, 3, 0), (0, 3, 0), (74, 0, 0)):
        with pytest.raises(_lib.WayneError) as e:
            _lib.fits_layout(S, R, flags)
        assert e.value.status == _lib.E_INVALID
    with pytest.raises(KeyError):
        _lib.fits_layout(74, 3, np.int32)


def made_up_reads(dtype, S=74, n=4, seed=3):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint16:
        reads = rng.integers(0, 65536, (n, S, S)).astype(np.uint16)
        reads[0, 0, :6] = [0, 1, 32767, 32768, 65534, 65535]
        reads[-1, -1, -3:] = [65535, 0, 32768]
        return reads
    reads = rng.normal(2000.0, 900.0, (n, S, S)).astype(dtype)
    tiny = np.finfo(np.float32).tiny
    special = [-20.5, 0.0, -0.0, 65535.0, tiny / 2, -tiny / 4, np.float32(1e-45), np.inf, -np.inf, 78000.25]
    reads[0, 0, :len(special)] = special
    reads[-1, -1, -len(special):] = special[::-1]
    reads[1, 5, 7] = -0.0
    return reads


def exposure_for(info_of):
    cal = calibration.CalibrationSet.synthetic(11)
    det, gr = detector.WFC3_IR(), grism.G141(cal)
    eg = ExposureGenerator(det, gr, 4, "RAPID", 64, None, "0003_raw.fits", 2456196.25, calibration=cal, seed=77)
    # (the clock's SIM-TIME fixed, as tests/test_visit_driver.py does)
    info = dict(eg.exp_info, x_ref=401.5, y_ref=399.0, samp_rate=25.0, SCAN=True, SCAN_DIR=1, sim_time=0.002, **info_of)
    return exposure.Exposure(det, gr, None, info), det.get_read_times(4, 64, "RAPID")


@pytest.mark.parametrize("dtype", DTYPES)
def test_stored_pieces_write_the_bytes_of_the_array_path(tmp_path, dtype):
    S = 74
    reads = made_up_reads(dtype, S)
    plane_bytes, stride, bitpix = law.layout(S, 3, dtype)
    assert plane_bytes % 2880 != 0                      # the padding is part of the comparison

    def info(r, t):
        return {"cumulative_exp_time": float(t[r - 1]) if r else 0.0,
                "read_exp_time": float(t[r - 1] - (t[r - 2] if r > 1 else 0.0)) if r else 0.0, "CRPIX1": 0}

    by_array, t = exposure_for({})
    for r in range(4):
        by_array.add_read(reads[r], info(r, t))
    os.makedirs(str(tmp_path / "a"))
    a = by_array.generate_fits(str(tmp_path / "a"), "0003_raw.fits")

    payload = law.payload(reads)
    pieces = fits_delivery.stored_pieces(payload, (plane_bytes, stride, bitpix), 4)
    assert all(len(p) == stride for p in pieces)
    stored, _ = exposure_for({})
    code = "u2" if np.dtype(dtype) == np.uint16 else "f8"
    for r in range(4):
        stored.add_stored_read(pieces[3 - r], info(r, t), (S, S), code)        # plane f holds read 3 - f
    os.makedirs(str(tmp_path / "b"))
    b = stored.generate_fits(str(tmp_path / "b"), "0003_raw.fits")
    raw_a, raw_b = open(a, "rb").read(), open(b, "rb").read()
    assert len(raw_a) == len(raw_b) and len(raw_a) % 2880 == 0
    assert clock_free(raw_a) == clock_free(raw_b)
    # and the file reads back as the reads (the comparison above is not one of two empty files)
    sci = [h for h in fitsio.read(b) if h.name == "SCI"]
    assert [h.header["SAMPNUM"] for h in sci] == [3, 2, 1, 0]
    for h in sci:
        want = reads[h.header["SAMPNUM"]]
        np.testing.assert_array_equal(np.asarray(h.data), want if code == "u2" else want.astype(np.float64))
    # a piece of the wrong length, or both kinds of read in one exposure, are refused
    with pytest.raises(ValueError):
        stored.add_stored_read(pieces[0][:-1], info(0, t), (S, S), code)
    mixed, _ = exposure_for({})
    mixed.add_read(reads[0], info(0, t))
    mixed.add_stored_read(pieces[3], info(0, t), (S, S), code)
    with pytest.raises(ValueError):
        mixed.generate_fits(str(tmp_path / "b"), "mixed.fits")


class FakeContext(object):
    def __init__(self, log):
        self.log = log

    def upload(self, slot, desc):
        self.log.append(("upload", slot))


class SignallingCondition(threading.Condition):
    """A Condition that tells when a thread has gone to sleep in it."""

    def __init__(self):
        threading.Condition.__init__(self)
        self.asleep = threading.Event()

    def wait(self, timeout=None):
        self.asleep.set()
        return threading.Condition.wait(self, timeout)


class GatedExposure(object):
    """What a writer thread is handed: generate_fits blocks until the gate opens, then writes -- or fails."""

    def __init__(self, log, gate, fail=False):
        self.log, self.gate, self.fail = log, gate, fail

    def generate_fits(self, out_dir, filename):
        assert self.gate.wait(60)
        if self.fail:
            self.log.append("failed")
            raise OSError("no space left on device (made up)")
        self.log.append("written")


@pytest.mark.parametrize("fail", [False, True])
def test_upload_waits_for_the_file_written_from_the_slot(fail):
    log, gate = [], threading.Event()
    d = fits_delivery.FitsDelivery(FakeContext(log))
    d._cv = SignallingCondition()
    d._last = 0                                        # (what wait(0) notes)
    pool = exposure.FitsWriterPool(threads=1)
    release = d.lease()
    assert d.leased(0) and not d.leased(1)

    def done():
        log.append("released")
        release()

    pool.submit(GatedExposure(log, gate, fail), "nowhere", "0001_raw.fits", done=done)
    uploader = threading.Thread(target=d.upload, args=(0, "desc"), daemon=True)
    uploader.start()
    assert d._cv.asleep.wait(60)                       # the upload into the pending slot is held ...
    assert uploader.is_alive() and ("upload", 0) not in log
    d.upload(1, "desc")                                # ... one into another slot is not
    assert log == [("upload", 1)]
    gate.set()
    uploader.join(60)
    assert not uploader.is_alive() and not d.leased(0)
    # the writer's outcome, then the release, and only then the upload
    assert log == [("upload", 1), "failed" if fail else "written", "released", ("upload", 0)]
    if fail:
        with pytest.raises(OSError):
            pool.close()
    else:
        pool.close()


def test_slot_count_of_the_loop():
    for depth in (3, 4):
        for writers in (1, 2, 4, 16, 64):
            n = fits_delivery.slots_for(depth, writers)
            assert n % 2 == 0 and depth + min(writers, 28) <= n <= 32, (depth, writers, n)
    assert fits_delivery.slots_for(4, 1) == 6 and fits_delivery.slots_for(4, 16) == 20


def test_refused_beside_spectra_only(tmp_path):
    yml = os.path.join(MINI, "params.yml")
    with pytest.raises(ValueError, match="spectra-only"):
        run_visit.run(["-p", yml, "--device-fits", "--spectra-only", str(tmp_path / "s.npz")])
    obs = run_visit.build_observation(yaml.safe_load(open(yml)), base_dir=MINI)
    obs.frame_options.update(extraction=True, device_fits=True)
    obs.spectra_only, obs.spectra_out = True, str(tmp_path / "s.npz")
    with pytest.raises(ValueError, match="spectra_only"):
        obs.run_observation()
    assert not os.path.exists(str(tmp_path / "s.npz"))


def _descriptor(obs, **kw):
    gen = ExposureGenerator(obs.detector, obs.grism, obs.NSAMP, obs.SAMPSEQ, obs.SUBARRAY, calibration=obs.calibration,
                            seed=obs.seed, exposure_index=0)
    _, mid, dur, ri = gen._gen_scanning_sample_times(obs.sample_rate)
    return gen.build_descriptor(None, float(obs.x_ref[0]), float(obs.y_ref[0]), 0.0, 0.0, obs.wl, obs.stellar_flux, None,
                                obs.scan_speed, obs.sample_rate, mid, dur, ri, **kw)


def test_a_descriptor_without_the_option_is_todays():
    obs = run_visit.build_observation(yaml.safe_load(open(os.path.join(MINI, "params.yml"))), base_dir=MINI)
    d = _descriptor(obs)
    assert d._device_fits is False
    assert visit.descriptor_digest(d) == DIGEST_TODAY
    # the option asks the device for one more product of the same reads: what the descriptor hands over is the same
    on = _descriptor(obs, device_fits=True)
    assert on._device_fits is True
    assert visit.descriptor_digest(on) == DIGEST_TODAY
    assert on.flags == d.flags
