"""GPU: device-side spectral extraction (wayne_exposure_set_extraction, k_extract; wayne_amd/extraction.py).

The oracle in every case is the law restated in numpy (tests/extraction_law.py) applied to the reads of the SAME slot,
fetched with `download`: the device's spectra may differ from it only by the order of their float64 row sums, 1e-9 of
M[x] per column (the derivation: extraction_law's docstring).  Host side: tests/test_extraction.py."""
import os
import shutil

import numpy as np
import pytest

import extraction_law as law
import helpers
import visit_science as vs
from wayne_amd import _lib, engine, extraction, run_visit
from wayne_amd.visit import VisitRunner

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "fixtures", "mini_visit")
_visits, _planes = {}, {}


def visit(name, n=1):
    if (name, n) not in _visits:
        _visits[(name, n)] = helpers.make_visit(name, n_exposures=n)
    return _visits[(name, n)]


def planes(v):
    if v.name not in _planes:
        _planes[v.name] = law.Planes(v)
    return _planes[v.name]


def engine_of(v):
    return engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


def descriptor(v, i, ex, out_dtype=np.float32, **over):
    eng = engine_of(v)
    gen = helpers.product_generator(v, i)
    return gen.build_descriptor(eng, out_dtype=out_dtype, extraction=ex, **v.frame_kwargs(i, **over)), gen


def extracted(v, i, ex, out_dtype=np.float32, slot=0, **over):
    """(reads, spectra, sky, the exposure's plan) of exposure i run in `slot` with extraction `ex`."""
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(slot, desc)
    ctx.run(slot)
    reads = ctx.download(slot)
    spectra, sky = ctx.download_spectra(slot)
    assert reads.dtype == np.dtype(out_dtype)
    return reads, spectra, sky, gen.extraction_plan


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("name", ["tiny", "small256", "stare256", "cfg3", "cfg4"])
def test_spectra_are_the_law_applied_to_the_slots_reads(name, out_dtype):
    v = visit(name)
    # (tiny's scan stays inside the frame under the default margin: a wider one sends its windows to both clamps)
    ex = extraction.ExtractionOptions(margin=40) if name == "tiny" else True
    reads, spectra, sky, plan = extracted(v, 0, ex, out_dtype)
    R, S = v.NSAMP - 1, planes(v).S
    assert spectra.shape == (R + 1, S) and sky.shape == (R + 1,) and plan.row_windows.shape == (R + 1, 2)
    if name == "tiny":
        # S = 74: a second column tile of 10 columns; windows clamped at both borders
        assert S == 74 and plan.row_windows[:, 0].min() == 5 and plan.row_windows[:, 1].max() == S - 5
    if name == "cfg4":
        assert S == 1024 and R == 15 and plan.row_windows[R, 1] - plan.row_windows[R, 0] > 20 * 32     # many chunks
    want, _, M = law.assert_parity(spectra, sky, reads, planes(v), plan.row_windows, plan.bg_cols,
                                   what="%s %s" % (name, np.dtype(out_dtype).name))
    assert (M[:, 40:60].sum(axis=1) > 0).all() and np.abs(want).max() > 0


def test_hand_made_windows():
    # one row; a window that ends exactly at S - 5; three chunks of 32 rows and a remainder of 7; the whole frame
    v = visit("small256")
    S = 266
    for windows in ([(100, 101), (200, S - 5), (5, 5 + 3 * 32 + 7), (0, S)],
                    [(S - 1, S), (0, 1), (31, 65), (5, S - 5)]):
        ex = extraction.Extraction(windows, bg_cols=(0, S))
        reads, spectra, sky, _ = extracted(v, 0, ex)
        law.assert_parity(spectra, sky, reads, planes(v), windows, (0, S), what="windows %s" % (windows,))
    ex = extraction.Extraction([(100, 101)] * 4, bg_cols=(265, 266))         # one row, one background column
    reads, spectra, sky, _ = extracted(v, 0, ex)
    law.assert_parity(spectra, sky, reads, planes(v), [(100, 101)] * 4, (265, 266), what="one row, one column")


def test_channel_fluxes_from_device_spectra_are_the_observers():
    sv = vs.ScienceVisit("cfg3", 2)
    v, R = sv.v, sv.R
    pl = law.Planes(v)
    t = np.concatenate([[0.0], sv.read_times])
    for i in range(2):
        windows = [sv.row_window(i, t[r], t[r + 1]) for r in range(R)] + [sv.row_window(i, 0.0, t[-1])]
        ex = extraction.Extraction(windows, bg_cols=vs.BG_COLS)
        reads, spectra, sky, _ = extracted(v, i, ex, **sv.frame_overrides)
        ramp, last = sv.extract(i, reads)
        _, _, M, _ = law.restate(reads, pl, windows, vs.BG_COLS)
        cw = extraction.channel_weights(v.x_refs[i], sv.edges, sv.sub_scale, sv.S)
        got_ramp, got_last = cw @ spectra[:R].sum(axis=0), cw @ spectra[R]
        err_ramp = np.abs(got_ramp - ramp) / (cw @ M[:R].sum(axis=0))
        err_last = np.abs(got_last - last) / (cw @ M[R])
        print("exposure %d: channel flux error / sum M: ramp %.3g, last read %.3g" % (i, err_ramp.max(), err_last.max()))
        assert err_ramp.max() <= 1e-9 and err_last.max() <= 1e-9
        assert ramp.min() > 1e5                                      # (there is a spectrum in every channel)


@pytest.mark.parametrize("off", ["LINEARISE", "DARK", "GAIN", "SKY", "LAST_READ"])
def test_each_step_can_be_switched_off(off):
    v = visit("small256")
    steps = extraction.ALL & ~getattr(extraction, off)
    reads, spectra, sky, plan = extracted(v, 0, extraction.ExtractionOptions(steps=steps))
    want, _, _ = law.assert_parity(spectra, sky, reads, planes(v), plan.row_windows, plan.bg_cols, steps, what="no " + off)
    full, _, _, _ = law.restate(reads, planes(v), plan.row_windows, plan.bg_cols)
    assert np.abs(want - full).max() > 1.0                           # the step matters on this exposure
    if off == "SKY":
        assert (sky == 0.0).all()
    if off == "LAST_READ":
        assert (spectra[-1] == 0.0).all() and sky[-1] == 0.0 and (sky[:-1] != 0.0).all()


def test_the_same_exposure_gives_the_same_bytes_in_any_slot_and_after_other_work():
    v = visit("small256", 3)
    ctx = engine_of(v).ctx
    desc, _ = descriptor(v, 1, True)
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    a, a_sky = ctx.download_spectra(0)
    b, b_sky = ctx.download_spectra(1)
    assert a.tobytes() == b.tobytes() and a_sky.tobytes() == b_sky.tobytes() and np.abs(a).max() > 0
    for slot, i in ((0, 0), (1, 2), (2, 0)):                         # other exposures, with other plans, in between
        other, _ = descriptor(v, i, extraction.ExtractionOptions(margin=3 + slot, steps=extraction.ALL & ~extraction.DARK))
        ctx.upload(slot, other)
        ctx.run(slot)
    ctx.synchronize()
    ctx.upload(3, desc)
    ctx.run(3)
    c, c_sky = ctx.download_spectra(3)
    assert c.tobytes() == a.tobytes() and c_sky.tobytes() == a_sky.tobytes()


def test_an_exposure_run_a_second_time_is_extracted_a_second_time():
    # status bit 1 (knob lane_reach, as tests/test_uint16_reads_gpu.py): wait_spectra runs the general sequence, whose
    # back half extracts again, fetches again and hands over the spectra of the run without the knob
    v = visit("small256")
    ctx = engine_of(v).ctx
    desc, _ = descriptor(v, 0, True)
    ctx.upload(0, desc)
    ctx.run(0)
    want, want_sky = ctx.download_spectra(0)
    want_reads = ctx.download(0).copy()
    _lib.set_knob_all("lane_reach", "5")
    try:
        n0 = ctx.reruns
        ctx.upload(4, desc)
        ctx.run(4)
        ctx.fetch_spectra_async(4)
        got, got_sky = ctx.wait_spectra(4)
        got, got_sky = got.copy(), got_sky.copy()
        assert ctx.reruns == n0 + 1 and ctx.status(4) == 0
        # reads and spectra fetched side by side: one second run serves both
        ctx.upload(5, desc)
        ctx.run(5)
        ctx.fetch_async(5)
        ctx.fetch_spectra_async(5)
        reads = ctx.wait(5).copy()
        both, both_sky = ctx.wait_spectra(5)
        both, both_sky = both.copy(), both_sky.copy()
        assert ctx.reruns == n0 + 2
    finally:
        _lib.set_knob_all("lane_reach", None)
    assert got.tobytes() == want.tobytes() and got_sky.tobytes() == want_sky.tobytes()
    assert both.tobytes() == want.tobytes() and both_sky.tobytes() == want_sky.tobytes()
    np.testing.assert_array_equal(reads, want_reads)


def test_delivery():
    v = visit("small256")
    ctx = engine_of(v).ctx
    plain, _ = descriptor(v, 0, None)
    ctx.upload(2, plain)
    ctx.run(2)
    ctx.fetch_async(2)
    reads_without = ctx.wait(2).copy()
    for call in (ctx.fetch_spectra_async, ctx.wait_spectra, ctx.download_spectra):     # no extraction set
        with pytest.raises(_lib.WayneError) as e:
            call(2)
        assert e.value.status == _lib.E_STATE
    desc, gen = descriptor(v, 0, True)
    ctx.upload(2, desc)
    ctx.run(2)
    ctx.fetch_async(2)
    ctx.fetch_spectra_async(2)
    reads = ctx.wait(2).copy()
    spectra, sky = ctx.wait_spectra(2)
    spectra, sky = spectra.copy(), sky.copy()
    blocking, blocking_sky = ctx.download_spectra(2)
    assert spectra.tobytes() == blocking.tobytes() and sky.tobytes() == blocking_sky.tobytes()
    np.testing.assert_array_equal(reads, reads_without)                    # the reads do not know about the extraction
    np.testing.assert_array_equal(ctx.download(2), reads_without)
    law.assert_parity(spectra, sky, reads, planes(v), gen.extraction_plan.row_windows, (6, 26), what="delivery")
    # set_extraction(None) and upload both clear it
    ctx.set_extraction(2, None)
    with pytest.raises(_lib.WayneError) as e:
        ctx.fetch_spectra_async(2)
    assert e.value.status == _lib.E_STATE
    ctx.set_extraction(2, gen.extraction_plan)
    ctx.run(2)
    again, _ = ctx.download_spectra(2)
    assert again.tobytes() == spectra.tobytes()
    ctx.upload(2, plain)
    with pytest.raises(_lib.WayneError) as e:
        ctx.wait_spectra(2)
    assert e.value.status == _lib.E_STATE
    # a refused plan leaves the slot usable, without extraction; a slot that was never uploaded is a state error
    S = 266
    for bad in (extraction.Extraction([(5, 9), (9, 9), (5, 9), (5, 9)]), extraction.Extraction([(5, S + 1)] * 4),
                extraction.Extraction([(5, 9)] * 4, steps=32), extraction.Extraction([(5, 9)] * 4, bg_cols=(30, 30))):
        ctx.set_extraction(2, gen.extraction_plan)
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_extraction(2, bad)
        assert e.value.status == _lib.E_INVALID
        with pytest.raises(_lib.WayneError) as e:
            ctx.download_spectra(2)
        assert e.value.status == _lib.E_STATE
    ctx.set_extraction(2, extraction.Extraction([(5, 9)] * 3 + [(0, 0)], steps=extraction.ALL & ~extraction.LAST_READ))
    ctx.run(2)
    np.testing.assert_array_equal(ctx.download(2), reads_without)
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_extraction(200, gen.extraction_plan)
    assert e.value.status == _lib.E_STATE


def test_frames_carry_their_spectra():
    v = visit("stare256")
    kw = v.frame_kwargs(0)
    kw = {k: kw[k] for k in kw if k not in ("scan_speed", "sample_rate", "ssv_generator")}
    exp = helpers.product_generator(v, 0).staring_frame(extraction=True, **kw)
    reads = np.stack([r[0] for r in exp.reads])
    assert (exp.extraction.row_windows == exp.extraction.row_windows[0]).all()        # a staring exposure: one window
    law.assert_parity(exp.spectra, exp.sky, reads, planes(v), exp.extraction.row_windows, (6, 26), what="staring_frame")
    plain = helpers.product_generator(v, 0).staring_frame(**kw)
    assert not hasattr(plain, "spectra")
    np.testing.assert_array_equal(np.stack([r[0] for r in plain.reads]), reads)


def test_a_visit_delivers_spectra_without_its_reads():
    v = visit("tiny", 6)
    runner = VisitRunner(v)
    spectra, sky = runner.run_spectra(range(6))
    assert spectra.shape == (6, 4, 74) and sky.shape == (6, 4) and len(runner.plans) == 6
    for i in range(6):
        exp = helpers.product_generator(v, i).scanning_frame(extraction=True, **v.frame_kwargs(i))
        assert exp.spectra.tobytes() == spectra[i].tobytes() and exp.sky.tobytes() == sky[i].tobytes(), i
        np.testing.assert_array_equal(runner.plans[i].row_windows, exp.extraction.row_windows)
    # ... and with them: the same spectra beside the reads of a run without extraction
    seen = {}
    both = runner.run([1, 4], keep=True, extraction=True, on_spectra=lambda i, sp, sk: seen.setdefault(i, sp.copy()))
    plain = VisitRunner(v).run([1, 4], keep=True)
    for i in (1, 4):
        np.testing.assert_array_equal(both[i][0], plain[i])
        assert both[i][1].tobytes() == spectra[i].tobytes() == seen[i].tobytes() and both[i][2].tobytes() == sky[i].tobytes()


def test_cli_spectra_only_writes_the_npz_and_no_raw_file(tmp_path):
    work = str(tmp_path / "visit")
    shutil.copytree(MINI, work)
    yml = os.path.join(work, "params.yml")
    out = str(tmp_path / "spectra.npz")
    with pytest.raises(SystemExit):
        run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", out, "--resume"])
    obs = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", out])
    assert sorted(os.listdir(obs.outdir)) == ["0000_flt.fits", "params.yml", "visit_plan.txt"]
    z = np.load(out)
    assert sorted(z.files) == sorted(["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref",
                                      "read_times", "exp_start"])
    assert z["spectra"].shape == (3, 4, 138) and z["sky"].shape == (3, 4) and list(z["exposure_index"]) == [0, 1, 2]
    assert z["row_lo"].shape == z["row_hi"].shape == (3, 4) and list(z["bg_cols"]) == [6, 26]
    assert z["x_ref"].shape == z["y_ref"].shape == z["exp_start"].shape == (3,) and z["read_times"].shape == (3,)
    np.testing.assert_array_equal(z["exp_start"], obs.exp_start_times[:3])
    assert np.isfinite(z["spectra"]).all() and np.abs(z["spectra"]).max() > 0
    # --spectra: the same spectra beside the _raw files, which are those of a visit without the flag
    both = str(tmp_path / "both.npz")
    obs = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra", both])
    assert sorted(os.listdir(obs.outdir)) == ["0000_flt.fits", "0001_raw.fits", "0002_raw.fits", "0003_raw.fits",
                                              "params.yml", "visit_plan.txt"]
    zb = np.load(both)
    assert zb["spectra"].tobytes() == z["spectra"].tobytes() and zb["sky"].tobytes() == z["sky"].tobytes()
    frame = obs._generate_exposure(obs.exp_start_times[1], 2, write_fits=False)
    assert frame.spectra.tobytes() == z["spectra"][1].tobytes()
