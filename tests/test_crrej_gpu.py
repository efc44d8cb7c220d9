"""GPU: cosmic-ray rejection of the device-side extraction (wayne_exposure_set_crrej; k_extract_crmask and the
rejecting instantiations of k_extract_rows / k_extract_finish).

The oracle in every case is the law restated in numpy (tests/crrej_law.py) applied to the reads of the SAME slot: the
flag plane and the counts must be equal -- a flag is one float64 comparison formed with the law's own operations; the
pixels where a contracted multiply-add could decide it the other way are reported by the oracle and every case first
checks that it has none -- and spectra and sky may differ by the order of their float64 row sums, 1e-9 of M[x] per
column (tests/extraction_law.py).  Host side: tests/test_crrej.py."""
import collections
import os
import shutil

import numpy as np
import pytest

import crrej_law
import extraction_law as law
import helpers
from wayne_amd import _lib, engine, extraction, run_visit
from wayne_amd.visit import VisitRunner

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "fixtures", "mini_visit")
_visits, _planes = {}, {}
Run = collections.namedtuple("Run", "reads spectra sky rejected mask plan")


def visit(name, n=6):
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
    gen = helpers.product_generator(v, i)
    return gen.build_descriptor(engine_of(v), out_dtype=out_dtype, extraction=ex, **v.frame_kwargs(i, **over)), gen


def fetch(ctx, slot, plan):
    reads = ctx.download(slot)
    spectra, sky = ctx.download_spectra(slot)
    cr = plan.crrej is not None
    return Run(reads, spectra, sky, ctx.rejected(slot) if cr else None, ctx.download_crmask(slot) if cr else None, plan)


def extracted(v, i, ex, out_dtype=np.float32, slot=0, **over):
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, i, ex, out_dtype, **over)
    ctx.upload(slot, desc)
    ctx.run(slot)
    return fetch(ctx, slot, gen.extraction_plan)


def busy_rate(v, per_interval=30.0):
    """The cosmic_rate (hits / s / 1024^2) at which the shortest read interval of v carries `per_interval` hits."""
    dt = np.diff(np.concatenate([[0.0], np.asarray(v.read_times, dtype=float)]))
    N = v.detector.light_sensitive_size(v.SUBARRAY)
    return per_interval * 1024.0 ** 2 / (N * N * dt.min())


def oracle_of(run, v, steps=law.ALL, k=8.0, rn=20.0, windows=None, bg=None):
    windows = run.plan.row_windows if windows is None else windows
    return crrej_law.restate(run.reads, planes(v), windows, run.plan.bg_cols if bg is None else bg, steps, k, rn)


def assert_is_the_law(run, want, what):
    assert not want.undecided.any(), "%s: %d undecided pixels -- take another exposure" % (what, want.undecided.sum())
    lo, hi = run.plan.mask_rows
    assert not run.mask[:lo].any() and not run.mask[hi:].any(), what
    np.testing.assert_array_equal(run.mask, want.mask, err_msg=what)
    np.testing.assert_array_equal(run.rejected, want.n_rejected, err_msg=what)
    crrej_law.assert_parity(run.spectra, run.sky, want, what)


def flags_in_windows(mask, windows, R):
    """(flags of interval j inside window j, flags of interval j inside the last-read window but outside window j)"""
    inside = last_only = 0
    rows = np.arange(mask.shape[0])[:, None]
    for j in range(R):
        f = (mask >> j) & 1 == 1
        own = (rows >= windows[j][0]) & (rows < windows[j][1])
        last = (rows >= windows[R][0]) & (rows < windows[R][1])
        inside += int((f & own).sum())
        last_only += int((f & last & ~own).sum())
    return inside, last_only


# (name, exposure of a 6-exposure visit): the exposure is one whose hits -- the CPU oracle's PhiloxDraws place them where
# the device does -- fall inside a read interval's window and, where the windows differ on tested rows (a scan under
# the default margin), inside the last-read window alone too.  tiny under margin=40 and a staring exposure have the
# same tested rows in every window, so no flag can lie in the last-read window alone there.
CASES = [("tiny", 0), ("small256", 1), ("stare256", 0), ("cfg3", 0)]
LAST_ONLY = ("small256", "cfg3", "cfg4")


def parity_case(name, i, out_dtype):
    v = visit(name)
    if name == "tiny":
        # S = 74, a second column tile of 10 columns, windows at both clamps; a few tens of hits per read interval: next
        # to the +-7 margin, in a tile's halo, and adjacent to each other
        ex, over = extraction.ExtractionOptions(margin=40, crrej=True), dict(cosmic_rate=busy_rate(v))
    else:
        ex, over = extraction.ExtractionOptions(crrej=True), {}
    run = extracted(v, i, ex, out_dtype, **over)
    R, S = v.NSAMP - 1, planes(v).S
    what = "%s[%d] %s" % (name, i, np.dtype(out_dtype).name)
    assert run.spectra.shape == (R + 1, S) and run.rejected.shape == (R + 1,) and run.rejected.dtype == np.uint32
    assert run.mask.shape == (S, S) and run.mask.dtype == np.uint16
    if name == "tiny":
        assert S == 74 and run.plan.row_windows[:, 0].min() == 5 and run.plan.row_windows[:, 1].max() == S - 5
    if name == "cfg3":
        assert R == 14 and int(run.mask.max()) >> 8 > 0                # bits beyond the low byte are in use
    if name == "cfg4":
        assert S == 1024 and R == 15 and run.plan.row_windows[R, 1] - run.plan.row_windows[R, 0] > 20 * 32
    want = oracle_of(run, v)
    assert_is_the_law(run, want, what)
    inside, last_only = flags_in_windows(run.mask, run.plan.row_windows, R)
    print("%s: %d flags, %d in their interval's window, %d in the last-read window alone, n_rejected %s" % (
        what, np.count_nonzero(run.mask), inside, last_only, list(run.rejected)))
    assert inside >= 1 and run.rejected[:R].sum() == inside and run.rejected[R] >= 1
    if name in LAST_ONLY:
        assert last_only >= 1 and run.rejected[R] == inside + last_only
    # the rejection matters: the plain law on the same reads is far off in a flagged column
    plain, _, _, _ = law.restate(run.reads, planes(v), run.plan.row_windows, run.plan.bg_cols)
    assert np.abs(plain - want.spectra).max() > 1000.0


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64, np.uint16], ids=["f32", "f64", "u16"])
@pytest.mark.parametrize("name,i", CASES, ids=[c[0] for c in CASES])
def test_mask_counts_and_spectra_are_the_law_applied_to_the_slots_reads(name, i, out_dtype):
    parity_case(name, i, out_dtype)


def test_mask_counts_and_spectra_on_the_full_array():
    parity_case("cfg4", 0, np.float32)


def test_rejected_spectra_against_the_exposure_without_cosmic_rays():
    v = visit("small256")
    steps = extraction.ALL & ~extraction.SKY
    i = 4
    on = extracted(v, i, extraction.ExtractionOptions(steps=steps, crrej=True), slot=0)
    raw = extracted(v, i, extraction.ExtractionOptions(steps=steps), slot=1)
    clean = extracted(v, i, extraction.ExtractionOptions(steps=steps), slot=2, cosmic_rate=None)
    # the two runs differ at the hit pixels alone (the streams of the other stages do not depend on the cosmic rays)
    differ = (on.reads != clean.reads).any(axis=0)
    hit = (np.abs(on.reads.astype(np.float64) - clean.reads.astype(np.float64)) > 100.0).any(axis=0)
    print("pixels whose reads differ between the runs: %d, of which hit pixels: %d" % (differ.sum(), (differ & hit).sum()))
    assert hit.sum() >= 5 and not (differ & ~hit).any()
    np.testing.assert_array_equal(on.reads, raw.reads)
    R = v.NSAMP - 1
    inside, last_only = flags_in_windows(on.mask, on.plan.row_windows, R)
    assert inside >= 1 and last_only >= 1 and on.rejected[R] == inside + last_only
    # a column without a flag in any interval: every product is that of the exposure without cosmic rays, byte for byte
    # (a flagged column's LATER intervals differ too: the hit's charge stays in the pixel and the linearity correction
    # of what follows is taken at another level)
    flagged = on.mask.any(axis=0)
    assert flagged.sum() >= 5 and not flagged.all()
    assert on.spectra[:, ~flagged].tobytes() == clean.spectra[:, ~flagged].tobytes()
    left, was = np.abs(on.spectra - clean.spectra).sum(), np.abs(raw.spectra - clean.spectra).sum()
    print("sum|rejected - clean| / sum|unrejected - clean| = %.1f / %.1f = %.3g" % (left, was, left / was))
    assert left <= 0.01 * was


def test_hand_made_windows_with_rejection():
    # one row; a window that ends exactly at S - 5; chunks and a remainder; the whole frame, whose border rows are untested
    v = visit("small256")
    S = 266
    for windows in ([(100, 101), (200, S - 5), (5, 5 + 3 * 32 + 7), (0, S)],
                    [(S - 9, S - 8), (7, 8), (31, 65), (5, S - 5)],
                    [(100, 101)] * 4):
        ex = extraction.Extraction(windows, bg_cols=(0, S), crrej=True)
        run = extracted(v, 0, ex, cosmic_rate=busy_rate(v, 3.0))
        assert run.plan.mask_rows == (min(w[0] for w in windows), max(w[1] for w in windows))
        want = oracle_of(run, v)
        assert_is_the_law(run, want, "windows %s" % (windows,))
        if windows[-1][1] - windows[-1][0] > 100:
            assert want.n_rejected[-1] >= 1
        if windows[-1] == (0, S):
            assert not run.mask[:7].any() and not run.mask[S - 7:].any() and run.mask[7:S - 7].any()
            assert not run.mask[:, :7].any() and not run.mask[:, S - 7:].any()


def test_other_thresholds_and_steps():
    v = visit("small256")
    for k, rn, steps in ((4.0, 0.0, extraction.ALL), (6.0, 30.0, extraction.GAIN),
                         (8.0, 20.0, extraction.ALL & ~extraction.LAST_READ)):
        ex = extraction.ExtractionOptions(steps=steps, crrej=extraction.CosmicRejection(k, rn))
        run = extracted(v, 1, ex, cosmic_rate=busy_rate(v, 3.0))
        want = oracle_of(run, v, steps, k, rn)
        assert_is_the_law(run, want, "k %g rn %g steps %d" % (k, rn, steps))
        assert want.n_rejected[:-1].sum() >= 1
        if not steps & extraction.LAST_READ:
            assert run.rejected[-1] == 0 and (run.spectra[-1] == 0.0).all()


def test_the_same_exposure_gives_the_same_bytes():
    v = visit("small256")
    ctx = engine_of(v).ctx
    ex = extraction.ExtractionOptions(crrej=True)
    desc, gen = descriptor(v, 1, ex, cosmic_rate=busy_rate(v, 3.0))
    for slot in (0, 1):                                              # the two streams
        ctx.upload(slot, desc)
        ctx.run(slot)
    a, b = fetch(ctx, 0, gen.extraction_plan), fetch(ctx, 1, gen.extraction_plan)

    def same(x, y):
        return (x.spectra.tobytes() == y.spectra.tobytes() and x.sky.tobytes() == y.sky.tobytes() and
                x.rejected.tobytes() == y.rejected.tobytes() and x.mask.tobytes() == y.mask.tobytes())

    assert same(a, b) and a.rejected.sum() > 0 and a.mask.any()
    for slot, i in ((0, 0), (1, 2), (2, 0)):                         # other exposures, with other plans, in between
        other, _ = descriptor(v, i, extraction.ExtractionOptions(margin=3 + slot, crrej=extraction.CosmicRejection(5.0)),
                              cosmic_rate=busy_rate(v, 10.0))
        ctx.upload(slot, other)
        ctx.run(slot)
    ctx.synchronize()
    ctx.upload(3, desc)
    ctx.run(3)
    assert same(fetch(ctx, 3, gen.extraction_plan), a)
    ctx.run(3)                                                       # a second run rewrites the plane, it does not add to it
    assert same(fetch(ctx, 3, gen.extraction_plan), a)
    # ... also in a slot whose plane holds another exposure's flags
    ctx.upload(0, desc)
    ctx.run(0)
    assert same(fetch(ctx, 0, gen.extraction_plan), a)


def test_off_means_off():
    v = visit("small256")
    ctx = engine_of(v).ctx
    desc, gen = descriptor(v, 1, True)
    with_cr, _ = descriptor(v, 1, extraction.ExtractionOptions(crrej=True))
    ctx.upload(0, desc)
    ctx.run(0)
    never, never_sky = ctx.download_spectra(0)
    assert not ctx.has_crrej(0)
    ctx.upload(1, with_cr)
    assert ctx.has_crrej(1)
    ctx.set_crrej(1, None)                                           # set, then cleared
    ctx.run(1)
    got, got_sky = ctx.download_spectra(1)
    assert got.tobytes() == never.tobytes() and got_sky.tobytes() == never_sky.tobytes()
    for call in (ctx.rejected, ctx.download_crmask):
        with pytest.raises(_lib.WayneError) as e:
            call(1)
        assert e.value.status == _lib.E_STATE
    ctx.upload(2, with_cr)
    ctx.run(2)
    rejecting, _ = ctx.download_spectra(2)
    assert rejecting.tobytes() != never.tobytes()
    ctx.upload(2, desc)                                              # a fresh upload clears it; so does set_extraction
    ctx.run(2)
    got, got_sky = ctx.download_spectra(2)
    assert got.tobytes() == never.tobytes() and got_sky.tobytes() == never_sky.tobytes()
    ctx.upload(2, with_cr)
    ctx.set_extraction(2, gen.extraction_plan)
    assert not ctx.has_crrej(2)
    ctx.run(2)
    ctx.fetch_spectra_async(2)
    got, got_sky = ctx.wait_spectra(2)
    assert got.tobytes() == never.tobytes() and got_sky.tobytes() == never_sky.tobytes()


def test_errors():
    v = visit("small256")
    ctx = engine_of(v).ctx
    plain, _ = descriptor(v, 1, None)
    ctx.upload(0, plain)
    with pytest.raises(_lib.WayneError) as e:                        # no extraction on the slot
        ctx.set_crrej(0, extraction.CosmicRejection())
    assert e.value.status == _lib.E_STATE
    with pytest.raises(_lib.WayneError) as e:                        # a slot that was never uploaded
        ctx.set_crrej(201, extraction.CosmicRejection())
    assert e.value.status == _lib.E_STATE
    desc, gen = descriptor(v, 1, True)
    ctx.upload(1, desc)
    ctx.run(1)
    never, never_sky = ctx.download_spectra(1)

    def bad_desc(k, rn):
        d = _lib.CrrejDesc()
        d.k, d.read_noise_e = k, rn
        cr = extraction.CosmicRejection()
        cr.desc = lambda: d
        return cr

    nan, inf = float("nan"), float("inf")
    for k, rn in ((0.0, 20.0), (-8.0, 20.0), (nan, 20.0), (inf, 20.0), (8.0, -1.0), (8.0, nan), (8.0, inf)):
        ctx.upload(0, desc)
        ctx.set_crrej(0, extraction.CosmicRejection())
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_crrej(0, bad_desc(k, rn))
        assert e.value.status == _lib.E_INVALID, (k, rn)
        assert not ctx.has_crrej(0)
    ctx.run(0)                                                       # ... and the slot extracts, without rejection
    got, got_sky = ctx.download_spectra(0)
    assert got.tobytes() == never.tobytes() and got_sky.tobytes() == never_sky.tobytes()
    with pytest.raises(_lib.WayneError) as e:
        ctx.rejected(0)
    assert e.value.status == _lib.E_STATE
    # the noise model is in electrons: no rejection of an extraction in DN
    no_gain, gen_ng = descriptor(v, 1, extraction.ExtractionOptions(steps=extraction.ALL & ~extraction.GAIN))
    ctx.upload(0, no_gain)
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_crrej(0, extraction.CosmicRejection())
    assert e.value.status == _lib.E_INVALID
    ctx.run(0)
    got, got_sky = ctx.download_spectra(0)
    reads = ctx.download(0)
    law.assert_parity(got, got_sky, reads, planes(v), gen_ng.extraction_plan.row_windows, (6, 26),
                      extraction.ALL & ~extraction.GAIN, what="no gain, rejection refused")
    # the counts exist once the spectra have been fetched
    with_cr, _ = descriptor(v, 1, extraction.ExtractionOptions(crrej=True))
    ctx.upload(0, with_cr)
    ctx.run(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.rejected(0)
    assert e.value.status == _lib.E_STATE
    ctx.download_spectra(0)
    assert ctx.rejected(0).shape == (v.NSAMP,)


def test_delivery_brings_the_counts():
    v = visit("small256")
    ctx = engine_of(v).ctx
    ex = extraction.ExtractionOptions(crrej=True)
    over = dict(cosmic_rate=busy_rate(v, 3.0))
    delivery = extraction.Delivery(ctx, reads=True)
    descs = [descriptor(v, i, ex, **over)[0] for i in (1, 2)] + [descriptor(v, 3, True, **over)[0]]
    for slot, desc in enumerate(descs):                             # alternating streams; the third without rejection
        delivery.upload(slot, desc)
        delivery.run(slot)
        delivery.fetch_async(slot)
    got = []
    for slot in range(3):
        reads, spectra, sky = delivery.wait(slot)
        got.append((reads.copy(), spectra.copy(), sky.copy(), delivery.rejected))
    assert got[2][3] is None and got[0][3].sum() > 0 and got[1][3].sum() > 0
    for slot in range(2):
        spectra, sky = ctx.download_spectra(slot)
        assert got[slot][1].tobytes() == spectra.tobytes() and got[slot][2].tobytes() == sky.tobytes()
        np.testing.assert_array_equal(got[slot][3], ctx.rejected(slot))
        np.testing.assert_array_equal(got[slot][0], ctx.download(slot))


def test_frames_and_visits_carry_the_counts():
    v = visit("tiny")
    over = dict(cosmic_rate=busy_rate(v))
    exp = helpers.product_generator(v, 0).scanning_frame(extraction=True, crrej=True, **v.frame_kwargs(0, **over))
    assert exp.extraction.crrej.k == 8.0 and exp.rejected.shape == (4,) and exp.rejected.sum() > 0
    plain = helpers.product_generator(v, 0).scanning_frame(extraction=True, **v.frame_kwargs(0, **over))
    assert not hasattr(plain, "rejected") and plain.spectra.tobytes() != exp.spectra.tobytes()

    runner = VisitRunner(v, frame_overrides=over)
    spectra, sky = runner.run_spectra(range(3), extraction=extraction.ExtractionOptions(crrej=True))
    assert runner.rejected.shape == (3, 4) and runner.rejected.dtype == np.uint32 and (runner.rejected.sum(axis=1) > 0).all()
    assert spectra[0].tobytes() == exp.spectra.tobytes() and list(runner.rejected[0]) == list(exp.rejected)
    runner.run_spectra(range(2))
    assert runner.rejected is None


def test_cli_writes_the_counts_only_when_asked(tmp_path):
    work = str(tmp_path / "visit")
    shutil.copytree(MINI, work)
    yml = os.path.join(work, "params.yml")
    out, plain = str(tmp_path / "rejected.npz"), str(tmp_path / "plain.npz")
    obs = run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", out, "--reject-cosmics"])
    assert sorted(os.listdir(obs.outdir)) == ["0000_flt.fits", "params.yml", "visit_plan.txt"]
    z = np.load(out)
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start"]
    assert sorted(z.files) == sorted(base + ["n_rejected", "crrej_k", "crrej_read_noise"])
    assert z["n_rejected"].shape == (3, 4) and z["n_rejected"].dtype == np.uint32
    assert float(z["crrej_k"]) == 8.0 and float(z["crrej_read_noise"]) == 20.0
    np.testing.assert_array_equal(z["n_rejected"], obs.spectra_result["rejected"])
    run_visit.run(["-p", yml, "--max-exposures", "3", "--spectra-only", plain])
    assert sorted(np.load(plain).files) == sorted(base)
    six = str(tmp_path / "six.npz")
    run_visit.run(["-p", yml, "--max-exposures", "2", "--spectra-only", six, "--reject-cosmics", "6"])
    assert float(np.load(six)["crrej_k"]) == 6.0
