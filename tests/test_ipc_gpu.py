"""GPU: inter-pixel capacitance on the device (wayne_exposure_set_ipc; k_ipc, k_ipc_clear) against the integer law of
tests/ipc_law.py, tolerance 0 everywhere.

The coupling draws nothing and acts on the thrower's accumulators, so a run with it and the same run without it share
every random stream: the accumulators between the two halves of the plain run, put through the law, ARE what the coupled
run must hold there, bit for bit.  The reads are checked without restating k_ramp: the identity kernel must leave them
as they are, a kernel whose one weight sits on the right-hand neighbour must shift them by a column.
"""
import copy
import os
import shutil

import numpy as np
import pytest
import yaml

import helpers
import ipc_law as law
from wayne_amd import _lib, engine, fitsio, ipc, run_visit, traps as T
from wayne_amd import visit as visit_mod
from wayne_amd.sources import Contaminant

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")

# every neighbour different: a transposed or flipped stencil is another kernel
ASYM = ipc.InterpixelCapacitance(kernel=[[0.011, 0.023, 0.004], [0.031, None, 0.017], [0.002, 0.027, 0.008]])
IDENTITY = ipc.InterpixelCapacitance(kernel=[[0, 0, 0], [0, 1, 0], [0, 0, 0]])
SHIFT = ipc.InterpixelCapacitance(kernel=[[0, 0, 0], [0, 0, 1], [0, 0, 0]])
VISITS = ["tiny", "tiny_g102", "tiny128", "small256", "stare256", "ramp16_128"]
# The thrower's boxes reach 6.9 sigma of the wide PSF component (49 px for G141) beyond the trace: where the 64-pixel
# visits point, they cover the whole 74-pixel frame and no hit can lie outside them.  These two are pointed at the
# frame's lower edge, so that the uppermost light-sensitive rows lie outside every interval's dilated box, and get a
# rate at which those few rows still collect their hits.
POINTING = {"tiny": dict(y_ref=476.0, hits=400.0), "tiny_g102": dict(y_ref=476.0, hits=200.0)}
Q = 2.0 ** 28
# every stage that can be switched off, off: a read is then the cumulative accumulators over the constant gain
BARE = dict(sky_background=0.0, add_gain_variations=False, add_dark=False, add_non_linear=False,
            clip_values_det_limits=False, add_read_noise=False, add_initial_bias=False)


def cosmic_rate_for(v, hits=80.0):
    """A rate (hits per second per 1024^2 pixels) at which the exposure expects `hits` cosmic rays: on the small
    sub-arrays that is far above the natural 11."""
    N = v.SUBARRAY if v.SUBARRAY != 1024 else 1014
    t = float(np.max(v.detector.get_read_times(v.NSAMP, v.SUBARRAY, v.SAMPSEQ)))
    return max(11.0, hits * 1024.0 * 1024.0 / (N * N * t))


def prepare(name, out=np.float32, i=0, **over):
    v = helpers.make_visit(name, n_exposures=i + 1)
    opts = {k: over.pop(k) for k in ("ipc", "contaminants", "charge_traps", "extraction", "expected", "rng_mode") if k in over}
    hits = over.pop("hits", 80.0)
    over.setdefault("cosmic_rate", cosmic_rate_for(v, hits))
    kw = v.frame_kwargs(i, **over)
    pg = helpers.product_generator(v, i)
    pg.prepare(out_dtype=out, **opts, **kw)
    eng, desc, _ = pg._prepared
    pg._prepared = None
    return v, pg, eng, desc


def halves(ctx, desc, model=None, slot=0):
    """upload (+ the coupling), front half, accumulators as integers, back half -> (acc int64 [R, S, S], reads)."""
    ctx.upload(slot, desc)
    if model is not None:
        ctx.set_ipc(slot, model)
    ctx.run_front(slot)
    acc = ctx.debug_fetch(slot, acc=True)[3]
    ctx.run_back(slot)
    q = acc * Q
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < 2.0 ** 53          # (the doubles hold the integers exactly)
    return q.astype(np.int64), ctx.download(slot).copy()


def whole(ctx, desc, model=None, slot=0):
    ctx.upload(slot, desc)
    if model is not None:
        ctx.set_ipc(slot, model)
    ctx.run(slot)
    return ctx.download(slot).copy()


def hits_outside_dilated_boxes(ctx, slot, a0):
    """Pixels of the plain accumulators that are non-zero outside their read interval's box dilated by a pixel: cosmic-ray
    hits that only the segment bits tell k_ramp about."""
    use, boxes, _ = ctx.debug_boxes(slot)
    assert use, "the visit runs without accumulator boxes"
    S = a0.shape[1]
    n = 0
    for r in range(a0.shape[0]):
        x0, x1, y0, y1 = (int(b) for b in boxes.reshape(16, 4)[r])
        inside = np.zeros((S, S), dtype=bool)
        if x0 < x1 and y0 < y1:
            inside[max(y0 - 1, 0):y1 + 1, max(x0 - 1, 0):x1 + 1] = True
        n += int(((a0[r] != 0) & ~inside).sum())
    return n


def two_contaminants(desc):
    wl, fl = desc._keep[0], desc._keep[1]
    # one beside the target, one whose trace leaves the frame on the right: half of it lands nowhere
    return [Contaminant(14.0, -22.0, wl.copy(), fl * 0.3, 1), Contaminant(150.0, 9.0, wl.copy(), fl * 0.4, 2)]


# ---- 1. the law, tolerance 0 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VISITS)
def test_the_coupled_accumulators_are_the_law_of_the_plain_ones(name):
    v, pg, eng, desc = prepare(name, **POINTING.get(name, {}))
    if name == "small256":
        v, pg, eng, desc = prepare(name, contaminants=two_contaminants(desc))
        assert len(desc._sources) == 2
    ctx = eng.ctx
    a0, reads0 = halves(ctx, desc)
    outside = hits_outside_dilated_boxes(ctx, 0, a0)
    print("%s: %d hits outside the dilated boxes" % (name, outside))
    assert outside >= 8
    a1, reads1 = halves(ctx, desc, ASYM)
    want = law.couple(a0, ASYM.weights())
    assert a0.shape[0] == v.NSAMP - 1 and a0.any(axis=(1, 2)).all()
    bad = np.argwhere(a1 != want)
    assert bad.size == 0, "%d accumulators off the law, first (r, y, x) = %s" % (len(bad), bad[:5].tolist())
    assert not np.array_equal(reads0, reads1)
    # the plain slot afterwards: as it was
    a2, reads2 = halves(ctx, desc)
    np.testing.assert_array_equal(a2, a0)
    np.testing.assert_array_equal(reads2, reads0)


@pytest.mark.parametrize("name", ["tiny_g102", "small256", "stare256"])
def test_the_ramp_kernel_gets_the_boxes_a_pixel_wider(name):
    """The planner's boxes keep 3 px of slack beyond where an electron can land, so no thrown charge ever shows that the
    box handed to the ramp kernel is dilated: it is looked at as the library reports it (debug_boxes)."""
    v, pg, eng, desc = prepare(name, **POINTING.get(name, {}))
    ctx = eng.ctx
    ctx.upload(0, desc)
    use, plain, seg_plain = ctx.debug_boxes(0)
    ctx.set_ipc(0, ASYM)
    use_on, wide, seg_wide = ctx.debug_boxes(0)
    S, R = ctx.S, v.NSAMP - 1
    assert use and use_on
    want = plain.copy()
    for r in range(R):
        x0, x1, y0, y1 = (int(b) for b in plain[r])
        assert x0 < x1 and y0 < y1
        want[r] = [max(x0 - 1, 0), min(x1 + 1, S), max(y0 - 1, 0), min(y1 + 1, S)]
    np.testing.assert_array_equal(wide, want)
    assert (wide[:R, 3] - wide[:R, 2] > plain[:R, 3] - plain[:R, 2]).all()       # (every visit here has room to grow in y)
    assert (seg_wide[:R] >= seg_plain[:R]).all() and (seg_wide[:R] > seg_plain[:R]).any()
    ctx.set_ipc(0, None)
    np.testing.assert_array_equal(ctx.debug_boxes(0)[1], plain)


# ---- 2. the reads, tolerance 0 -------------------------------------------------------------------------------------

@pytest.mark.parametrize("out", [np.float32, np.float64, np.uint16])
@pytest.mark.parametrize("slot", [0, 5])
def test_the_identity_kernel_leaves_every_read_as_it_is(out, slot):
    v, pg, eng, desc = prepare("tiny128", out=out)
    plain = whole(eng.ctx, desc, slot=slot)
    got = whole(eng.ctx, desc, IDENTITY, slot=slot)
    assert got.dtype == np.dtype(out)
    np.testing.assert_array_equal(got.view(np.uint8), plain.view(np.uint8))


@pytest.mark.parametrize("history", ["planned", "carried"])
def test_the_identity_kernel_under_charge_traps(history):
    model = T.ChargeTraps(slow=dict(initial=300.0, orbit_fill=150.0), fast=dict(initial=40.0, orbit_fill=20.0))
    traps = T.ExposureTraps(model) if history == "planned" else T.CarriedTraps(model, 60.0, False, (30.0, 5.0))
    v, pg, eng, desc = prepare("small256", charge_traps=traps)
    ctx = eng.ctx
    got = {}
    for key, kernel in (("plain", None), ("identity", IDENTITY)):
        if history == "carried":
            ctx.trap_state_reset(model.array("initial"))
        reads = whole(ctx, desc, kernel)
        state = ctx.trap_state_download() if history == "carried" else np.zeros(1, dtype=np.float32)
        got[key] = (reads, state)
    assert ctx.ramp_variant(0).startswith("k_ramp_hist<" if history == "carried" else "k_ramp_trap<")
    np.testing.assert_array_equal(got["identity"][0].view(np.uint8), got["plain"][0].view(np.uint8))
    np.testing.assert_array_equal(got["identity"][1].view(np.uint32), got["plain"][1].view(np.uint32))


@pytest.mark.parametrize("out", [np.float32, np.float64, np.uint16])
def test_a_weight_on_the_right_hand_neighbour_shifts_the_reads_by_a_column(out):
    v, pg, eng, desc = prepare("tiny128", out=out, **BARE)
    plain = whole(eng.ctx, desc)
    got = whole(eng.ctx, desc, SHIFT)
    S = plain.shape[1]
    assert plain[-1, 5:S - 5, 5:S - 5].max() > 100
    # light-sensitive columns whose right-hand neighbour is light-sensitive too
    np.testing.assert_array_equal(got[:, 5:S - 5, 5:S - 6], plain[:, 5:S - 5, 6:S - 5])
    assert not np.array_equal(got, plain)


# ---- 3. cleanliness ------------------------------------------------------------------------------------------------

def fresh_engine(v):
    return engine.Engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)


@pytest.fixture(scope="module")
def small():
    """small256 with cosmic rays and the asymmetric kernel: the descriptors, and the reads of a context of its own that
    ran nothing else -- plain and coupled."""
    v, pg, eng, desc = prepare("small256")
    _, _, _, desc_x = prepare("small256", extraction=True)
    fresh = fresh_engine(v)
    try:
        plain = whole(fresh.ctx, desc)
        fresh.ctx.upload(0, desc_x)
        fresh.ctx.run(0)
        plain_x = (fresh.ctx.download(0).copy(),) + tuple(a.copy() for a in fresh.ctx.download_spectra(0))
    finally:
        fresh.close()
    fresh = fresh_engine(v)
    try:
        coupled = whole(fresh.ctx, desc, ASYM)
    finally:
        fresh.close()
    assert not np.array_equal(plain, coupled)
    return dict(v=v, ctx=eng.ctx, desc=desc, desc_x=desc_x, plain=plain, plain_x=plain_x, coupled=coupled)


def test_a_second_run_of_the_slot_gives_the_same_bytes(small):
    ctx = small["ctx"]
    np.testing.assert_array_equal(whole(ctx, small["desc"], ASYM), small["coupled"])
    ctx.run(0)                                     # the slot again, as it stands
    np.testing.assert_array_equal(ctx.download(0), small["coupled"])
    np.testing.assert_array_equal(whole(ctx, small["desc"], ASYM), small["coupled"])


def test_a_front_half_alone_leaves_nothing_behind(small):
    ctx = small["ctx"]
    ctx.upload(0, small["desc"])
    ctx.set_ipc(0, ASYM)
    ctx.run_front(0)                               # ... and no back half
    ctx.run_front(0)
    ctx.run_back(0)
    np.testing.assert_array_equal(ctx.download(0), small["coupled"])
    # a front half with the option, then the slot uploaded without it
    ctx.upload(0, small["desc"])
    ctx.set_ipc(0, ASYM)
    ctx.run_front(0)
    np.testing.assert_array_equal(whole(ctx, small["desc"]), small["plain"])
    np.testing.assert_array_equal(whole(ctx, small["desc"], ASYM), small["coupled"])


def test_an_upload_without_the_option_after_a_run_with_it(small):
    ctx = small["ctx"]
    np.testing.assert_array_equal(whole(ctx, small["desc"], ASYM), small["coupled"])
    np.testing.assert_array_equal(whole(ctx, small["desc"]), small["plain"])
    # set, then cleared by NULL
    ctx.upload(0, small["desc"])
    ctx.set_ipc(0, ASYM)
    ctx.set_ipc(0, None)
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), small["plain"])


def test_either_stream_gives_the_same_bytes(small):
    ctx = small["ctx"]
    for slot in (0, 1, 2, 3):
        ctx.upload(slot, small["desc"])
        ctx.set_ipc(slot, ASYM)
        ctx.run(slot)
    for slot in (0, 1, 2, 3):
        np.testing.assert_array_equal(ctx.download(slot), small["coupled"])


def test_a_rerun_the_library_makes_itself_comes_out_the_same(small):
    ctx = small["ctx"]
    ctx.set_knob("lane_reach", 5)
    try:
        n0 = ctx.reruns
        got = whole(ctx, small["desc"], ASYM)
        ctx.synchronize()
        assert ctx.reruns == n0 + 1
        # ... and one between the halves
        ctx.upload(0, small["desc"])
        ctx.set_ipc(0, ASYM)
        ctx.run_front(0)
        acc = ctx.debug_fetch(0, acc=True)[3]
        ctx.run_back(0)
        again = ctx.download(0).copy()
    finally:
        ctx.set_knob("lane_reach", None)
    np.testing.assert_array_equal(got, small["coupled"])
    np.testing.assert_array_equal(again, small["coupled"])
    a0, _ = halves(ctx, small["desc"])
    np.testing.assert_array_equal((acc * Q).astype(np.int64), law.couple(a0, ASYM.weights()))


# ---- 4. everything else keeps its bytes ----------------------------------------------------------------------------

def test_the_expected_image_is_not_coupled():
    v, pg, eng, desc = prepare("tiny128", expected="counts")
    ctx = eng.ctx
    ctx.upload(0, desc)
    ctx.run(0)
    plain, e_plain = ctx.download(0).copy(), ctx.expected(0)
    ctx.upload(0, desc)
    ctx.set_ipc(0, ASYM)
    ctx.run(0)
    coupled, e_coupled = ctx.download(0).copy(), ctx.expected(0)
    assert e_plain.any() and not np.array_equal(plain, coupled)
    np.testing.assert_array_equal(e_coupled.view(np.uint64), e_plain.view(np.uint64))


def test_without_the_option_reads_and_spectra_are_those_of_a_context_that_never_saw_it(small):
    ctx = small["ctx"]
    whole(ctx, small["desc"], ASYM)
    ctx.upload(0, small["desc_x"])
    ctx.set_ipc(0, ASYM)
    ctx.run(0)
    spectra_on = ctx.download_spectra(0)[0].copy()
    ctx.upload(0, small["desc_x"])
    ctx.run(0)
    reads, (spectra, sky) = ctx.download(0).copy(), ctx.download_spectra(0)
    np.testing.assert_array_equal(reads, small["plain_x"][0])
    np.testing.assert_array_equal(spectra.view(np.uint64), small["plain_x"][1].view(np.uint64))
    np.testing.assert_array_equal(sky.view(np.uint64), small["plain_x"][2].view(np.uint64))
    assert not np.array_equal(spectra_on, spectra)          # (the extraction does see the coupled reads)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------

def test_refusals_leave_the_slot_usable(small):
    ctx, desc = small["ctx"], small["desc"]
    nan, inf = float("nan"), float("inf")
    good = ASYM.kernel
    bad = []
    for value in (nan, inf, -1e-3, 0.95):
        k = good.copy()
        k[0, 2] = value
        bad.append(k)
    for k in bad:
        ctx.upload(0, desc)
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_ipc(0, k)
        assert e.value.status == _lib.E_INVALID
        ctx.run(0)
        np.testing.assert_array_equal(ctx.download(0), small["plain"])
    # a refusal clears an option that was set
    ctx.upload(0, desc)
    ctx.set_ipc(0, ASYM)
    with pytest.raises(_lib.WayneError):
        ctx.set_ipc(0, bad[0])
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), small["plain"])
    # a slot that was never uploaded
    unused = int(ctx._L.wayne_ctx_slots(ctx._h)) - 1
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_ipc(unused, ASYM)
    assert e.value.status == _lib.E_STATE
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_ipc(-1, ASYM)
    assert e.value.status == _lib.E_INVALID
    # replay mode reproduces the reference, which has no coupling
    _, _, reng, rdesc = prepare("small256", rng_mode=_lib.RNG_REPLAY, cosmic_rate=None)
    want = whole(reng.ctx, rdesc, slot=1)
    reng.ctx.upload(1, rdesc)
    with pytest.raises(_lib.WayneError) as e:
        reng.ctx.set_ipc(1, ASYM)
    assert e.value.status == _lib.E_INVALID
    reng.ctx.run(1)
    np.testing.assert_array_equal(reng.ctx.download(1), want)


def test_the_profile_slot_counts_coupled_exposures_only(small):
    ctx = small["ctx"]
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        whole(ctx, small["desc"])
        assert ctx.ipc_profile()[0] == 0
        whole(ctx, small["desc"], ASYM)
        whole(ctx, small["desc"], ASYM, slot=1)
        n, ms = ctx.ipc_profile()
        assert n == 2 and ms > 0.0
        ctx.profile_select(["k_ipc"])
        ctx.profile_reset()
        whole(ctx, small["desc"], ASYM)
        assert ctx.ipc_profile()[0] == 1 and ctx.profile_get()["k_ramp"]["launches"] == 0
    finally:
        ctx.profile_select(None)
        ctx.profile_enable(False)


# ---- 6. the public path --------------------------------------------------------------------------------------------

def test_scanning_frame_and_the_visit_runner_take_the_option():
    v = helpers.make_visit("tiny128", n_exposures=2)
    frames = {}
    for key, model in (("plain", None), ("coupled", ASYM)):
        frames[key] = [np.stack([r[0] for r in helpers.product_generator(v, i).scanning_frame(ipc=model, **v.frame_kwargs(i)).reads])
                       for i in range(2)]
    assert not np.array_equal(frames["plain"][0], frames["coupled"][0])
    runner = visit_mod.VisitRunner(v, ipc=ASYM)
    got = runner.run([0, 1], keep=True)
    for i in range(2):
        np.testing.assert_array_equal(np.asarray(got[i]), frames["coupled"][i])
    got = visit_mod.VisitRunner(v).run([0, 1], keep=True)
    for i in range(2):
        np.testing.assert_array_equal(np.asarray(got[i]), frames["plain"][i])
    # a staring frame passes it on
    s = helpers.make_visit("stare256")
    with pytest.raises(ValueError):
        helpers.product_generator(s, 0).scanning_frame(ipc=ASYM, rng_mode=_lib.RNG_REPLAY, **s.frame_kwargs(0))


VOLATILE = ("DATE", "SIM-TIME")


def _files(outdir):
    out = {}
    for n in sorted(f for f in os.listdir(outdir) if f.endswith("_raw.fits")):
        hdus = fitsio.read(os.path.join(outdir, n))
        cards = [[(k, v) for k, v, _ in hd.header.cards if k not in VOLATILE] for hd in hdus]
        out[n] = (cards, [hd.data for hd in hdus])
    return out


def _same(a, b):
    return a[0] == b[0] and all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def _cli(work, section="absent", resume=False):
    yml = os.path.join(work, "params.yml")
    cfg = yaml.safe_load(open(os.path.join(MINI, "params.yml")))
    if section != "absent":
        cfg["interpixel_capacitance"] = copy.deepcopy(section)
    with open(yml, "w") as f:
        yaml.safe_dump(cfg, f)
    obs = run_visit.run(["-p", yml, "--max-exposures", "2"] + (["--resume"] if resume else []))
    return obs, _files(obs.outdir)


def test_the_cli_writes_the_cards_and_resume_knows_them(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    shutil.copytree(MINI, a)
    shutil.copytree(MINI, b)
    _, plain = _cli(a)
    names = ["0001_raw.fits", "0002_raw.fits"]
    assert sorted(plain) == names
    p0 = dict(plain[names[0]][0][0])
    assert not any(k.startswith("IPC") for k in p0)
    # with the section: the cards, and other reads
    obs, coupled = _cli(b, {"alpha": 0.02})
    model = ipc.InterpixelCapacitance(alpha=0.02)
    for n in names:
        p0 = dict(coupled[n][0][0])
        for key, value, _ in model.cards():
            assert p0[key] == value and type(p0[key]) is type(value), key
        assert not _same(coupled[n], plain[n])
        sci_c = [d for d in coupled[n][1] if d is not None][0]
        sci_p = [d for d in plain[n][1] if d is not None][0]
        assert sci_c.shape == sci_p.shape and not np.array_equal(sci_c, sci_p)
    # --resume with the same kernel: nothing to do
    obs, again = _cli(b, {"alpha": 0.02}, resume=True)
    assert obs.skipped == [0, 1] and all(_same(again[n], coupled[n]) for n in names)
    # ... after the kernel is changed: every file again
    obs, changed = _cli(b, {}, resume=True)
    assert obs.skipped == []
    assert dict(changed[names[0]][0][0])["IPCW01"] == 1638 and not _same(changed[names[0]], coupled[names[0]])
    # ... and after it is removed: every file again, and the bytes of the visit that never had the section (whose slots
    # have seen the option in between)
    obs, removed = _cli(b, resume=True)
    assert obs.skipped == []
    assert all(_same(removed[n], plain[n]) for n in names)
    # ... and switched on over plain files
    obs, on = _cli(b, {"alpha": 0.02}, resume=True)
    assert obs.skipped == [] and all(_same(on[n], coupled[n]) for n in names)
