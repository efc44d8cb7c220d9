"""GPU: every product of a slot whose exposure the library runs a second time is the second run's.

One exposure of configuration tiny with the extraction, FITS words, the expected image (counts), the ramp fit and the
calibrated reads all set.  It is run once as it is and every product downloaded; then, under knob lane_reach = 5 (as in
tests/test_expected_gpu.py: the first launch sequence meets a bin beyond a lane's reach, status bit 1), uploaded into
another slot and run again for each way of bringing a product back -- each called first after an upload and a run of its
own.  Each raises ctx.reruns by exactly 1 and returns the bytes of the run without the knob: no tolerance, the general
launch sequence draws the same electrons."""
import numpy as np
import pytest

import helpers
from wayne_amd import _lib, engine

pytestmark = pytest.mark.gpu

BLOCKING = ["download", "download_spectra", "download_fits", "expected", "rampfit", "ima"]
_state = {}


def as_bytes(product):
    """The product as a tuple of uint8 arrays of its own."""
    if hasattr(product, "bytes"):                       # ima.Payload
        product = product.bytes
    parts = product if isinstance(product, tuple) else (product,)
    return tuple(np.ascontiguousarray(p).view(np.uint8).copy() for p in parts)


def setup():
    """(context, descriptor, {way: bytes of the run without the knob})"""
    if not _state:
        v = helpers.make_visit("tiny")
        eng = engine.get_engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
        desc = helpers.product_generator(v, 0).build_descriptor(eng, out_dtype=np.float32, extraction=True, device_fits=True,
                                                                expected="counts", ramp_fit=True, ima="counts",
                                                                **v.frame_kwargs(0))
        ctx = eng.ctx
        _lib.set_knob_all("lane_reach", None)
        n0 = ctx.reruns
        ctx.upload(0, desc)
        assert ctx.has_fits(0) and ctx.has_expected(0) and ctx.has_rampfit(0) and ctx.has_ima(0)
        ctx.run_checked(0)
        want = {way: as_bytes(getattr(ctx, way)(0)) for way in BLOCKING}
        assert ctx.reruns == n0                         # (the run without the knob is not repeated)
        assert want["download"][0].view(np.float32).max() > 5 and want["expected"][0].view(np.float64).sum() > 1e3
        _state["all"] = (ctx, desc, want)
    return _state["all"]


def same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(as_bytes(got), want):
        assert g.shape == w.shape and (g == w).all(), what


@pytest.mark.parametrize("way", BLOCKING)
def test_a_blocking_download_brings_the_second_run(way):
    ctx, desc, want = setup()
    _lib.set_knob_all("lane_reach", "5")
    try:
        ctx.upload(3, desc)
        ctx.run(3)
        n0 = ctx.reruns
        got = as_bytes(getattr(ctx, way)(3))
        print("%s: reruns + %d" % (way, ctx.reruns - n0))
        assert ctx.reruns == n0 + 1
        assert ctx.status(3) == 0
        same(got, want[way], way)
    finally:
        _lib.set_knob_all("lane_reach", None)


@pytest.mark.parametrize("fetch,wait,way", [("fetch_async", "wait", "download"),
                                            ("fetch_spectra_async", "wait_spectra", "download_spectra"),
                                            ("fetch_fits_async", "wait_fits", "download_fits")], ids=["reads", "spectra", "fits"])
def test_a_fetch_alone_brings_the_second_run(fetch, wait, way):
    ctx, desc, want = setup()
    _lib.set_knob_all("lane_reach", "5")
    try:
        ctx.upload(4, desc)
        ctx.run(4)
        getattr(ctx, fetch)(4)
        n0 = ctx.reruns
        got = as_bytes(getattr(ctx, wait)(4))
        print("%s: reruns + %d" % (wait, ctx.reruns - n0))
        assert ctx.reruns == n0 + 1
        assert ctx.status(4) == 0
        same(got, want[way], wait)
    finally:
        _lib.set_knob_all("lane_reach", None)


# Reruns of one exposure with reads, spectra and FITS words all fetched and wait_fits called first: the number recorded
# from the library as it was before slot_gate / download_settled / PinnedMirror came in (1 behind wait_fits, 1 in all --
# wait_fits fetches the other two mirrors again, so wait and wait_spectra find the second run's status word).  Which
# mirrors each wait_* fetches again differs from one to the other and is not to be unified.
RERUNS_ALL_FETCHED = 1


def test_all_three_fetched_and_the_fits_words_waited_for_first():
    ctx, desc, want = setup()
    _lib.set_knob_all("lane_reach", "5")
    try:
        ctx.upload(5, desc)
        ctx.run(5)
        ctx.fetch_async(5)
        ctx.fetch_spectra_async(5)
        ctx.fetch_fits_async(5)
        n0 = ctx.reruns
        fits = as_bytes(ctx.wait_fits(5))
        after_fits = ctx.reruns - n0
        reads = as_bytes(ctx.wait(5))
        spectra = as_bytes(ctx.wait_spectra(5))
        print("all three fetched, wait_fits first: reruns + %d behind wait_fits, + %d in all" % (after_fits, ctx.reruns - n0))
        assert after_fits == 1
        assert ctx.reruns - n0 == RERUNS_ALL_FETCHED
        assert ctx.status(5) == 0
        same(fits, want["download_fits"], "wait_fits")
        same(reads, want["download"], "wait")
        same(spectra, want["download_spectra"], "wait_spectra")
    finally:
        _lib.set_knob_all("lane_reach", None)
