"""GPU: what every slot-taking entry point of the library refuses, and in which words.

Called through ctx._L / ctx._h: the Python wrappers refuse some of these cases before the library is asked.  One context
of its own (no slot of it has been fetched before), configuration tiny.  The texts are those of
wayne_amd/csrc/wayne_hip.hip; the rows are (entry point, the arguments behind the slot, `who` of "<who>: slot", the text
of a slot that was never uploaded).  Nothing here is a tolerance: codes and texts are compared as they are, bytes as bytes."""
import ctypes as C

import numpy as np
import pytest

import helpers
from wayne_amd import _lib, engine

pytestmark = pytest.mark.gpu

OUT = object()          # a result pointer: valid memory of this test's own, null in the rows that ask for null
NEVER = 200             # a slot this test never uploads
NOT_UP = "slot not uploaded"
NO_EX = "no extraction set for the slot"
NO_OPT = "no optimal extraction set for the slot"
NO_REJ = "no rejection set for the slot"
NO_PROF = "no profile delivery set for the slot"

# (entry point, arguments behind the slot, who, text of a slot never uploaded)
ENTRIES = [
    ("run", (), "run", NOT_UP),
    ("run_checked", (), "run", NOT_UP),
    ("run_front", (), "run", NOT_UP),
    ("run_back", (), "run", "run_back: run_front first"),
    ("ramp_variant", (OUT, 64), None, NOT_UP),
    ("status", (OUT,), None, NOT_UP),
    ("download", (OUT,), None, NOT_UP),
    ("fetch_async", (), None, NOT_UP),
    ("wait", (OUT,), None, "fetch_async first"),
    ("debug_fetch", (None, None, None, None), None, NOT_UP),
    ("debug_fetch_source", (0, None, None, None), "debug_fetch", NOT_UP),
    ("debug_boxes", (OUT, OUT, OUT), None, NOT_UP),
    ("debug_depth", (OUT,), None, "no depth matrix in this slot"),
    ("set_sources", (None, 0), None, NOT_UP),
    ("set_limb_darkening", (None, 0), None, NOT_UP),
    ("set_spots", (None, 0, 0), None, NOT_UP),
    ("set_traps", (None,), None, NOT_UP),
    ("set_trap_history", (None,), None, NOT_UP),
    ("set_extraction", (None,), None, NOT_UP),
    ("set_crrej", (None,), None, NO_EX),
    ("set_channels", (None,), None, NO_EX),
    ("set_variance", (None,), None, NO_EX),
    ("set_optimal", (None,), None, "no variances set for the slot"),
    ("fetch_spectra_async", (), None, NOT_UP),
    ("wait_spectra", (OUT, OUT), None, NOT_UP),
    ("download_spectra", (OUT, OUT), None, NOT_UP),
    ("rejected", (OUT,), None, NO_REJ),
    ("channels", (OUT,), None, "no channels set for the slot"),
    ("variances", (OUT, OUT, OUT), None, "no variances set for the slot"),
    ("optimal", (OUT, OUT), None, NO_OPT),
    ("set_optimal_channels", (1,), None, "the slot needs channels and the optimal extraction"),
    ("optimal_channels", (OUT, OUT), None, "no optimal channels set for the slot"),
    ("deliver_profile", (1,), None, NO_OPT),
    ("set_optimal_profile", (None, None), None, NO_OPT),
    ("set_optimal_profile_tagged", (None, None, 0), "set_optimal_profile", NO_OPT),
    ("fetch_profile", (), None, NO_PROF),
    ("profile", (OUT, OUT), None, NO_PROF),
    ("download_crmask", (OUT,), None, NO_REJ),
    ("set_fits", (1,), None, NOT_UP),
    ("fetch_fits_async", (), None, NOT_UP),
    ("wait_fits", (OUT,), None, NOT_UP),
    ("download_fits", (OUT,), None, NOT_UP),
    ("set_expected", (1,), None, NOT_UP),
    ("download_expected", (OUT,), None, NOT_UP),
    ("set_rampfit", (None,), None, NOT_UP),
    ("download_rampfit", (OUT, OUT, OUT), None, NOT_UP),
    ("set_ima", (None,), None, NOT_UP),
    ("download_ima", (OUT,), None, NOT_UP),
    ("set_ipc", (None,), None, NOT_UP),
]
# an uploaded and run slot with no option set: (entry point, text)
NO_OPTION = [
    ("download_spectra", NO_EX), ("download_crmask", NO_REJ), ("download_fits", "no FITS words set for the slot"),
    ("download_expected", "no expected image set for the slot"), ("download_rampfit", "no ramp fit set for the slot"),
    ("download_ima", "no calibrated reads set for the slot"),
    ("fetch_fits_async", "no FITS words set for the slot"), ("fetch_spectra_async", NO_EX), ("fetch_profile", NO_PROF),
    ("wait", "fetch_async first"), ("wait_spectra", NO_EX), ("wait_fits", "no FITS words set for the slot"),
]
# a slot with the extraction, FITS words, the ramp fit and the calibrated reads set, before any run or fetch
BEFORE_RUN = [
    ("download_rampfit", "run first"), ("download_ima", "run first"),
    ("wait_spectra", "fetch_spectra_async first"), ("wait_fits", "fetch_fits_async first"),
]


class Caller(object):
    """Calls wayne_exposure_<name>(ctx, slot, ...) with the row's arguments: OUT becomes a pointer of the argument's own
    type into one scratch block (large enough for any product of configuration tiny), or null."""

    def __init__(self, ctx):
        self.L, self.h = ctx._L, ctx._h
        self.block = np.zeros(1 << 21, dtype=np.uint8)
        self.text = C.create_string_buffer(128)

    def __call__(self, name, slot, args, null=False):
        sym = "wayne_exposure_" + name
        types = _lib.SYMBOLS[sym][1][2:]
        assert len(types) == len(args), sym
        real = []
        for t, a in zip(types, args):
            if a is not OUT:
                real.append(a)
            elif null:
                real.append(None)
            elif t is C.c_char_p:
                real.append(self.text)
            else:
                real.append(C.cast(self.block.ctypes.data, t))
        return getattr(self.L, sym)(self.h, slot, *real)

    def last(self):
        return self.L.wayne_last_error(self.h).decode()


def test_every_slot_entry_point_refuses_in_its_own_words():
    v = helpers.make_visit("tiny")
    eng = engine.Engine(0, v.grism, v.detector, v.calibration, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    try:
        ctx = eng.ctx
        call = Caller(ctx)
        gen = helpers.product_generator(v, 0)
        plain = gen.build_descriptor(eng, out_dtype=np.float32, **v.frame_kwargs(0))
        full = helpers.product_generator(v, 0).build_descriptor(eng, out_dtype=np.float32, extraction=True, device_fits=True,
                                                                ramp_fit=True, ima="counts", **v.frame_kwargs(0))
        ctx.upload(7, plain)
        ctx.run_checked(7)
        want = ctx.download(7).copy()
        assert want[-1].max() > 5

        # slots outside 0 .. 255
        for bad in (-1, 256):
            assert call.L.wayne_exposure_upload(call.h, bad, C.byref(plain)) == _lib.E_INVALID
            assert call.last() == "upload: slot"
            for name, args, who, _ in ENTRIES:
                assert call(name, bad, args) == _lib.E_INVALID, (name, bad)
                assert call.last() == "%s: slot" % (who or name), (name, bad)
            assert call.L.wayne_exposure_device_reads(call.h, bad) is None
        # a slot never uploaded
        for name, args, who, text in ENTRIES:
            assert call(name, NEVER, args) == _lib.E_STATE, name
            assert call.last() == (text if ": " in text else "%s: %s" % (who or name, text)), name
        # an uploaded and run slot with no option set
        rows = {name: args for name, args, _, _ in ENTRIES}
        for name, text in NO_OPTION:
            assert call(name, 7, rows[name]) == _lib.E_STATE, name
            assert call.last() == "%s: %s" % (name, text), name
        # options set, nothing run or fetched
        ctx.upload(8, full)
        assert ctx.has_rampfit(8) and ctx.has_ima(8) and ctx.has_fits(8)
        for name, text in BEFORE_RUN:
            assert call(name, 8, rows[name]) == _lib.E_STATE, name
            assert call.last() == "%s: %s" % (name, text), name
        # a null result pointer: refused without a word -- the last error stays
        assert call("run", -1, ()) == _lib.E_INVALID
        assert call.L.wayne_exposure_upload(call.h, 7, None) == _lib.E_INVALID
        checked = [(name, args) for name, args, _, _ in ENTRIES if OUT in args]
        assert len(checked) == 20
        for name, args in checked:
            for slot in (7, 8):
                assert call(name, slot, args, null=True) == _lib.E_INVALID, name
                assert call.last() == "run: slot", name
        # ... and the slots are as they were
        ctx.run_checked(7)
        np.testing.assert_array_equal(ctx.download(7).view(np.uint32), want.view(np.uint32))
        ctx.run_checked(8)
        np.testing.assert_array_equal(ctx.download(8).view(np.uint32), want.view(np.uint32))
    finally:
        eng.close()
