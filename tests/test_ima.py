"""CPU: the calibrated reads -- the payload's layout against its formula, the law (tests/ima_law.py) against the laws it
borrows from on CPU-oracle reads, the Python binding, the host-side argument check, the refusals and the FITS file.
Device side: tests/test_ima_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import extraction_law
import helpers
import ima_law as law
import rampfit_law
from oracle import wayne_oracle as wo
from wayne_amd import _lib, exposure, fitsio, ima, run_visit, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 15])
@pytest.mark.parametrize("S", [74, 138, 266, 522, 1024])
def test_the_layout_is_the_formula(S, R):
    L = _lib.load()
    sci, dq, imset = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    assert L.wayne_ima_layout(S, R, C.byref(sci), C.byref(dq), C.byref(imset)) == 0
    n = S * S
    want_sci, want_dq = -(-4 * n // 2880) * 2880, -(-2 * n // 2880) * 2880
    assert (sci.value, dq.value, imset.value) == (want_sci, want_dq, 2 * want_sci + want_dq) == law.strides(S)
    lay = ima.layout(S, R)
    assert (lay.sci_stride, lay.dq_stride, lay.imset_stride, lay.nbytes) == (want_sci, want_dq, imset.value, (R + 1) * imset.value)
    # every section starts 16-byte aligned; the int16 plane ends on a whole 16-byte vector on the full array alone
    assert want_sci % 16 == 0 and want_dq % 16 == 0 and (n % 8 == 0) == (S == 1024) and n % 4 == 0
    assert L.wayne_ima_layout(S, R, None, None, None) == 0


def test_the_layout_refuses_what_has_none():
    L = _lib.load()
    out = [C.c_size_t(0) for _ in range(3)]
    for S, R in ((74, 0), (74, 16), (74, -1), (75, 3), (0, 3), (-74, 3)):
        assert L.wayne_ima_layout(S, R, *[C.byref(o) for o in out]) == _lib.E_INVALID, (S, R)
        with pytest.raises(ValueError):
            ima.layout(S, R)
    assert ima.layout(1024, 15).nbytes == 16 * (2 * 4196160 + 2099520)          # 168 MB at the metric's configuration


# ---- the law against the laws it borrows from, on CPU-oracle reads ---------------------------------------------------
_oracle = {}


def oracle_reads(E, cosmic):
    key = (E, cosmic)
    if key not in _oracle:
        v = helpers.make_visit("stare16_128", E=E)
        eo = helpers.oracle_generator(v)
        kw = v.frame_kwargs(0, cosmic_rate=11.0 if cosmic else None, ssv_generator=None)
        draws = wo.PhiloxDraws(v.seed, 0, v.detector.light_sensitive_size(v.SUBARRAY))
        reads = np.stack(eo.scanning_frame(threads=2, draws=draws, thrower="oracle", **helpers.oracle_kwargs(kw)))
        _oracle[key] = (v, reads, extraction_law.Planes(v))
    return _oracle[key]


def test_consecutive_reads_differ_by_the_extractions_interval_term():
    # e_{j+1} - e_j against (L_{j+1} - L_j) g, which extraction_law sums over a window: a window of one row is the term
    # itself.  The two round differently -- e_{j+1} and e_j are rounded before the subtraction, the extraction's
    # difference before the product -- by at most 4 * 2^-53 (|e_{j+1}| + |e_j|): derived, each side has two roundings.
    v, reads, pl = oracle_reads(2e7, True)
    R, S = reads.shape[0] - 1, reads.shape[-1]
    want = law.restate(reads, pl, "counts")
    worst = 0.0
    for y in (5, 37, 64, 70, S - 6):
        spectra, _, _, _ = extraction_law.restate(reads, pl, [(y, y + 1)] * (R + 1), (0, 1), steps=law.LINEARISE | law.DARK | law.GAIN)
        for j in range(R):
            d = want.e[j + 1, y] - want.e[j, y]
            bound = 2.0 ** -51 * (np.abs(want.e[j + 1, y]) + np.abs(want.e[j, y]))
            assert (np.abs(d - spectra[j]) <= bound).all(), (y, j)
            worst = max(worst, float((np.abs(d - spectra[j]) / np.maximum(bound, 1e-300)).max()))
    print("e_{j+1} - e_j against the extraction's interval term: worst difference %.3f of the bound" % worst)
    assert np.abs(want.e[R]).max() > 1e3                     # (not a comparison of zeros)
    # ... and the float32 planes are those electrons, rounded once
    inner = (slice(None), slice(5, -5), slice(5, -5))
    assert (want.sci[inner] == want.e[inner].astype(np.float32)).all() and not want.sci[0].any() and not want.err[0].any()
    assert not want.sci[:, :5].any() and not want.err[:, :, -5:].any() and not want.dq[:, :5].any()


def test_saturation_is_the_ramp_fits():
    v, reads, pl = oracle_reads(1.2e8, False)
    R = reads.shape[0] - 1
    fit = rampfit_law.restate(reads, pl)
    want = law.restate(reads, pl)
    K = (fit.word >> 16).astype(np.int64)
    assert (want.K[5:-5, 5:-5] == K[5:-5, 5:-5]).all()
    rate_dq, _, _ = rampfit_law.derived(fit.word, pl.dt)
    in_rate = (rate_dq & 256) != 0
    in_last = (want.dq[R] & 256) != 0
    inner = np.zeros(K.shape, dtype=bool)
    inner[5:-5, 5:-5] = True
    print("stare16_128 at 1.2e8: %d pixels with 256 in the rate image's DQ and in the last read's" % int(in_last.sum()))
    assert in_last.sum() >= 100 and (in_rate[inner] == in_last[inner]).all()
    # read k carries 256 exactly when k > K (K >= 1 here: read 0 is never flagged)
    for k in range(R + 1):
        assert (((want.dq[k] & 256) != 0)[inner] == (k > K)[inner]).all(), k
    assert (K[inner] >= 1).all() and not want.dq[0].any()
    # a saturated zero read flags every read, its own included; a NaN is not below saturation
    r2 = reads[:, :20, :20].astype(np.float64).copy()
    r2[0, 8, 8] = 70000.0
    r2[3, 9, 9] = np.nan
    small = types.SimpleNamespace(lin=[p[:20, :20] for p in pl.lin], dark=pl.dark[:, :20, :20], gain=pl.gain[:20, :20], dt=pl.dt)
    w2 = law.restate(r2, small)
    assert (w2.dq[:, 8, 8] == 256).all() and not w2.dq[:3, 9, 9].any() and (w2.dq[3:, 9, 9] == 256).all()
    assert np.isnan(w2.sci[3, 9, 9]) and np.isnan(w2.err[3, 9, 9]) and np.isfinite(w2.sci[4, 9, 9])


def test_reads_behind_a_jump_carry_8192():
    v, reads, pl = oracle_reads(2e7, True)
    R = reads.shape[0] - 1
    fit = rampfit_law.restate(reads, pl)
    assert (fit.jump != 0).sum() >= 5
    want = law.restate(reads, pl, jump=fit.word)              # (the word: the law takes its low half)
    none = law.restate(reads, pl)
    assert not (none.dq & 8192).any()
    for k in range(R + 1):
        behind = np.zeros(fit.jump.shape, dtype=bool)
        for j in range(k):
            behind |= ((fit.jump >> np.uint32(j)) & 1).astype(bool)
        assert (((want.dq[k] & 8192) != 0) == behind).all(), k
    assert not (want.dq[0] & 8192).any() and ((want.dq[R] & 8192) != 0).sum() == (fit.jump != 0).sum()
    assert (want.sci.view(np.uint32) == none.sci.view(np.uint32)).all()      # the flags change no sample
    # the rate is the counts over t_k, the error likewise, rounded once
    counts = law.restate(reads, pl, "counts")
    for k in range(1, R + 1):
        assert (want.sci[k, 5:-5, 5:-5] == (counts.e[k, 5:-5, 5:-5] / counts.t[k]).astype(np.float32)).all()
    assert np.isclose(counts.t[R], pl.dt.sum()) and counts.t[0] == 0.0


def test_the_payload_is_the_file_order():
    rs = np.random.RandomState(2)
    S, R = 74, 2
    w = law.Law(rs.normal(0, 100, (R + 1, S, S)).astype(np.float32), rs.uniform(1, 2, (R + 1, S, S)).astype(np.float32),
                rs.choice([0, 256, 8192, 8448], (R + 1, S, S)).astype(np.int16), None, None, None)
    buf = law.payload(w)
    sci_stride, dq_stride, imset = law.strides(S)
    assert buf.size == 3 * imset
    # the last read first
    assert (buf[:4 * S * S].view(">f4") == w.sci[2].ravel()).all()
    assert (buf[2 * imset + 2 * sci_stride:][:2 * S * S].view(">i2") == w.dq[0].ravel()).all()
    sci, err, dq, rest = law.sections(buf, S, R)
    assert (sci == w.sci).all() and (err == w.err).all() and (dq == w.dq).all() and not rest.any()
    assert rest.size == 3 * (2 * (sci_stride - 4 * S * S) + dq_stride - 2 * S * S)
    law.assert_parity(buf, w, "the law against itself")
    p = ima.Payload(buf, ima.layout(S, R))
    for k in range(R + 1):
        assert (p.sci(k) == w.sci[k]).all() and (p.err(k) == w.err[k]).all() and (p.dq(k) == w.dq[k]).all()
        assert p.sci(k).dtype == np.dtype(">f4") and p.dq(k).dtype == np.dtype(">i2") and p.sci(k).base is not None
        assert np.shares_memory(p.sci(k), buf) and np.shares_memory(p.dq(k), buf) and np.shares_memory(p.piece(k, "ERR"), buf)
    with pytest.raises(IndexError):
        p.sci(R + 1)
    with pytest.raises(ValueError):
        ima.Payload(buf[:-1], ima.layout(S, R))
    # what parity refuses: one flipped bit of a sample, a flag, a byte of padding, the imsets in read order
    for at in (5, sci_stride + 9, 2 * sci_stride + 3, 4 * S * S + 1, imset - 1):
        bad = buf.copy()
        bad[at] ^= 1
        with pytest.raises(AssertionError):
            law.assert_parity(bad, w, "outside")
    with pytest.raises(AssertionError):
        law.assert_parity(buf.reshape(3, imset)[::-1].reshape(-1).copy(), w, "read order")


# ---- the binding, the validator, the refusals ------------------------------------------------------------------------
def test_ima_struct_mirrors_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    fields = [f[0] for f in _lib.ImaDesc._fields_]
    assert fields == ["steps", "units", "read_noise_e", "saturation_dn"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wayne_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(wayne_ima_desc));\n' +
                   "".join('  printf(" %%zu", offsetof(wayne_ima_desc, %s));\n' % f for f in fields) +
                   '  printf(" %d %d\\n", WAYNE_IMA_RATE, WAYNE_IMA_COUNTS);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.ImaDesc) == 24
    assert got[1:5] == [getattr(_lib.ImaDesc, f).offset for f in fields] == [0, 4, 8, 16]
    assert got[5:] == [ima.RATE, ima.COUNTS] == [1, 2]
    header = open(os.path.join(ROOT, "include", "wayne_hip.h")).read()
    for name in ("wayne_ima_layout", "wayne_exposure_set_ima", "wayne_exposure_download_ima", "wayne_ima_profile"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name) and ("int %s(" % name) in header
    assert _lib.ABI_VERSION == 7 and "#define WAYNE_ABI_VERSION 7" in header


HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include "host_plan.h"
using namespace wayne;
int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const unsigned three = X_LINEARISE | X_DARK | X_GAIN;
  int bad = 0;
  auto expect = [&](bool ok, unsigned steps, int units, double rn, double sat, const char* what) {
    const char* why = plan::ima_desc_error(steps, units, rn, sat);
    if ((why == nullptr) != ok) { std::printf("WRONG %s: %s\n", what, why ? why : "accepted"); ++bad; }
  };
  expect(true, three, 1, 20.0, 65000.0, "defaults");
  expect(true, three, 2, 20.0, 65000.0, "counts");
  expect(true, X_GAIN, 1, 1e-3, 1.0, "gain alone");
  expect(true, X_GAIN | X_DARK, 2, 20.0, 1e9, "dark, no linearise");
  expect(false, X_LINEARISE | X_DARK, 1, 20.0, 65000.0, "gain off");
  expect(false, 0u, 1, 20.0, 65000.0, "no step");
  expect(false, three | X_SKY, 1, 20.0, 65000.0, "sky bit");
  expect(false, three | X_LAST_READ, 1, 20.0, 65000.0, "last-read bit");
  expect(false, three | (1u << 31), 1, 20.0, 65000.0, "high bit");
  expect(false, three, 0, 20.0, 65000.0, "unit 0");
  expect(false, three, 3, 20.0, 65000.0, "unit 3");
  expect(false, three, -1, 20.0, 65000.0, "unit -1");
  expect(false, three, 1, 0.0, 65000.0, "rn 0");
  expect(false, three, 1, -1.0, 65000.0, "rn negative");
  expect(false, three, 1, nan, 65000.0, "rn nan");
  expect(false, three, 1, inf, 65000.0, "rn inf");
  expect(false, three, 1, 20.0, 0.0, "sat 0");
  expect(false, three, 1, 20.0, -5.0, "sat negative");
  expect(false, three, 1, 20.0, nan, "sat nan");
  expect(false, three, 1, 20.0, inf, "sat inf");
  expect(false, three, 1, 20.0, -inf, "sat -inf");
  size_t sci = 0, dq = 0, imset = 0;
  if (!plan::ima_layout(74, 3, &sci, &dq, &imset) || sci != 23040 || dq != 11520 || imset != 57600) { std::printf("WRONG layout 74\n"); ++bad; }
  if (!plan::ima_layout(1024, 15, &sci, &dq, &imset) || sci != 4196160 || dq != 2099520) { std::printf("WRONG layout 1024\n"); ++bad; }
  if (plan::ima_layout(74, 16, &sci, &dq, &imset) || plan::ima_layout(74, 0, &sci, &dq, &imset) || plan::ima_layout(75, 3, &sci, &dq, &imset) ||
      !plan::ima_layout(74, 3, nullptr, nullptr, nullptr)) { std::printf("WRONG layout refusals\n"); ++bad; }
  std::printf("checked\n");
  return bad ? 1 : 0;
}
"""


def test_ima_desc_error_and_layout_in_a_program_of_their_own(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "ima_plan.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "ima_plan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr


def test_options_are_validated_and_descriptors_carry_them():
    d = ima.Ima()
    assert (d.units, d.read_noise, d.saturation_dn, d.linearise, d.dark) == ("rate", 20.0, 65000.0, True, True)
    assert d.steps == 7 and ima.Ima(linearise=False).steps == 6 and ima.Ima(dark=False).steps == 5
    c = ima.Ima("counts", 13.0, 3e4).desc()
    assert isinstance(c, _lib.ImaDesc) and (c.steps, c.units, c.read_noise_e, c.saturation_dn) == (7, 2, 13.0, 3e4)
    assert ima.Ima("rate").desc().units == 1
    for bad in (dict(units="dn"), dict(units=1), dict(units=None), dict(read_noise=0.0), dict(read_noise=-1.0),
                dict(read_noise=float("nan")), dict(read_noise=float("inf")), dict(saturation_dn=0.0),
                dict(saturation_dn=-3.0), dict(saturation_dn=float("nan")), dict(saturation_dn=float("inf"))):
        with pytest.raises(ValueError):
            ima.Ima(**bad)
    assert ima.as_ima(None) is None and ima.as_ima(False) is None
    assert ima.as_ima(True).units == "rate" and ima.as_ima(d) is d and ima.as_ima("counts").units == "counts"
    assert ima.as_ima("rate").units == "rate"
    with pytest.raises(ValueError):
        ima.as_ima("yes")
    with pytest.raises(TypeError):
        ima.as_ima(3.0)
    assert "counts" in repr(ima.Ima("counts"))
    # the descriptor carries it beside the C struct, whose bytes stay as they are
    v = helpers.make_visit("tiny")
    gen = helpers.product_generator(v, 0)
    plain = gen.build_descriptor(None, **v.frame_kwargs(0))
    asked = gen.build_descriptor(None, ima=True, **v.frame_kwargs(0))
    own = gen.build_descriptor(None, ima=d, ramp_fit=True, **v.frame_kwargs(0))
    assert plain._ima is None and asked._ima.units == "rate" and own._ima is d and own._ramp_fit is not None
    with pytest.raises(TypeError):
        gen.build_descriptor(None, ima=3.0, **v.frame_kwargs(0))
    assert ima.ima_filename("0007_raw.fits") == "0007_ima.fits" and ima.ima_filename("x.fits") == "x_ima.fits"
    assert exposure.Exposure().ima is None


def test_refusals():
    ima.refuse_combinations(None, resume=True, device_fits=True, spectra_only=True)      # nothing asked: nothing refused
    ima.refuse_combinations(True)
    for what in ("resume", "device_fits", "spectra_only"):
        with pytest.raises(ValueError) as e:
            ima.refuse_combinations("counts", **{what: True})
        assert "ima: not together with " + what in str(e.value)


def test_cli_argument_errors():
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    for bad in ("dn", "RATE", "1"):
        with pytest.raises(SystemExit):
            run_visit.run(["-p", yml, "--ima", bad])
    for unit in ([], ["rate"], ["counts"]):
        for other, what in ((["--resume"], "resume"), (["--device-fits"], "device_fits"), (["--spectra-only", "x.npz"], "spectra_only")):
            with pytest.raises(ValueError) as e:
                run_visit.run(["-p", yml, "--ima"] + unit + other)
            assert "ima: not together with " + what in str(e.value)


# ---- the file --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", ["rate", "counts"])
def test_the_ima_file_reads_back(tmp_path, units):
    v = helpers.make_visit("tiny")
    gen = helpers.product_generator(v, 0)
    gen.build_descriptor(None, **v.frame_kwargs(0))
    S, R = 74, v.NSAMP - 1
    frame = gen._fill_exposure(np.zeros((R + 1, S, S), dtype=np.float32))
    with pytest.raises(ValueError):
        ima.write_fits(str(tmp_path / "none_ima.fits"), frame)                          # no payload on the exposure yet
    rs = np.random.RandomState(11)
    w = law.Law(rs.normal(0, 100, (R + 1, S, S)).astype(np.float32), rs.uniform(1, 2, (R + 1, S, S)).astype(np.float32),
                rs.choice([0, 256, 8192, 8448], (R + 1, S, S)).astype(np.int16), None, None, None)
    opt = ima.Ima(units, read_noise=17.0, saturation_dn=6e4, dark=False)
    frame.ima = ima.Payload(law.payload(w), ima.layout(S, R), opt)
    path = ima.write_fits(str(tmp_path / "0001_ima.fits"), frame)
    raw_path = frame.generate_fits(str(tmp_path), "0001_raw.fits")
    hdus, raw = fitsio.read(path), fitsio.read(raw_path)
    assert len(hdus) == len(raw) == 1 + 5 * v.NSAMP
    assert [h.name for h in hdus] == [h.name for h in raw]
    p = hdus[0].header
    assert (p["IMAUNIT"], p["IMARN"], p["IMASAT"], p["IMALIN"], p["IMADARK"]) == (units.upper(), 17.0, 6e4, True, False)
    assert hdus[0].data is None
    for key in raw[0].header.keys():
        if key not in ("DATE", "SIM-TIME", "COMMENT", "HISTORY", ""):
            assert p[key] == raw[0].header[key], key
    dt = np.diff(np.concatenate([[0.0], v.read_times]))
    t = law.times(dt)
    for r in range(v.NSAMP):
        at = 1 + 5 * (v.NSAMP - 1 - r)
        sci, err, dq, samp, time = hdus[at:at + 5]
        assert [h.name for h in (sci, err, dq, samp, time)] == ["SCI", "ERR", "DQ", "SAMP", "TIME"]
        assert [h.header["BITPIX"] for h in (sci, err, dq)] == [-32, -32, 16] and samp.data is None and time.data is None
        assert samp.header["NAXIS"] == 0 and time.header["NAXIS"] == 0
        for h, rh in zip((sci, err, dq, samp, time), raw[at:at + 5]):
            assert h.header["EXTVER"] == rh.header["EXTVER"] == v.NSAMP - r
        for key in ("SAMPNUM", "SAMPTIME", "DELTATIM", "CRPIX1"):
            assert sci.header[key] == raw[at].header[key], key
        assert sci.header["SAMPNUM"] == r and sci.header["BUNIT"] == ("ELECTRONS/S" if units == "rate" else "ELECTRONS")
        assert samp.header["PIXVALUE"] == (1 if r else 0) and time.header["PIXVALUE"] == t[r]
        assert sci.header["SAMPTIME"] == (float(v.read_times[r - 1]) if r else 0.0)
        assert (sci.data.view(np.uint32) == w.sci[r].astype(">f4").view(np.uint32)).all() and (err.data == w.err[r]).all()
        assert (dq.data == w.dq[r]).all() and dq.data.dtype == np.dtype(">i2")
    # the data sections are the payload's bytes, padding included and zero
    blob = open(path, "rb").read()
    first = blob.find(frame.ima.piece(R, "SCI").tobytes())
    assert first > 0 and first % 2880 == 0
    sci_stride = frame.ima.layout.sci_stride
    assert not any(blob[first + 4 * S * S:first + sci_stride]) and len(blob) % 2880 == 0
    assert not [m for m in os.listdir(str(tmp_path)) if m.endswith(".part")]
    # a payload of another exposure's shape is refused
    frame.ima = ima.Payload(np.zeros(ima.layout(S, R - 1).nbytes, dtype=np.uint8), ima.layout(S, R - 1), opt)
    with pytest.raises(ValueError):
        ima.write_fits(str(tmp_path / "short_ima.fits"), frame)


def test_full3_is_the_configuration_the_issue_names():
    cfg = synthetic.CONFIGS["full3"]
    assert (cfg["SUBARRAY"], cfg["SAMPSEQ"], cfg["NSAMP"]) == (1024, "RAPID", 3) and cfg["K"] <= 8 and 1e5 <= cfg["E"] <= 1e6
    v = helpers.make_visit("full3")
    assert extraction_law.Planes(v).S == 1024 and len(v.read_times) == 2
