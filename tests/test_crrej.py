"""CPU: cosmic-ray rejection of the device-side extraction -- the law (tests/crrej_law.py) against the truth of the
CPU oracle, the Python binding and the host-side argument check.  Device side: tests/test_crrej_gpu.py.

Truth: ExposureOracle reads of the same exposure with and without cosmic rays under the same PhiloxDraws; a true hit is
a tested pixel whose difference image differs between the two by more than 1000 e- (a hit is 10 000 - 35 000 e-, what a
hit leaves in LATER intervals through the non-linearity correction is far below that).  All tested pixels of the frame
are tried: the one window is the whole frame.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import crrej_law
import extraction_law as law
import helpers
from oracle import wayne_oracle as wo
from wayne_amd import _lib, extraction, run_visit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, RN = 8.0, 20.0          # the defaults


def oracle_reads(v, **over):
    eo = helpers.oracle_generator(v)
    kw = v.frame_kwargs(0, **over)
    draws = wo.PhiloxDraws(v.seed, 0, v.detector.light_sensitive_size(v.SUBARRAY))
    return np.stack(eo.scanning_frame(threads=2, draws=draws, thrower="oracle", **helpers.oracle_kwargs(kw)))


@pytest.mark.parametrize("name", ["small256", "stare256"])
def test_the_law_finds_the_oracles_hits_and_nothing_else(name):
    v = helpers.make_visit(name)
    pl = law.Planes(v)
    S = pl.S
    on, off = oracle_reads(v), oracle_reads(v, cosmic_rate=None)
    every = slice(0, S)
    I_on = crrej_law.difference_images(on, pl, law.ALL, every)[0]
    I_off = crrej_law.difference_images(off, pl, law.ALL, every)[0]
    tested = np.zeros((S, S), dtype=bool)
    tested[crrej_law.MARGIN:S - crrej_law.MARGIN, crrej_law.MARGIN:S - crrej_law.MARGIN] = True
    hits = shielded = found = false = 0
    sum_hit = sum_left = 0.0
    for j in range(I_on.shape[0]):
        truth = tested & (np.abs(I_on[j] - I_off[j]) > 1000.0)
        flag, repl, _ = crrej_law.flags(I_on[j], K, RN)
        assert not crrej_law.flags(I_off[j], K, RN)[0].any(), "a flag on the exposure without cosmic rays, interval %d" % j
        # a true hit whose stencil holds another hit of the same interval may be shielded by it: not counted for recall
        near = np.zeros_like(truth)
        for dy, dx in ((-1, 0), (1, 0), (-2, 0), (2, 0), (0, -1), (0, 1), (0, -2), (0, 2)):
            near |= crrej_law._shift(truth.astype(np.float64), dy, dx) > 0
        alone = truth & ~near
        hits += int(truth.sum())
        shielded += int((truth & near).sum())
        found += int((flag & truth).sum())
        false += int((flag & ~truth).sum())
        assert (flag[alone]).all(), "a hit was missed in interval %d" % j
        sum_hit += float(np.abs(I_on[j] - I_off[j])[truth].sum())
        sum_left += float(np.abs(repl - I_off[j])[flag].sum())
    ratio = sum_left / sum_hit
    print("%s: %d true hits, %d flagged, %d shielded, %d false; sum|repl - clean| / sum|hit| = %.1f / %.1f = %.3g" % (
        name, hits, found, shielded, false, sum_left, sum_hit, ratio))
    assert hits >= 10 and false == 0
    assert shielded <= 0.02 * hits
    assert found >= hits - shielded
    assert sum_left <= 0.01 * sum_hit


def test_restate_without_flags_is_the_extraction_law():
    # a smooth synthetic exposure: no pixel stands out, so the rejecting law must restate the plain one exactly
    v = helpers.make_visit("small256")
    pl = law.Planes(v)
    S = pl.S
    y, x = np.mgrid[0:S, 0:S]
    ramp = 200.0 * np.exp(-0.5 * ((y - 130.0) / 30.0) ** 2) + 0.01 * x
    reads = np.stack([1000.0 + r * ramp for r in range(4)]).astype(np.float32)
    windows = [(100, 140), (110, 150), (120, 160), (20, 246)]
    got = crrej_law.restate(reads, pl, windows, (6, 26))
    want, want_sky, _, _ = law.restate(reads, pl, windows, (6, 26))
    assert not got.mask.any() and not got.n_rejected.any() and not got.undecided.any()
    assert got.spectra.tobytes() == want.tobytes() and got.sky.tobytes() == want_sky.tobytes()
    # one spike: flagged in its interval alone, replaced in its products, the rest of the frame untouched
    reads[2:, 125, 80] += 8000.0
    hit = crrej_law.restate(reads, pl, windows, (6, 26))
    assert hit.mask[125, 80] == 2 and np.count_nonzero(hit.mask) == 1
    assert list(hit.n_rejected) == [0, 1, 0, 1]
    cols = np.arange(S) != 80
    assert hit.spectra[:, cols].tobytes() == want[:, cols].tobytes()
    assert np.abs(hit.spectra[:, 80] - want[:, 80]).max() <= 0.01 * 8000.0 * 2.35      # 1 % of the spike's electrons
    assert crrej_law.mask_rows(windows, 3) == (20, 246) and crrej_law.mask_rows(windows, 3, law.ALL & ~law.LAST_READ) == (100, 160)


def test_cosmic_rejection_is_validated_and_leaves_the_extract_descriptor_alone():
    cr = extraction.CosmicRejection()
    assert (cr.k, cr.read_noise) == (8.0, 20.0)
    assert extraction.CosmicRejection(read_noise=0).read_noise == 0.0
    for bad in (dict(k=0), dict(k=-1), dict(k=float("nan")), dict(k=float("inf")), dict(read_noise=-1),
                dict(read_noise=float("nan")), dict(read_noise=float("inf"))):
        with pytest.raises(ValueError):
            extraction.CosmicRejection(**bad)
    with pytest.raises(TypeError):
        extraction.Extraction([(5, 9)] * 4, crrej=6.0)
    windows = [(5, 9), (6, 10), (7, 11), (5, 11)]
    plain, with_cr = extraction.Extraction(windows), extraction.Extraction(windows, crrej=True)
    assert plain.crrej is None and extraction.Extraction(windows, crrej=False).crrej is None
    assert (with_cr.crrej.k, with_cr.crrej.read_noise) == (8.0, 20.0)
    assert bytes(plain.desc()) == bytes(with_cr.desc())
    assert with_cr.mask_rows == (5, 11)
    assert extraction.Extraction(windows[:3] + [(0, 99)], steps=extraction.ALL & ~extraction.LAST_READ).mask_rows == (5, 11)
    opts = extraction.ExtractionOptions(crrej=extraction.CosmicRejection(k=6))
    assert opts.crrej.k == 6.0 and extraction.ExtractionOptions().crrej is None
    d = with_cr.crrej.desc()
    assert (d.k, d.read_noise_e) == (8.0, 20.0)
    # the frame's crrej= replaces the plan's; without an extraction it is an error
    args = (None, None, 0.0, 0.0, 0.0, [1.0], 0, 266)
    assert extraction.for_exposure(plain, *args, crrej=True).crrej.k == 8.0
    assert extraction.for_exposure(with_cr, *args).crrej is with_cr.crrej
    assert extraction.for_exposure(with_cr, *args, crrej=False).crrej is None
    assert extraction.for_exposure(None, *args) is None
    with pytest.raises(ValueError):
        extraction.for_exposure(None, *args, crrej=True)


def test_crrej_struct_mirrors_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wayne_hip.h"\n'
                   'int main(void) {\n  printf("%zu %zu %zu\\n", sizeof(wayne_crrej_desc), offsetof(wayne_crrej_desc, k),\n'
                   '         offsetof(wayne_crrej_desc, read_noise_e));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    size, off_k, off_rn = (int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_lib.CrrejDesc) == 16
    assert off_k == _lib.CrrejDesc.k.offset == 0 and off_rn == _lib.CrrejDesc.read_noise_e.offset == 8
    for name in ("wayne_exposure_set_crrej", "wayne_exposure_rejected", "wayne_exposure_download_crmask"):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 7


def test_cli_argument_errors():
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    with pytest.raises(SystemExit) as e:
        run_visit.run(["-p", yml, "--reject-cosmics"])
    assert "--spectra" in str(e.value)
    for k in ("0", "-3", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml, "--spectra-only", "x.npz", "--reject-cosmics=" + k])
        assert "K must be" in str(e.value)


def test_algorithmic_bytes_count_the_mask_kernel():
    S, R = 266, 3
    plan = extraction.Extraction([(100, 140), (110, 150), (120, 160), (100, 160)])
    base = extraction.algorithmic_bytes(plan, S, R)
    assert extraction.algorithmic_bytes(plan, S, R, crrej=False) == base
    more = extraction.algorithmic_bytes(plan, S, R, crrej=True)
    rows = 60
    mask_kernel = rows * S * ((R + 1) * 4 + 4 * R + 16 + 4 + 2)
    window_pixels = (40 + 40 + 40 + 60) * S
    chunks = 2 + 2 + 2 + 2
    assert more - base == mask_kernel + window_pixels * 2 + 2 * chunks * S * 4 + (R + 1) * 4
    assert extraction.algorithmic_bytes(plan, S, R, read_bytes=2, crrej=True) < more


HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include "host_plan.h"
using namespace wayne;
int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int bad = 0;
  auto expect = [&](bool ok, unsigned steps, double k, double rn, const char* what) {
    const char* why = plan::crrej_desc_error(steps, k, rn);
    if ((why == nullptr) != ok) { std::printf("WRONG %s: %s\n", what, why ? why : "accepted"); ++bad; }
  };
  expect(true, X_ALL, 8.0, 20.0, "defaults");
  expect(true, X_GAIN, 0.5, 0.0, "gain alone, rn 0");
  expect(false, X_ALL, 0.0, 20.0, "k 0");
  expect(false, X_ALL, -8.0, 20.0, "k negative");
  expect(false, X_ALL, nan, 20.0, "k nan");
  expect(false, X_ALL, inf, 20.0, "k inf");
  expect(false, X_ALL, 8.0, -1.0, "rn negative");
  expect(false, X_ALL, 8.0, nan, "rn nan");
  expect(false, X_ALL, 8.0, inf, "rn inf");
  expect(false, X_ALL & ~X_GAIN, 8.0, 20.0, "gain off");
  int lo[17] = {40, 30, 50, 10}, hi[17] = {60, 70, 90, 200}, m_lo = -1, m_hi = -1;
  plan::crrej_mask_rows(3, X_ALL, lo, hi, &m_lo, &m_hi);
  if (m_lo != 10 || m_hi != 200) { std::printf("WRONG mask rows %d %d\n", m_lo, m_hi); ++bad; }
  plan::crrej_mask_rows(3, X_ALL & ~X_LAST_READ, lo, hi, &m_lo, &m_hi);
  if (m_lo != 30 || m_hi != 90) { std::printf("WRONG mask rows without the last read %d %d\n", m_lo, m_hi); ++bad; }
  std::printf("checked\n");
  return bad ? 1 : 0;
}
"""


def test_crrej_desc_error_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "crrej_plan.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "crrej_plan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr
