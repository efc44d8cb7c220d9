"""CPU: kLaneR16 (k_narrow.h), the reach in sigmas of an electron of k_lane whose radius is NOT refined.

k_lane draws the radius of an electron from its 16-bit half-word h as sigma sqrt(-2 ln u), u = (h + 1/2) / 2^16, and
only for h = 0 -- one electron in 65536 -- subdivides the cell with 17 more bits, u = (h' + 1/2) / 2^33.  A workgroup's
test-free tile is sized for the first kind alone, +- (kLaneR16 sigma_max + 1) px; the second kind takes a checked
deposit.  Here: the kernel's float32 arithmetic for the radius, restated in numpy over every h = 1 ... 65535, stays
below kLaneR16 as the header spells it, and kLaneR16 stays below the smallest refined radius.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    src = open(os.path.join(ROOT, "wayne_amd", "csrc", "k_narrow.h")).read()
    m = re.search(r"constexpr\s+float\s+%s\s*=\s*([0-9.]+)f\s*;" % name, src)
    assert m, name
    return np.float32(m.group(1))


def radius_in_sigmas(h, sigma):
    """sqrt(fma(c, log2(h + 0.5), c16)) / sigma with c = (-2 ln2 sigma) sigma and c16 = -16 c, every step rounded to
    float32 as in lane_body (the fma evaluated in float64 and rounded once: 24 x 24-bit products are exact there)."""
    f = np.float32
    s = f(sigma)
    c = f(f(f(-1.3862943611198906) * s) * s)
    c16 = f(f(-16.0) * c)
    lg = np.log2((h.astype(np.float32) + f(0.5)).astype(np.float64)).astype(np.float32)
    r2 = (c.astype(np.float64) * lg.astype(np.float64) + np.float64(c16)).astype(np.float32)
    return np.sqrt(r2.astype(np.float64)).astype(np.float32) / s


def test_unrefined_radius_stays_below_r16():
    r16 = header_constant("kLaneR16")
    h = np.arange(1, 65536, dtype=np.uint32)
    worst = 0.0
    for sigma in (0.05, 0.7, 1.0, 4.0, 5.5, 6.5, 6.8, 10.0):
        r = radius_in_sigmas(h, sigma)
        assert np.all(np.isfinite(r))
        assert int(np.argmax(r)) == 0                           # largest at h = 1
        worst = max(worst, float(r.max()))
    print("largest unrefined radius: %.5f sigma (kLaneR16 = %.5f)" % (worst, r16))
    assert abs(worst - 4.62275) < 2e-5                          # sqrt(2 ln (65536 / 1.5)) = 4.62275
    assert worst < float(r16)
    # the slack is three orders of magnitude above what 1-ulp log2 / sqrt and the float32 products can add
    assert float(r16) - worst > 1000 * 4 * 2.0 ** -24 * worst


def test_r16_is_below_the_smallest_refined_radius():
    r16 = header_constant("kLaneR16")
    # h = 0: u = (h' + 1/2) / 2^33 with h' < 2^17, so u < 2^-16 and R > sqrt(2 ln 65536) = 4.7096 sigma
    smallest_refined = np.sqrt(2.0 * np.log(65536.0))
    assert 4.70 < smallest_refined < 4.72
    assert float(r16) < 4.71 and float(r16) < smallest_refined
    # and the rule with the knob off covers the refined radius: sqrt(2 ln 2^34) = 6.87 sigma
    assert float(header_constant("kLaneR34")) >= np.sqrt(2.0 * 34 * np.log(2.0))
