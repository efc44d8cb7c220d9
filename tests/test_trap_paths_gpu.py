"""GPU: the charge traps' paths through ramp_body (wayne_amd/csrc/k_ramp.h, TRAP / HIST) that no other test runs.

pick_ramp_trap / pick_ramp_hist can hand out 38 + 38 instantiations; read as code the traps have few distinct paths.  The
unit here is the path: each case names the path it covers and asserts the exact ctx.ramp_variant(0) string, so that a
change of the host's selection fails the case instead of re-testing another path.

Method (tests/test_traps_gpu.py, tests/test_trap_history_gpu.py): traps draw nothing, so an exposure and its traps-off
twin share every stream -- the accumulators of debug_fetch are equal to the bit, the collected charge of each interval is
recovered from the twin's float64 reads, and tests/trap_oracle.py / tests/trap_history_oracle.py predict the trapped
reads (and the state left behind).  Switches: PLAIN with cosmic_rate 30 unless a case says otherwise.

  path (k_ramp.h)                                              case that covers it
  -----------------------------------------------------------  ---------------------------------------------------------
  generic loop, `else` (direct sampler, s_tab[r][tid]):         A test_sky_branches[direct], F test_history[direct]
    chg = chg + k
  generic loop, `else if (ALIAS)`: chg = chg + k                A test_sky_branches[pieces] (SKY 2), [exact] (FAST off),
                                                                F test_history[pieces]
  generic loop, no sky at all: chg = px alone, f_bar = 0        A test_sky_branches[nosky]
    off the star (trap_start's e[0])
  chg = px BEFORE the gaussian-noise stage                      B test_noise_is_not_charge[alias|direct],
                                                                F test_history_noise_is_not_charge
  trap_start: !(f > 0), f < rate_lo, the clamp, G == 2          E test_table_ends[float64|float32 (__logf)-G8|G2]
  production chain's pipeline with traps at R mod 3 = 2, 1       D test_production_chain_other_ramp_lengths
    and a long ramp (te_s, te_f, te_0, dn over both tails)        [tiny_g102 R 2 | tiny128 R 4 | cfg3 R 14],
                                                                D test_production_chain_every_switch_on_four_reads
  float32 / uint16 stores of the generic loop (double           C test_generic_loop_float32_reads_are_rounded_float64,
    pre-pass, cast in st_out); uint16 with planned tables         C test_uint16_reads_are_quantised_float32
  k_ramp_hist's load / gap step / fill / store on the above     F test_history[...], test_history_noise_is_not_charge,
                                                                F test_history_production_chain[tiny_g102|tiny128]

(cfg3 has NSAMP 15: 14 read intervals, R mod 3 = 2, the longest ramp of a 256^2 configuration.)

Inputs found on the CPU (tests/plan_harness.py, plan_sky of host_plan.h, with the positive pixels of the 256^2 master
sky and small256's read intervals 0.278, 7.346, 7.347 s): alias_on up to sky_background = 20 e-/s, off from 22 -- the
direct cases use 25; with twelve pixels of the master sky at x 10, x 25 and x 50 (hot_calibration) the plan is alias_on
with pieces; scaled by a ramp of 0.4 ... 1.6 along x, with a 50 x 50 block of zeros off the trace (zero_calibration),
it is alias_on without pieces.

Tolerances.  float64 variants: 1e-9 DN (the project's bound for this path), and the effect is at least 1e6 times that.
float32 production chain: the bound of tests/test_traps_gpu.py, rtol 4 2^-24, atol R (N_s + N_f) 2^-21 / gain + 1e-3 DN,
and its differential form.  E adds a lookup term for the float32 table lookup: twice the worst deviation of a numpy
float32 emulation of the pre-pass and trap_start (float32 f_bar, np.log in float32, float32 u and w) from the float64
lookup on the same pixels, each pixel's deviation carried through its steps -- a start occupancy off by d moves read r by
d (1 - e^{-sum c dt}) / gain, the exact step being a contraction -- the factor of two for the hardware log differing from
numpy's float32 log by ulps.

Branch populations of E (interior pixels, from the oracle's f_bar; asserted >= 50 each), rate_lo 4.804 e-/s (the median
of the sky-only pixels), rate_hi 75.06 e-/s (the median of the pixels above ten times that).  G = 8: 2497 at f = 0, 26 672
below rate_lo, 35 534 in the middle (all six cells in use), 833 clamped.  G = 2: 2497, 26 672, and 36 367 at or above
rate_lo.  The float32 lookup figures of the run on an MI355X: profiles/README.md, "The traps' other paths".

Mutants (scripts/mutation_audit.py, each run once against this module): killed by
  trap_noise_is_charge       test_noise_is_not_charge[alias], [direct], test_history_noise_is_not_charge
  trap_direct_sky_uncharged  test_sky_branches[direct], test_history[direct]
  trap_alias_sky_uncharged   test_sky_branches[pieces], [exact], test_history[pieces]
  trap_start_clamp           test_table_ends[float64-G8], [float64-G2], [float32-G8], [float32-G2]
  trap_start_below_lo        test_table_ends[float64-G8], [float64-G2], [float32-G8], [float32-G2]
  trap_start_zero            test_table_ends[float64-G8], [float64-G2], [float32-G8], [float32-G2],
                             test_sky_branches[nosky]
"""
import collections
import math

import numpy as np
import pytest

import helpers
import test_trap_history_gpu as th
import test_traps_gpu as tp
import trap_history_oracle as tho
import trap_oracle as to
from test_traps_gpu import PLAIN, strong_traps
from wayne_amd import _lib, calibration, detector, grism, synthetic, traps as T

pytestmark = pytest.mark.gpu

OVER = dict(PLAIN, cosmic_rate=30.0)
DIRECT_SKY = 25.0            # e-/s: no alias table holds small256's 7.3 s intervals at this level (module docstring)
NOISE = dict(noise_mean=5.0, noise_std=40.0)
BOX0 = (1014 - 256) // 2     # the 256^2 sub-array's corner in the 1014^2 master sky

_cal = {}


def hot_calibration():
    """The synthetic set with twelve pixels of the 256^2 box's master sky at x 10, x 25 and x 50 of their neighbours:
    (set, y, x in box coordinates)."""
    if "hot" not in _cal:
        cal = calibration.CalibrationSet.synthetic(11)
        rng = np.random.default_rng(77)
        y, x = rng.integers(20, 236, 12), rng.integers(20, 236, 12)
        cal.sky["G141"][BOX0 + y, BOX0 + x] *= np.repeat(np.float32([10.0, 25.0, 50.0]), 4)
        _cal["hot"] = (cal, y, x)
    return _cal["hot"]


def zero_calibration():
    """The synthetic set with the 256^2 box's master sky scaled by a ramp of 0.4 ... 1.6 along x -- the sky-only pixels
    then span rate_lo / 2 ... 3 rate_lo / 2, so that the slope of the branch below rate_lo shows in float32 reads too --
    and a 50 x 50 block of exactly-zero master sky off small256's trace."""
    if "zero" not in _cal:
        cal = calibration.CalibrationSet.synthetic(11)
        cal.sky["G141"][BOX0:BOX0 + 256, BOX0:BOX0 + 256] *= np.linspace(0.4, 1.6, 256, dtype=np.float32)[None, :]
        cal.sky["G141"][BOX0 + 180:BOX0 + 230, BOX0 + 180:BOX0 + 230] = 0.0
        _cal["zero"] = cal
    return _cal["zero"]


Run = collections.namedtuple("Run", "v pg ctx desc acc reads left")
_runs = {}


def expose(name, cal=None, out=np.float64, traps=None, state=None, variant=None, **over):
    """One exposure of configuration `name` (over calibration set `cal`: None, "hot" or "zero"), one upload per run.
    `variant`: what ctx.ramp_variant(0) must say (required with traps).  `state`: the trap state uploaded before a
    carried exposure; what it leaves comes back as `left`.  Exposures without a carried history are run once and kept."""
    assert (variant is not None) == (traps is not None)
    key = (name, cal, np.dtype(out).str, None if traps is None else traps.digest_bytes(), tuple(sorted(over.items())))
    if state is None and key in _runs:
        return _runs[key]
    cal_set = hot_calibration()[0] if cal == "hot" else zero_calibration() if cal == "zero" else None
    assert cal in (None, "hot", "zero")
    if cal_set is None:
        v, pg, eng, desc = tp.prepare(name, out=out, traps=traps, **over)
    else:
        v = synthetic.Visit(name, detector.WFC3_IR(), grism.G141(cal_set), cal_set)
        pg = helpers.product_generator(v, 0)
        pg.prepare(rng_mode=_lib.RNG_SPLIT, out_dtype=out, charge_traps=traps, **v.frame_kwargs(0, **over))
        eng, desc, _ = pg._prepared
        pg._prepared = None
    ctx = eng.ctx
    if state is not None:
        ctx.trap_state_upload(state)
    acc, reads = tp.run(ctx, desc)
    name_ran = ctx.ramp_variant(0)
    if traps is None:
        assert name_ran.startswith("k_ramp<") or name_ran.startswith("k_ramp_wide<"), name_ran
    else:
        assert name_ran == variant, name_ran
    r = Run(v, pg, ctx, desc, acc, reads, ctx.trap_state_download() if state is not None else None)
    if state is None:
        _runs[key] = r
    return r


def planned(model=None):
    model = model or strong_traps()
    return T.ExposureTraps(model, tp.table_of(model))


def inner(S):
    return ~th.border(S)


def say(*a):
    print("[trap paths]", *a, flush=True)


def f32_bounds(model, R, off):
    """(rtol, atol, atol of the differential form) of tests/test_traps_gpu.py's float32 production chain."""
    trap_tol = R * float(model.array("n_traps").sum()) * 2.0 ** -21 / to.GAIN
    return 4 * 2.0 ** -24, trap_tol + 1e-3, trap_tol + 8 * 2.0 ** -24 * np.abs(off).max()


# ---------------------------------------------------------------------------------------------------------------
# A. where the collected charge comes from in the generic loop
# ---------------------------------------------------------------------------------------------------------------
SKY_CASES = {
    #          calibration, overrides, the instantiation
    "direct": (None, dict(sky_background=DIRECT_SKY), "k_ramp_trap<double, true, 0, false, false>"),
    "pieces": ("hot", dict(), "k_ramp_trap<double, true, 2, false, false>"),
    "exact": (None, dict(exact_samplers=True), "k_ramp_trap<double, false, 1, false, false>"),
    "nosky": (None, dict(sky_background=0), "k_ramp_trap<double, true, 0, false, false>"),
}


@pytest.mark.parametrize("case", list(SKY_CASES))
def test_sky_branches(case):
    cal, extra, variant = SKY_CASES[case]
    et = planned()
    off = expose("small256", cal, **OVER, **extra)
    on = expose("small256", cal, traps=et, variant=variant, **OVER, **extra)
    np.testing.assert_array_equal(on.acc, off.acc)
    want, trapped, dN = tp.oracle(off.v, off.pg, off.desc, off.reads, off.acc, et)
    S = off.reads.shape[1]
    effect = np.abs(want - off.reads).max()
    say("A", case, "effect %.3g DN, worst |on - want| %.3g DN" % (effect, np.abs(on.reads - want).max()))
    assert effect >= 1e6 * 1e-9
    if case == "pieces":
        _, hy, hx = hot_calibration()
        assert inner(S)[hy + 5, hx + 5].any()                       # the hot pixels are light-sensitive ones ...
        assert dN[:, hy + 5, hx + 5].max() > 16.0 * 10              # ... drew far more than one piece's mean (kSkyPiece)
        assert np.abs(want - off.reads)[:, hy + 5, hx + 5].max() > 1e-3      # ... and their traps took some of it
    if case == "nosky":
        fbar = tho.mean_rate(off.acc, tp.sky_plane(off.v, S), (off.desc.sky_ct_s * off.pg._read_dt).astype(np.float32),
                             off.pg._read_dt)
        dark = inner(S) & (fbar == 0.0)
        assert dark.sum() > 1000 and (inner(S) & (fbar > 0)).sum() > 1000
        assert not dN[:, dark].any()
    np.testing.assert_allclose(on.reads, want, rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------
# B. the gaussian-noise stage is not charge
# ---------------------------------------------------------------------------------------------------------------
NOISE_CASES = {
    "alias": (dict(), "k_ramp_trap<double, true, 1, %s, false>"),
    "direct": (dict(sky_background=DIRECT_SKY), "k_ramp_trap<double, true, 0, %s, false>"),
}


def noise_runs(case):
    extra, variant = NOISE_CASES[case]
    et = planned()
    off_p = expose("small256", **OVER, **extra)
    on_p = expose("small256", traps=et, variant=variant % "false", **OVER, **extra)
    off_n = expose("small256", **OVER, **extra, **NOISE)
    on_n = expose("small256", traps=et, variant=variant % "true", **OVER, **extra, **NOISE)
    return off_p, on_p, off_n, on_n


@pytest.mark.parametrize("case", list(NOISE_CASES))
def test_noise_is_not_charge(case):
    off_p, on_p, off_n, on_n = noise_runs(case)
    assert (NOISE["noise_std"] * off_p.pg._read_dt).min() >= 10.0   # electrons: charged to the traps they would show
    np.testing.assert_array_equal(on_n.acc, off_n.acc)
    np.testing.assert_array_equal(on_n.acc, off_p.acc)              # (the noise has its own stream: STAGE_NOISE)
    moved = np.abs(on_n.reads - on_p.reads).max()
    effect = np.abs(off_p.reads - on_p.reads).max()
    worst = np.abs((off_n.reads - on_n.reads) - (off_p.reads - on_p.reads)).max()
    say("B", case, "noise moved the reads by %.3g DN, traps by %.3g DN, identity to %.3g DN" % (moved, effect, worst))
    assert moved > 1.0 and effect >= 1e6 * 1e-9
    np.testing.assert_allclose(off_n.reads - on_n.reads, off_p.reads - on_p.reads, rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------
# C. store types
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["direct", "alias_noise"])
def test_generic_loop_float32_reads_are_rounded_float64(case):
    # tests/test_modes_gpu.py::test_float32_reads_are_rounded_float64_reads, with traps: the generic loop's arithmetic
    # (the double trap pre-pass included) does not depend on the reads' type, st_out alone casts
    et = planned()
    if case == "direct":
        extra = dict(sky_background=DIRECT_SKY)
        a = expose("small256", traps=et, variant="k_ramp_trap<double, true, 0, false, false>", **OVER, **extra)
        b = expose("small256", out=np.float32, traps=et, variant="k_ramp_trap<float, true, 0, false, false>", **OVER, **extra)
    else:
        a = expose("small256", traps=et, variant="k_ramp_trap<double, true, 1, true, false>", **OVER, **NOISE)
        b = expose("small256", out=np.float32, traps=et, variant="k_ramp_trap<float, true, 1, true, false>", **OVER, **NOISE)
    assert b.reads.dtype == np.float32
    np.testing.assert_array_equal(b.acc, a.acc)
    np.testing.assert_array_equal(b.reads.view(np.uint32), a.reads.astype(np.float32).view(np.uint32))


U16_CASES = {
    "planned": (OVER, "k_ramp_trap<%s, true, 1, false, false>"),
    "every_switch": (dict(cosmic_rate=30.0), "k_ramp_trap<%s, true, 1, false, true>"),
    "direct": (dict(OVER, sky_background=DIRECT_SKY), "k_ramp_trap<%s, true, 0, false, false>"),
}


@pytest.mark.parametrize("case", list(U16_CASES))
def test_uint16_reads_are_quantised_float32(case):
    over, variant = U16_CASES[case]
    et = planned()
    f = expose("small256", out=np.float32, traps=et, variant=variant % "float", **over)
    q = expose("small256", out=np.uint16, traps=et, variant=variant % "unsigned short", **over)
    plain = expose("small256", out=np.float32, **over)
    assert q.reads.dtype == np.uint16
    np.testing.assert_array_equal(q.acc, f.acc)
    assert np.abs(plain.reads.astype(np.float64) - f.reads).max() > 1.0      # the traps did something
    want = np.clip(np.rint(f.reads), 0, 65535).astype(np.uint16)
    assert (want[1:, 5:-5, 5:-5] > 0).mean() > 0.5 and (want < 65535).mean() > 0.99      # (the ADC's range is in use, not its ends)
    np.testing.assert_array_equal(q.reads, want)


# ---------------------------------------------------------------------------------------------------------------
# D. the production chain's pipeline at other ramp lengths
# ---------------------------------------------------------------------------------------------------------------
def rapid_traps():
    # (RAPID ramps last 0.12 - 0.45 s and collect tens of electrons a pixel: a larger efficiency makes them show)
    return strong_traps(efficiency=0.25)


@pytest.mark.parametrize("name,R", [("tiny_g102", 2), ("tiny128", 4), ("cfg3", 14)])
def test_production_chain_other_ramp_lengths(name, R):
    model = strong_traps() if name == "cfg3" else rapid_traps()
    et = planned(model)
    off = expose(name, **OVER)
    assert off.reads.shape[0] == R + 1
    want, trapped, dN = tp.oracle(off.v, off.pg, off.desc, off.reads, off.acc, et)
    off32 = expose(name, out=np.float32, **OVER)
    on32 = expose(name, out=np.float32, traps=et, variant="k_ramp_trap<float, true, 1, false, false>", **OVER)
    np.testing.assert_array_equal(on32.acc, off.acc)
    rtol, atol, atol_diff = f32_bounds(model, R, off.reads)
    effect = np.abs(want - off.reads).max()
    say("D", name, "R %d: effect %.3g DN, atol %.3g DN, worst |on32 - want| %.3g DN, differential %.3g DN (atol %.3g)" % (
        R, effect, atol, np.abs(on32.reads - want).max(),
        np.abs((off32.reads.astype(np.float64) - on32.reads) - (off.reads - want)).max(), atol_diff))
    assert effect > 100 * atol                                       # the effect is there, far above the tolerance
    np.testing.assert_allclose(on32.reads, want, rtol=rtol, atol=atol)
    np.testing.assert_allclose(off32.reads.astype(np.float64) - on32.reads, off.reads - want, rtol=0, atol=atol_diff)


def test_production_chain_every_switch_on_four_reads():
    et = planned(rapid_traps())
    a = expose("tiny128", traps=et, variant="k_ramp_trap<double, true, 1, false, false>", cosmic_rate=30.0)
    b = expose("tiny128", out=np.float32, traps=et, variant="k_ramp_trap<float, true, 1, false, true>", cosmic_rate=30.0)
    c = expose("tiny128", out=np.float32, cosmic_rate=30.0)
    assert b.reads.shape[0] == 5
    assert np.abs(c.reads.astype(np.float64) - b.reads).max() > 1.0        # the traps did something
    say("D every switch: worst |f32 - f64| %.3g DN, median %.3g DN" % (np.abs(b.reads - a.reads).max(),
                                                                       np.median(np.abs(b.reads - a.reads))))
    np.testing.assert_allclose(b.reads, a.reads, rtol=2e-7, atol=0.02)
    assert np.median(np.abs(b.reads - a.reads)) < 1e-3


# ---------------------------------------------------------------------------------------------------------------
# E. the start table's ends
# ---------------------------------------------------------------------------------------------------------------
def start_f32(table, acc, sky_plane, bg, read_dt, rate_lo, rate_hi):
    """trap_start<float> after the production chain's pre-pass, restated in numpy float32: [2, S, S] float64."""
    f4 = np.float32
    G = table.shape[1]
    t = table.astype(f4)
    sum_bg = 0.0
    for b in bg:
        sum_bg += float(f4(b))
    sum_dt = float(np.sum([float(d) for d in read_dt]))
    sky_px = np.where(sky_plane > 0, sky_plane, f4(0)).astype(f4)
    e_acc = acc.sum(axis=0).astype(f4)
    # fmaf(sky_px, sum_bg_f, e_acc) * inv_sum_dt_f: the fused multiply-add rounds once
    f = (sky_px.astype(np.float64) * float(f4(sum_bg)) + e_acc.astype(np.float64)).astype(f4) * f4(1.0 / sum_dt)
    assert f.dtype == f4
    lo = f4(rate_lo)
    u_scale = f4((G - 2) / math.log(rate_hi / rate_lo) if G > 2 else 0.0)
    u = (np.log(np.where(f > 0, f, lo)) - f4(math.log(rate_lo))) * u_scale
    assert u.dtype == f4
    i = np.clip(u.astype(np.int64), 0, max(G - 3, 0))
    w = u - i.astype(f4)
    out = np.empty((2,) + f.shape)
    for p in range(2):
        e = t[p]
        a, b = e[np.minimum(1 + i, G - 1)], e[np.minimum(2 + i, G - 1)]
        v = np.where(u < f4(G - 2), a + (b - a) * w, e[G - 1])
        v = np.where(f < lo, e[0] + (e[1] - e[0]) * (f / lo), v)
        v = np.where(f > 0, v, e[0])
        assert v.dtype == f4
        out[p] = v
    return out


@pytest.mark.parametrize("G", [8, 2], ids=["G8", "G2"])
@pytest.mark.parametrize("loop", ["float64", "float32"])
def test_table_ends(loop, G):
    base = strong_traps()
    N = base.array("n_traps")
    off = expose("small256", "zero", **OVER)
    S, R = off.reads.shape[1], off.reads.shape[0] - 1
    sky = tp.sky_plane(off.v, S)
    bg = (off.desc.sky_ct_s * off.pg._read_dt).astype(np.float32)
    fbar = tho.mean_rate(off.acc, sky, bg, off.pg._read_dt)
    live = inner(S)
    unlit = live & (off.acc.sum(axis=0) == 0)
    sky_only = unlit & (sky > 0)
    sky_med = float(np.median(fbar[sky_only]))
    star = live & (fbar > 10.0 * sky_med)
    rate_lo = sky_med
    rate_hi = float(np.median(fbar[star])) if G > 2 else rate_lo
    model = T.ChargeTraps(slow=base.params["slow"], fast=base.params["fast"], grid=G, rate_lo=rate_lo, rate_hi=rate_hi)
    table = np.random.RandomState(5).uniform(0.0, 1.0, (2, G)) * N[:, None]          # non-monotone: an index off by one shows
    et = T.ExposureTraps(model, table)
    # the four branches of trap_start, from the oracle's f_bar (a condition on the inputs)
    zero = live & ~(fbar > 0)
    below = live & (fbar > 0) & (fbar < rate_lo)
    if G > 2:
        u = (np.log(np.where(fbar > 0, fbar, rate_lo)) - math.log(rate_lo)) * ((G - 2) / math.log(rate_hi / rate_lo))
        clamped = live & (fbar >= rate_lo) & ~(u < G - 2)
        middle = live & (fbar >= rate_lo) & (u < G - 2)
        cells = np.unique(u[middle].astype(int)).size
    else:
        clamped, middle, cells = live & (fbar >= rate_lo), np.zeros_like(live), 0
    counts = dict(zero=int(zero.sum()), below=int(below.sum()), middle=int(middle.sum()), clamped=int(clamped.sum()))
    say("E G=%d rate_lo %.4g rate_hi %.4g e-/s, branch populations %r, cells of the middle branch in use %d" % (
        G, rate_lo, rate_hi, counts, cells))
    for k, n in counts.items():
        assert n >= 50 or (G == 2 and k == "middle"), counts
    assert G == 2 or cells == G - 2

    want, trapped, dN = tp.oracle(off.v, off.pg, off.desc, off.reads, off.acc, et)
    assert np.abs(want - off.reads).max() >= 1e6 * 1e-9
    for k, m in dict(zero=zero, below=below, middle=middle, clamped=clamped).items():
        if m.any():                                                   # every branch's pixels show the traps
            assert np.abs(want - off.reads)[:, m].max() >= 1e6 * 1e-9, k
    if loop == "float64":                                             # the generic loop: trap_start<double>
        on = expose("small256", "zero", traps=et, variant="k_ramp_trap<double, true, 1, false, false>", **OVER)
        np.testing.assert_array_equal(on.acc, off.acc)
        say("E G=%d float64: worst |on - want| %.3g DN" % (G, np.abs(on.reads - want).max()))
        np.testing.assert_allclose(on.reads, want, rtol=0, atol=1e-9)
        return
    # the production chain: the float32 lookup (hardware log)
    off32 = expose("small256", "zero", out=np.float32, **OVER)
    on32 = expose("small256", "zero", out=np.float32, traps=et, variant="k_ramp_trap<float, true, 1, false, false>", **OVER)
    np.testing.assert_array_equal(on32.acc, off.acc)
    rtol, atol, atol_diff = f32_bounds(model, R, off.reads)
    dev = np.abs(start_f32(table, off.acc, sky, bg, off.pg._read_dt, rate_lo, rate_hi) - to.interp_fast(table, fbar, rate_lo, rate_hi))
    eta, tau = model.array("efficiency"), model.array("lifetime_s")
    lookup = 0.0
    for p in range(2):
        x = sum((eta[p] / N[p] * (dN[r] / off.pg._read_dt[r]) + 1.0 / tau[p]) * off.pg._read_dt[r] for r in range(R))
        lookup += float((dev[p] * -np.expm1(-np.maximum(x, 0.0)))[live].max()) / to.GAIN
    worst = np.abs(on32.reads - want).max()
    say("E G=%d float32: emulated lookup deviation %.3g e- (slow) %.3g e- (fast), through the steps %.3g DN; bound %.3g DN + "
        "rtol; observed worst |on32 - want| %.3g DN, beyond rtol %.3g DN" % (
            G, dev[0][live].max(), dev[1][live].max(), lookup, atol + 2 * lookup, worst,
            np.maximum(np.abs(on32.reads - want) - rtol * np.abs(want), 0.0).max()))
    np.testing.assert_allclose(on32.reads, want, rtol=rtol, atol=atol + 2 * lookup)
    np.testing.assert_allclose(off32.reads.astype(np.float64) - on32.reads, off.reads - want, rtol=0,
                               atol=atol_diff + 2 * lookup)


# ---------------------------------------------------------------------------------------------------------------
# F. the carried history on these paths
# ---------------------------------------------------------------------------------------------------------------
HISTORIES = ((60.0, 0.0), (2800.0, 0.5))      # a gap inside an orbit; an orbit's start whose fill (x N_p) saturates pixels


@pytest.mark.parametrize("case", ["direct", "pieces"])
def test_history(case):
    cal, extra, variant = SKY_CASES[case]
    variant = variant.replace("k_ramp_trap", "k_ramp_hist")
    model = strong_traps()
    N = model.array("n_traps")
    off = expose("small256", cal, **OVER, **extra)
    S = off.reads.shape[1]
    state0 = th.random_state(model, S, 7)
    for gap, fill in HISTORIES:
        ct = T.CarriedTraps(model, gap, False, tuple(fill * N))
        on = expose("small256", cal, traps=ct, state=state0, variant=variant, **OVER, **extra)
        np.testing.assert_array_equal(on.acc, off.acc)
        want, left, e_zero, trapped = th.oracle(off.v, off.pg, off.desc, state0, off.reads, off.acc, ct)
        if fill > 0:
            full = e_zero[0][inner(S)] == N[0]
            assert full.any() and not full.all()
        assert np.abs(want - off.reads).max() >= 1e6 * 1e-9
        for p in range(2):
            assert np.abs(left[..., p].astype(np.float64) - state0[..., p])[inner(S)].max() > 1e3 * N[p] * th.ULP
        say("F", case, "gap %g: worst |on - want| %.3g DN" % (gap, np.abs(on.reads - want).max()))
        np.testing.assert_allclose(on.reads, want, rtol=0, atol=1e-9)
        th.assert_state(on.left, left, model, 1)
        np.testing.assert_array_equal(left[th.border(S)], state0[th.border(S)])


def test_history_noise_is_not_charge():
    model = strong_traps()
    N = model.array("n_traps")
    off_p = expose("small256", **OVER)
    off_n = expose("small256", **OVER, **NOISE)
    S = off_p.reads.shape[1]
    state0 = th.random_state(model, S, 7)
    for gap, fill in HISTORIES:
        ct = T.CarriedTraps(model, gap, False, tuple(fill * N))
        on_p = expose("small256", traps=ct, state=state0, variant="k_ramp_hist<double, true, 1, false, false>", **OVER)
        on_n = expose("small256", traps=ct, state=state0, variant="k_ramp_hist<double, true, 1, true, false>", **OVER, **NOISE)
        np.testing.assert_array_equal(on_n.acc, off_p.acc)
        want, left, _, _ = th.oracle(off_p.v, off_p.pg, off_p.desc, state0, off_p.reads, off_p.acc, ct)
        np.testing.assert_allclose(on_p.reads, want, rtol=0, atol=1e-9)          # (the noise-free run: held to the oracle)
        th.assert_state(on_p.left, left, model, 1)
        assert np.abs(on_n.reads - on_p.reads).max() > 1.0 and np.abs(off_p.reads - on_p.reads).max() >= 1e6 * 1e-9
        np.testing.assert_allclose(off_n.reads - on_n.reads, off_p.reads - on_p.reads, rtol=0, atol=1e-9)
        np.testing.assert_array_equal(on_n.left.view(np.uint32), on_p.left.view(np.uint32))


@pytest.mark.parametrize("name,R", [("tiny_g102", 2), ("tiny128", 4)])
def test_history_production_chain(name, R):
    model = rapid_traps()
    ct = T.CarriedTraps(model, 60.0, False, (30.0, 5.0))
    off = expose(name, **OVER)
    assert off.reads.shape[0] == R + 1
    S = off.reads.shape[1]
    state0 = th.random_state(model, S, 11)
    want, left, _, trapped = th.oracle(off.v, off.pg, off.desc, state0, off.reads, off.acc, ct)
    off32 = expose(name, out=np.float32, **OVER)
    on32 = expose(name, out=np.float32, traps=ct, state=state0, variant="k_ramp_hist<float, true, 1, false, false>", **OVER)
    np.testing.assert_array_equal(on32.acc, off.acc)
    rtol, atol, atol_diff = f32_bounds(model, R, off.reads)
    effect = np.abs(want - off.reads).max()
    say("F production", name, "R %d: effect %.3g DN, atol %.3g DN, worst |on32 - want| %.3g DN" % (
        R, effect, atol, np.abs(on32.reads - want).max()))
    assert effect > 100 * atol
    np.testing.assert_allclose(on32.reads, want, rtol=rtol, atol=atol)
    np.testing.assert_allclose(off32.reads.astype(np.float64) - on32.reads, off.reads - want, rtol=0, atol=atol_diff)
    th.assert_state(on32.left, left, model, R + 2, frac=2.0 ** -21)
