"""CPU: the charge-trapping model's host half (wayne_amd/traps.py) against tests/trap_oracle.py, its YAML section, FITS
cards and --resume check, the C header's wayne_trap_desc against its ctypes mirror, and the no-traps digest guard."""
import copy
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import yaml

import trap_oracle as to
from wayne_amd import _lib, exposure, run_visit, traps as T, visit
from wayne_amd.exposure_generator import ExposureGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
# visit.descriptor_digest of the mini visit's first descriptor, recorded on the tree before charge traps existed
DIGEST_WITHOUT_TRAPS = "ada2f5427249538616a40b32d67ff4f78fd7aab0"

POPS = [(T.DEFAULTS["slow"]["efficiency"], T.DEFAULTS["slow"]["n_traps"], T.DEFAULTS["slow"]["lifetime_s"]),
        (T.DEFAULTS["fast"]["efficiency"], T.DEFAULTS["fast"]["n_traps"], T.DEFAULTS["fast"]["lifetime_s"])]


@pytest.mark.parametrize("pop", [0, 1])
def test_closed_form_step_against_rk4(pop):
    eta, N, tau = POPS[pop]
    for f in [0.0, 1e-2, 1.0, 1e2, 1e4, 1e6]:
        for dt in [0.278, 7.3, 103.0]:
            for E0 in [0.0, N / 3.0, N]:
                c = eta * f / N + 1.0 / tau
                n = max(400, int(math.ceil(c * dt * 40)))
                want = to.rk4(E0, f, dt, eta, N, tau, n)
                got = T.step(E0, f, dt, eta, N, tau)
                assert abs(got - want) <= 1e-9 * max(N, 1.0), (pop, f, dt, E0, got, want)
                assert abs(got - to.exact(E0, f, dt, eta, N, tau)) <= 1e-10 * N


def _schedule(t_days, orbit_starts, exptime, f, staring):
    ev = []
    for k in range(len(t_days)):
        ev.append(("mark",))
        if k + 1 == len(t_days):
            break
        ev.append(("lit", exptime, f))
        gap = (t_days[k + 1] - t_days[k]) * 86400.0 - exptime
        if (k + 1) in orbit_starts:
            ev += [("dark", gap), ("orbit",)]
        else:
            ev.append(("lit", gap, f) if staring else ("dark", gap))
    return ev


@pytest.mark.parametrize("staring", [False, True])
@pytest.mark.parametrize("n_orbits", [1, 2, 4])
def test_start_tables_against_a_brute_force_replay(staring, n_orbits):
    fill_big = n_orbits == 4          # orbit_fill beyond the room left: the clip to n_traps
    m = T.ChargeTraps(slow=dict(initial=250.0, orbit_fill=1500.0 if fill_big else 90.0, lifetime_s=3000.0),
                      fast=dict(initial=35.0, orbit_fill=160.0 if fill_big else 12.0), grid=64, rate_lo=1e-1, rate_hi=1e5)
    exptime, per = 103.0, 3
    t, starts = [], []
    for o in range(n_orbits):
        starts.append(len(t))
        for k in range(per):
            t.append(o * 0.0667 + k * (exptime + 45.0) / 86400.0)
    plan = {"exp_start_times": np.array(t), "orbit_start_index": starts}
    tab = m.start_tables(plan, exptime, staring)
    assert tab.shape == (len(t), 2, 64)
    f_grid = m.rates()
    eta, N, tau = (m.array(k)[:, None] for k in ("efficiency", "n_traps", "lifetime_s"))
    for j in [0, 1, 20, 40, 63]:
        marks = to.replay(_schedule(t, set(starts[1:]), exptime, f_grid[j], staring), m.array("initial")[:, None], eta, N,
                          tau, m.array("orbit_fill")[:, None], step_s=0.5)
        for k, E in enumerate(marks):
            np.testing.assert_allclose(tab[k, :, j], E[:, 0], rtol=1e-7, atol=1e-6)
    assert (tab >= 0).all() and (tab <= m.array("n_traps")[None, :, None] + 1e-9).all()
    if fill_big and n_orbits > 1:
        assert np.isclose(tab[starts[1], 0, 0], m.params["slow"]["n_traps"])     # dark pixel, filled up to capacity
    if n_orbits > 1 and not staring:
        # a brighter history holds more at the zero read
        assert tab[-1, 0, 60] > tab[-1, 0, 10]


def test_default_grid_interpolates_within_its_bound():
    m = T.ChargeTraps(slow=dict(initial=100.0, orbit_fill=50.0), fast=dict(initial=20.0))
    plan = {"exp_start_times": np.array([0.0, 0.002, 0.004, 0.07, 0.072]), "orbit_start_index": [0, 3]}
    exptime = 103.0
    tab = m.start_tables(plan, exptime, staring=False)[-1]
    # the exact occupancy at any rate: the same history on a one-point grid
    def exact(f):
        one = T.ChargeTraps(slow=m.params["slow"], fast=m.params["fast"], grid=2, rate_lo=f, rate_hi=f)
        return one.start_tables(plan, exptime, staring=False)[-1][:, 1]
    G = m.grid
    h = math.log(m.rate_hi / m.rate_lo) / (G - 2)
    # the bound of linear interpolation in ln f: h^2 / 8 max |E''(ln f)|, the second derivative from the table itself
    d2 = np.abs(np.diff(tab[:, 1:], n=2, axis=1)).max() / h ** 2
    bound = h * h / 8.0 * d2 * 1.5 + 1e-9
    assert bound <= 0.05
    checks = [0.0, 3e-3, 0.5 * m.rate_lo, 0.07, 3.3, 471.0, 2.9e4, 8.1e5, 2e6, 1e9]
    got = m.interpolate(tab, np.array(checks))
    np.testing.assert_allclose(got, to.interp(tab, np.array(checks), m.rate_lo, m.rate_hi), rtol=1e-13, atol=1e-12)
    for j, f in enumerate(checks):
        if f == 0.0:
            np.testing.assert_array_equal(got[:, j], tab[:, 0])
        elif f < m.rate_lo:
            # linear in f below rate_lo: exactly between point 0 and point 1
            np.testing.assert_allclose(got[:, j], tab[:, 0] + (tab[:, 1] - tab[:, 0]) * f / m.rate_lo, rtol=1e-14)
            assert np.all(np.abs(got[:, j] - exact(f)) <= 0.05)
        elif f > m.rate_hi:
            np.testing.assert_array_equal(got[:, j], tab[:, -1])
        else:
            assert np.all(np.abs(got[:, j] - exact(f)) <= bound), (f, got[:, j], exact(f), bound)


def test_yaml_section_and_defaults():
    base = yaml.safe_load(open(os.path.join(MINI, "params.yml")))
    obs = run_visit.build_observation(copy.deepcopy(base), base_dir=MINI)
    assert obs.charge_traps is None
    cfg = copy.deepcopy(base)
    cfg["charge_traps"] = {}
    m = run_visit.build_observation(cfg, base_dir=MINI).charge_traps
    assert m == T.ChargeTraps() and m.params == T.DEFAULTS
    cfg["charge_traps"] = {"slow": {"n_traps": 1525.38, "efficiency": 0.013318, "lifetime_s": 16300.0, "initial": 0.0,
                                    "orbit_fill": 0.0},
                           "fast": {"n_traps": 162.38, "efficiency": 0.008407, "lifetime_s": 281.463, "initial": 0.0,
                                    "orbit_fill": 0.0}}
    assert run_visit.build_observation(cfg, base_dir=MINI).charge_traps == T.ChargeTraps()
    cfg["charge_traps"] = {"fast": {"lifetime_s": 100.0}}
    m = run_visit.build_observation(cfg, base_dir=MINI).charge_traps
    assert m.params["fast"]["lifetime_s"] == 100.0 and m.params["slow"] == T.DEFAULTS["slow"]
    assert m.params["fast"]["n_traps"] == T.DEFAULTS["fast"]["n_traps"]
    for bad in [{"slow": {"efficiency": 1.5}}, {"slow": {"efficiency": -0.1}}, {"fast": {"lifetime_s": 0}},
                {"fast": {"n_traps": 0.0}}, {"slow": {"initial": 2000.0}}, {"slow": {"orbit_fill": -1.0}},
                {"slow": {"n_traps": float("nan")}}, {"medium": {}}, {"slow": {"tau": 3.0}}, {"slow": "x"},
                {"slow": {"efficiency": "high"}}, ["slow"]]:
        cfg["charge_traps"] = bad
        with pytest.raises(run_visit.WFC3SimConfigError):
            run_visit.build_observation(cfg, base_dir=MINI)


def _header(traps=None):
    info = {"SUBARRAY": 128, "NSAMP": 4, "SAMPSEQ": "RAPID", "x_ref": 460.0}
    if traps is not None:
        info["charge_traps"] = traps
    return exposure.Exposure(exp_info=info).generate_science_header()


def test_cards_only_with_traps_and_the_resume_check_compares_them():
    m = T.ChargeTraps(slow=dict(initial=12.5), fast=dict(orbit_fill=3.0))
    plain, on = _header(), _header(m)
    assert not any(k.startswith("CT") for k, _, _ in plain.cards)
    assert [k for k, _, _ in plain.cards] == [k for k, _, _ in on.cards][:len(plain.cards)]
    assert on["CTRAPS"] is True
    assert (on["CTNS"], on["CTETAS"], on["CTTAUS"], on["CTE0S"], on["CTDES"]) == (1525.38, 0.013318, 16300.0, 12.5, 0.0)
    assert (on["CTNF"], on["CTETAF"], on["CTTAUF"], on["CTE0F"], on["CTDEF"]) == (162.38, 0.008407, 281.463, 0.0, 3.0)
    obs = run_visit.build_observation(yaml.safe_load(open(os.path.join(MINI, "params.yml"))), base_dir=MINI)
    assert obs._trap_cards_match(plain) and not obs._trap_cards_match(on)
    obs.setup_charge_traps(m)
    assert obs._trap_cards_match(on) and not obs._trap_cards_match(plain)
    changed = T.ChargeTraps(slow=dict(initial=12.5), fast=dict(orbit_fill=3.0, lifetime_s=280.0))
    assert not obs._trap_cards_match(_header(changed))
    # the start tables' grid is recorded and compared too
    assert (on["CTGRID"], on["CTRATELO"], on["CTRATEHI"]) == (T.GRID, T.RATE_LO, T.RATE_HI)
    for grid in (dict(grid=512), dict(rate_lo=1e-3), dict(rate_hi=1e5)):
        other = T.ChargeTraps(slow=dict(initial=12.5), fast=dict(orbit_fill=3.0), **grid)
        assert not obs._trap_cards_match(_header(other)), grid


def test_resume_regenerates_files_whose_trap_cards_differ(tmp_path):
    # exposure_file_is_whole on real files: written with the model, kept for the same model, refused for another
    from wayne_amd import fitsio
    obs = run_visit.build_observation(yaml.safe_load(open(os.path.join(MINI, "params.yml"))), base_dir=MINI)
    obs.outdir = str(tmp_path)
    m = T.ChargeTraps(fast=dict(initial=7.0))
    S = obs.SUBARRAY + 10
    e = exposure.Exposure(obs.detector, obs.grism, None, {"SUBARRAY": obs.SUBARRAY, "NSAMP": obs.NSAMP,
                                                          "SAMPSEQ": obs.SAMPSEQ, "EXPSTART": float(obs.exp_start_times[0]),
                                                          "x_ref": 460.0, "charge_traps": m})
    e.add_read(np.zeros((S, S)), {"cumulative_exp_time": 0.0, "read_exp_time": 0.0, "CRPIX1": 0})
    for r in range(obs.NSAMP - 1):
        e.add_read(np.zeros((S, S)), {"cumulative_exp_time": 1.0 + r, "read_exp_time": 1.0, "CRPIX1": 0})
    e.generate_fits(str(tmp_path), "0001_raw.fits")
    assert fitsio.scan(os.path.join(str(tmp_path), "0001_raw.fits")) is not None
    plain_ok = obs.exposure_file_is_whole(1)
    obs.setup_charge_traps(m)
    same_ok = obs.exposure_file_is_whole(1)
    obs.setup_charge_traps(T.ChargeTraps(fast=dict(initial=7.5)))
    other_ok = obs.exposure_file_is_whole(1)
    assert (plain_ok, same_ok, other_ok) == (False, True, False)


def test_trap_desc_matches_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    inc = os.path.join(ROOT, "include")
    fields = [f[0] for f in _lib.TrapDesc._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "wayne_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wayne_trap_desc));', '  printf("max %d\\n", WAYNE_MAX_TRAP_RATES);']
    for f in fields:
        lines.append('  printf("%s %%zu\\n", offsetof(wayne_trap_desc, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", exe], check=True)
    out = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == _lib.C.sizeof(_lib.TrapDesc)
    for f in fields:
        assert int(out[f]) == getattr(_lib.TrapDesc, f).offset, f
    assert int(out["max"]) == _lib.MAX_TRAP_RATES == T.MAX_GRID


def _descriptor(obs, charge_traps=None):
    gen = ExposureGenerator(obs.detector, obs.grism, obs.NSAMP, obs.SAMPSEQ, obs.SUBARRAY, calibration=obs.calibration,
                            seed=obs.seed, exposure_index=0)
    _, mid, dur, ri = gen._gen_scanning_sample_times(obs.sample_rate)
    return gen.build_descriptor(None, float(obs.x_ref[0]), float(obs.y_ref[0]), 0.0, 0.0, obs.wl, obs.stellar_flux, None,
                                obs.scan_speed, obs.sample_rate, mid, dur, ri, charge_traps=charge_traps)


def test_no_traps_keeps_the_digest():
    obs = run_visit.build_observation(yaml.safe_load(open(os.path.join(MINI, "params.yml"))), base_dir=MINI)
    d = _descriptor(obs)
    assert d._traps is None
    assert visit.descriptor_digest(d) == DIGEST_WITHOUT_TRAPS
    m = T.ChargeTraps()
    on = _descriptor(obs, m)
    assert isinstance(on._traps, T.ExposureTraps)
    np.testing.assert_array_equal(on._traps.table, m.flat_table())       # without a visit: flat at `initial`
    assert visit.descriptor_digest(on) != DIGEST_WITHOUT_TRAPS
    other = _descriptor(obs, T.ExposureTraps(m, m.flat_table() + 1.0))
    assert visit.descriptor_digest(other) != visit.descriptor_digest(on)
    # an Observation hands exposure i the table of its place in the visit
    obs.setup_charge_traps(T.ChargeTraps(slow=dict(initial=40.0)))
    exptime = obs.detector.exptime(obs.NSAMP, obs.SUBARRAY, obs.SAMPSEQ)
    tabs = obs.charge_traps.start_tables(obs.visit_plan, exptime, staring=False)
    for i in range(len(obs.exp_start_times)):
        np.testing.assert_array_equal(obs.exposure_traps(i).table, tabs[i])
