"""CPU: the host half of the carried trap history (wayne_amd/traps.py history_plan / CarriedTraps, the YAML's
`history:` key, Observation's and the CLI's refusals) against tests/trap_history_oracle.py and tests/trap_oracle.py."""
import copy
import os

import numpy as np
import pytest
import yaml

import trap_history_oracle as tho
import trap_oracle as to
from wayne_amd import _lib, launch, run_visit, traps as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")

# cards() and digest_bytes() of two planned models, recorded on the tree before the `history` option existed
CARDS_DEFAULT = [
    ('CTRAPS', True, 'per-pixel charge trapping (ramp effect) on'), ('CTNS', 1525.38, 'slow traps: capacity (e-)'),
    ('CTETAS', 0.013318, 'slow traps: trapping efficiency'), ('CTTAUS', 16300.0, 'slow traps: lifetime (s)'),
    ('CTE0S', 0.0, 'slow traps: occupancy at the visit start (e-)'), ('CTDES', 0.0, 'slow traps: added at each orbit start (e-)'),
    ('CTNF', 162.38, 'fast traps: capacity (e-)'), ('CTETAF', 0.008407, 'fast traps: trapping efficiency'),
    ('CTTAUF', 281.463, 'fast traps: lifetime (s)'), ('CTE0F', 0.0, 'fast traps: occupancy at the visit start (e-)'),
    ('CTDEF', 0.0, 'fast traps: added at each orbit start (e-)'), ('CTGRID', 1024, 'trap start tables: points of the rate grid'),
    ('CTRATELO', 0.01, 'trap start tables: lowest non-zero rate (e-/s)'),
    ('CTRATEHI', 1000000.0, 'trap start tables: highest rate (e-/s)')]
DIGEST_DEFAULT = ("6368617267655f747261707300040000ec51b81e85d5974022c495b377468b3f0000000000d6cf400000000000000000000000000000"
                  "00005c8fc2f5284c6440e1b37570b037813fc520b07268977140000000000000000000000000000000007b14ae47e17a843f00000000"
                  "80842e41")
DIGEST_STRONG64 = ("6368617267655f747261707340000000ec51b81e85d5974022c495b377468b3f0000000000d6cf400000000000c072400000000000c0"
                   "62405c8fc2f5284c6440e1b37570b037813fc520b07268977140000000000000444000000000000034409a9999999999b93f00000000"
                   "006af840")


def strong_traps(**kw):
    return T.ChargeTraps(slow=dict(initial=300.0, orbit_fill=150.0), fast=dict(initial=40.0, orbit_fill=20.0), **kw)


def visit_plan(n_orbits=2, per_orbit=4, exptime=15.0, gap_s=60.0):
    """(tests/test_traps_gpu.py's visit_plan)"""
    t, starts = [], []
    for o in range(n_orbits):
        starts.append(len(t))
        for k in range(per_orbit):
            t.append(o * 96.0 / 1440.0 + k * (exptime + gap_s) / 86400.0)
    return {"exp_start_times": np.array(t), "orbit_start_index": starts}


@pytest.mark.parametrize("staring", [False, True])
def test_history_plan_against_a_hand_written_schedule(staring):
    m = strong_traps()
    plan = m.history_plan(visit_plan(), 15.0, staring)
    # 2 orbits x 4: exposures 75 s apart (60 s between them), the second orbit 96 min after the first
    orbit_gap = 96.0 * 60.0 - 3 * 75.0 - 15.0
    np.testing.assert_allclose(plan["gap_s"], [0.0, 60.0, 60.0, 60.0, orbit_gap, 60.0, 60.0, 60.0], rtol=0, atol=1e-6)
    assert list(plan["lit"]) == [False] + [staring] * 3 + [False] + [staring] * 3      # an orbit's gap is dark
    want_fill = np.zeros((8, 2))
    want_fill[4] = [150.0, 20.0]
    np.testing.assert_array_equal(plan["fill"], want_fill)
    # fewer exposures than the plan holds; overlapping exposures give no negative gap
    short = m.history_plan(visit_plan(), 15.0, staring, n_exposures=3)
    assert len(short["gap_s"]) == 3 and short["fill"].shape == (3, 2)
    assert (m.history_plan(visit_plan(), 100.0, staring)["gap_s"][1:4] == 0.0).all()
    c = m.carried(plan, 4)
    assert isinstance(c, T.ExposureTraps) and (c.gap_s, c.lit) == (pytest.approx(orbit_gap), False)
    np.testing.assert_array_equal(c.fill, [150.0, 20.0])
    assert T.for_exposure(c) is c


@pytest.mark.parametrize("staring", [False, True])
def test_the_two_modes_agree_for_a_pixel_at_constant_rate(staring):
    # what start_tables assumes -- the same rate in every earlier exposure -- stepped through history_plan by the oracle
    # reproduces the tables: the exact step composes, so the bound is rounding alone
    m = strong_traps()
    vp = visit_plan()
    tab = m.start_tables(vp, 15.0, staring)
    chain = tho.constant_rate_chain(m.history_plan(vp, 15.0, staring), 15.0, m.rates(), m.array("initial"),
                                    m.array("efficiency"), m.array("n_traps"), m.array("lifetime_s"))
    assert chain.shape == tab.shape
    for p in range(2):
        assert np.abs(chain[:, p] - tab[:, p]).max() <= 1e-12 * m.array("n_traps")[p]
    assert np.abs(tab[4] - tab[0]).max() > 1.0            # (the schedule moves the occupancies: the check is not empty)


@pytest.mark.parametrize("staring", [False, True])
def test_the_chain_against_a_brute_force_replay(staring):
    # the schedule and the bound of tests/test_traps_cpu.py's start-table test
    m = T.ChargeTraps(slow=dict(initial=250.0, orbit_fill=1500.0, lifetime_s=3000.0), fast=dict(initial=35.0, orbit_fill=12.0),
                      grid=64, rate_lo=1e-1, rate_hi=1e5)
    exptime, per, n_orbits = 103.0, 3, 3
    t, starts = [], []
    for o in range(n_orbits):
        starts.append(len(t))
        for k in range(per):
            t.append(o * 0.0667 + k * (exptime + 45.0) / 86400.0)
    vp = {"exp_start_times": np.array(t), "orbit_start_index": starts}
    eta, N, tau = (m.array(k) for k in ("efficiency", "n_traps", "lifetime_s"))
    f_grid = m.rates()
    chain = tho.constant_rate_chain(m.history_plan(vp, exptime, staring), exptime, f_grid, m.array("initial"), eta, N, tau)
    for j in [0, 1, 20, 40, 63]:
        ev = []
        for k in range(len(t)):
            ev.append(("mark",))
            if k + 1 == len(t):
                break
            ev.append(("lit", exptime, f_grid[j]))
            gap = (t[k + 1] - t[k]) * 86400.0 - exptime
            if (k + 1) in starts:
                ev += [("dark", gap), ("orbit",)]
            else:
                ev.append(("lit", gap, f_grid[j]) if staring else ("dark", gap))
        marks = to.replay(ev, m.array("initial")[:, None], eta[:, None], N[:, None], tau[:, None],
                          m.array("orbit_fill")[:, None], step_s=0.5)
        for k, E in enumerate(marks):
            np.testing.assert_allclose(chain[k, :, j], E[:, 0], rtol=1e-7, atol=1e-6)
    assert np.isclose(chain[starts[1], 0, 0], N[0])       # a dark pixel filled up to capacity: the clip


def test_config_parsing_cards_and_digests():
    carried = T.ChargeTraps.from_config({"history": "carried", "slow": {"initial": 10.0}})
    assert carried.history == "carried" and carried.params["slow"]["initial"] == 10.0
    assert T.ChargeTraps.from_config({"history": "planned"}).history == "planned"
    assert T.ChargeTraps.from_config({}).history == "planned"
    for bad in ("sequential", 1, ["carried"], True):
        with pytest.raises(T.ChargeTrapConfigError):
            T.ChargeTraps.from_config({"history": bad})
    with pytest.raises(T.ChargeTrapConfigError):
        T.ChargeTraps.from_config({"histroy": "carried"})
    # the CTHIST card: carried mode only
    assert ("CTHIST", "CARRIED") in [(k, v) for k, v, _ in carried.cards()]
    assert "CTHIST" not in [k for k, _, _ in T.ChargeTraps.from_config({"history": "planned"}).cards()]
    # a planned model's cards and digest: today's bytes
    assert T.ChargeTraps().cards() == CARDS_DEFAULT
    assert T.ChargeTraps.from_config({"history": "planned"}).cards() == CARDS_DEFAULT
    assert T.ChargeTraps().digest_bytes().hex() == DIGEST_DEFAULT
    assert strong_traps(grid=64, rate_lo=0.1, rate_hi=1e5).digest_bytes().hex() == DIGEST_STRONG64
    assert T.ExposureTraps(T.ChargeTraps()).digest_bytes() == bytes.fromhex(DIGEST_DEFAULT) + np.zeros((2, 1024)).tobytes()
    # the two modes, and two histories, are told apart
    assert T.ChargeTraps(history="carried") != T.ChargeTraps()
    m = T.ChargeTraps(history="carried")
    a, b = T.CarriedTraps(m, 60.0, False, (0.0, 0.0)), T.CarriedTraps(m, 61.0, False, (0.0, 0.0))
    digests = {a.digest_bytes(), b.digest_bytes(), T.CarriedTraps(m, 60.0, True, (0.0, 0.0)).digest_bytes(),
               T.CarriedTraps(m, 60.0, False, (1.0, 0.0)).digest_bytes(), T.ExposureTraps(m).digest_bytes()}
    assert len(digests) == 5
    assert a.digest_bytes() == T.CarriedTraps(m, 60.0, False, (0.0, 0.0)).digest_bytes()


def test_the_binding_mirrors_the_history_struct(tmp_path):
    import ctypes as C
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "hist.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wayne_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(wayne_trap_history_desc), offsetof(wayne_trap_history_desc, gap_s),\n'
                   '         offsetof(wayne_trap_history_desc, lit), offsetof(wayne_trap_history_desc, fill));\n  return 0;\n}\n')
    exe = str(tmp_path / "hist")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    D = _lib.TrapHistoryDesc
    assert got == [C.sizeof(D), D.gap_s.offset, D.lit.offset, D.fill.offset]


def _mini_cfg(history="carried"):
    cfg = yaml.safe_load(open(os.path.join(MINI, "params.yml")))
    cfg["charge_traps"] = {"history": history, "slow": {"initial": 200.0, "orbit_fill": 100.0}, "fast": {"initial": 30.0}}
    return cfg


def test_observation_refuses_what_a_carried_history_cannot_do():
    obs = run_visit.build_observation(_mini_cfg(), base_dir=MINI)
    assert obs.traps_carried and obs.trap_history == "carried"
    e0 = obs.exposure_traps(0)
    assert isinstance(e0, T.CarriedTraps) and e0.gap_s == 0.0 and not e0.fill.any()
    first_of_orbit_2 = int(obs.visit_plan["orbit_start_index"][1])
    np.testing.assert_array_equal(obs.exposure_traps(first_of_orbit_2).fill, [100.0, 0.0])
    with pytest.raises(ValueError, match="world"):
        obs.run_observation(rank=0, world=2, write_fits=False)
    with pytest.raises(ValueError, match="resume"):
        obs.run_observation(write_fits=False, resume=True)
    obs.optimal_profile_exposures = 2
    with pytest.raises(ValueError, match="optimal_profile_exposures"):
        obs.run_observation(write_fits=False)
    # the mode can be given to setup_charge_traps; a planned visit hands out start tables as before
    planned = run_visit.build_observation(_mini_cfg("planned"), base_dir=MINI)
    assert not planned.traps_carried and type(planned.exposure_traps(1)) is T.ExposureTraps
    planned.setup_charge_traps(planned.charge_traps, history="carried")
    assert planned.traps_carried and "CTHIST" in [k for k, _, _ in planned.charge_traps.cards()]
    with pytest.raises(ValueError):
        planned.setup_charge_traps(planned.charge_traps, history="planned", initial_state=np.zeros((138, 138, 2)))
    with pytest.raises(ValueError):
        planned.setup_charge_traps(planned.charge_traps, history="carried", initial_state=np.zeros((138, 138)))


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--ranks-per-gpu", "2"], ["--resume"]])
def test_the_cli_refuses_before_any_process_is_started(flags, tmp_path, monkeypatch):
    started = []
    monkeypatch.setattr(launch, "launch_ranks", lambda *a, **k: started.append(a) or ([0], None))
    monkeypatch.setattr(run_visit, "build_observation", lambda *a, **k: started.append(a))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    path = tmp_path / "params.yml"
    path.write_text(yaml.safe_dump(_mini_cfg()))
    with pytest.raises(SystemExit) as e:
        run_visit.run(["-p", str(path)] + flags)
    assert "carried" in str(e.value) and flags[0] in str(e.value)
    assert not started
    # the same flags with a planned history go on to the launcher / the visit
    path.write_text(yaml.safe_dump(_mini_cfg("planned")))
    try:
        run_visit.run(["-p", str(path)] + flags)
    except BaseException:
        pass
    assert started
