"""GPU: the carried trap history (wayne_exposure_set_trap_history, k_ramp_hist, the context's trap state) against the
float64 restatement in tests/trap_history_oracle.py.

As in tests/test_traps_gpu.py an exposure with traps and its traps-off twin share every random stream, so the oracle
predicts the trapped reads and the state an exposure leaves from the twin's reads and accumulators.  Tolerances:
  * float64 variant: reads 1e-9 DN; state one float32 unit in the last place of the capacity, N_p 2^-23 (the device
    rounds its float64 occupancy to float32 once, as the oracle does);
  * float32 production chain: reads as tests/test_traps_gpu.py with R + 1 trap steps (the gap's step beside the R
    reads'), state (R + 2) N_p 2^-21 (R + 1 float32 steps and the final store);
  * a chain of exposures: exposure k starts from a state that may be k float32 units off the oracle's (the step
    contracts, so earlier differences do not grow): state (k + 1) N_p 2^-23, reads 1e-9 DN + k (N_s + N_f) 2^-23 / gain.
"""
import copy
import os

import numpy as np
import pytest

import helpers
import trap_history_oracle as tho
import trap_oracle as to
from wayne_amd import _lib, run_visit, traps as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = dict(add_dark=False, add_read_noise=False, add_non_linear=False, clip_values_det_limits=False,
             add_gain_variations=False)
ULP = 2.0 ** -23


def strong_traps(**over):
    """(tests/test_traps_gpu.py's) the default populations with large occupancies and fills"""
    return T.ChargeTraps(slow=dict(initial=300.0, orbit_fill=150.0, **over), fast=dict(initial=40.0, orbit_fill=20.0, **over))


def prepare(name, out=np.float64, traps=None, i=0, **over):
    v = helpers.make_visit(name, n_exposures=i + 1)
    kw = v.frame_kwargs(i, **over)
    pg = helpers.product_generator(v, i)
    pg.prepare(rng_mode=_lib.RNG_SPLIT, out_dtype=out, charge_traps=traps, **kw)
    eng, desc, _ = pg._prepared
    pg._prepared = None
    return v, pg, eng, desc


def run(ctx, desc, slot=0):
    ctx.upload(slot, desc)
    ctx.run_front(slot)
    acc = ctx.debug_fetch(slot, acc=True)[3]
    ctx.run_back(slot)
    return acc, ctx.download(slot).copy()


def sky_plane(v, S):
    planes = v.calibration.for_mode(v.grism.name, v.SUBARRAY, v.SAMPSEQ, v.read_times, add_initial_bias=True,
                                    detector=v.detector, flat_grism=v.grism.name, flat_shift=0)
    out = np.zeros((S, S), dtype=np.float32)
    out[5:S - 5, 5:S - 5] = planes["sky"]
    return out


def random_state(model, S, seed):
    """[S, S, 2] float32 in [0, N_p], different per pixel and population"""
    rng = np.random.RandomState(seed)
    return (rng.uniform(0.0, 1.0, (S, S, 2)) * model.array("n_traps")[None, None, :]).astype(np.float32)


def oracle(v, pg, desc, state, reads_off, acc, ct):
    S = reads_off.shape[1]
    bg = (desc.sky_ct_s * pg._read_dt).astype(np.float32)
    m = ct.traps
    return tho.exposure(state, reads_off, acc, sky_plane(v, S), bg, pg._read_dt, ct.gap_s, ct.lit, ct.fill,
                        m.array("efficiency"), m.array("n_traps"), m.array("lifetime_s"))


def border(S):
    b = np.ones((S, S), dtype=bool)
    b[to.BORDER:S - to.BORDER, to.BORDER:S - to.BORDER] = False
    return b


def assert_state(got, want, model, ulps, frac=ULP):
    N = model.array("n_traps")
    S = got.shape[0]
    for p in range(2):
        assert np.abs(got[..., p].astype(np.float64) - want[..., p]).max() <= ulps * N[p] * frac, p
    np.testing.assert_array_equal(got[border(S)].view(np.uint32), want[border(S)].view(np.uint32))


@pytest.mark.parametrize("name,lit", [("tiny", False), ("small256", False), ("stare256", True)])
def test_one_exposure_float64_against_the_oracle(name, lit):
    model = strong_traps()
    N = model.array("n_traps")
    over = dict(PLAIN, cosmic_rate=30.0)
    v, pg, eng, off_d = prepare(name, **over)
    ctx = eng.ctx
    acc, off = run(ctx, off_d)
    S = off.shape[1]
    state0 = random_state(model, S, 7)
    # a gap inside an orbit, then an orbit's start whose fill saturates some pixels
    for gap, fill in ((60.0, (0.0, 0.0)), (2800.0, tuple(0.5 * N))):
        ct = T.CarriedTraps(model, gap, lit, fill)
        _, _, _, on_d = prepare(name, traps=ct, **over)
        ctx.trap_state_upload(state0)
        acc_on, on = run(ctx, on_d)
        assert ctx.ramp_variant(0) == "k_ramp_hist<double, true, 1, false, false>"
        np.testing.assert_array_equal(acc_on, acc)           # traps draw nothing: the same charge, the same streams
        want, left, e_zero, trapped = oracle(v, pg, off_d, state0, off, acc, ct)
        inner = ~border(S)
        if fill[0] > 0:      # (the slow traps: in a dark gap the fast ones empty over 2800 s, ten lifetimes, and stay below N_f)
            full = e_zero[0][inner] == N[0]
            assert full.any() and not full.all()
        # the effect is there, far above the tolerances: a million times the reads' (`tiny` is short and faint: its
        # traps take under an electron), a thousand float32 units of the capacity in the state
        assert np.abs(want - off).max() > 1e6 * 1e-9
        for p in range(2):
            assert np.abs(left[..., p].astype(np.float64) - state0[..., p])[inner].max() > 1e3 * N[p] * ULP
        np.testing.assert_allclose(on, want, rtol=0, atol=1e-9)
        got = ctx.trap_state_download()
        assert_state(got, left, model, 1)
        np.testing.assert_array_equal(left[border(S)], state0[border(S)])


def test_production_chain_reads_and_state():
    model = strong_traps()
    ct = T.CarriedTraps(model, 60.0, False, (30.0, 5.0))
    over = dict(PLAIN, cosmic_rate=30.0)
    v, pg, eng, off_d = prepare("small256", **over)
    ctx = eng.ctx
    acc, off = run(ctx, off_d)
    S, R = off.shape[1], off.shape[0] - 1
    state0 = random_state(model, S, 11)
    want, left, _, trapped = oracle(v, pg, off_d, state0, off, acc, ct)
    assert np.abs(trapped).max() > 5.0
    # float32 reads, the plain switches: against the oracle
    _, _, _, off32_d = prepare("small256", out=np.float32, **over)
    _, _, _, on32_d = prepare("small256", out=np.float32, traps=ct, **over)
    _, off32 = run(ctx, off32_d)
    ctx.trap_state_upload(state0)
    _, on32 = run(ctx, on32_d)
    assert ctx.ramp_variant(0) == "k_ramp_hist<float, true, 1, false, false>"
    trap_tol = (R + 1) * float(model.array("n_traps").sum()) * 2.0 ** -21 / to.GAIN
    np.testing.assert_allclose(on32, want, rtol=4 * 2.0 ** -24, atol=trap_tol + 1e-3)
    np.testing.assert_allclose(off32.astype(np.float64) - on32, off - want, rtol=0,
                               atol=trap_tol + 8 * 2.0 ** -24 * np.abs(off).max())
    assert_state(ctx.trap_state_download(), left, model, R + 2, frac=2.0 ** -21)
    # every switch on: float32 and uint16 reads against the float64 variant (the bound of tests/test_modes_gpu.py); the
    # state depends on the collected charge alone, so it is the oracle's still
    _, _, _, d64 = prepare("small256", traps=ct, cosmic_rate=30.0)
    _, _, _, d32 = prepare("small256", out=np.float32, traps=ct, cosmic_rate=30.0)
    _, _, _, d16 = prepare("small256", out=np.uint16, traps=ct, cosmic_rate=30.0)
    ctx.trap_state_upload(state0)
    _, a = run(ctx, d64)
    assert ctx.ramp_variant(0) == "k_ramp_hist<double, true, 1, false, false>"
    assert_state(ctx.trap_state_download(), left, model, 1)
    ctx.trap_state_upload(state0)
    _, b = run(ctx, d32)
    assert ctx.ramp_variant(0) == "k_ramp_hist<float, true, 1, false, true>"
    state32 = ctx.trap_state_download()
    np.testing.assert_allclose(b, a, rtol=2e-7, atol=0.02)
    assert_state(state32, left, model, R + 2, frac=2.0 ** -21)
    ctx.trap_state_upload(state0)
    _, c = run(ctx, d16)
    assert ctx.ramp_variant(0) == "k_ramp_hist<unsigned short, true, 1, false, true>"
    assert c.dtype == np.uint16
    np.testing.assert_array_equal(c, np.clip(np.rint(b), 0, 65535).astype(np.uint16))
    np.testing.assert_array_equal(ctx.trap_state_download().view(np.uint32), state32.view(np.uint32))


def test_zero_efficiency_leaves_every_read_and_the_state_only_decays():
    model = T.ChargeTraps(slow=dict(efficiency=0.0), fast=dict(efficiency=0.0))
    ct = T.CarriedTraps(model, 60.0, False, (0.0, 0.0))
    for out in (np.float64, np.float32):
        v, pg, eng, off_d = prepare("small256", out=out)         # every detector switch on
        _, _, _, on_d = prepare("small256", out=out, traps=ct)
        ctx = eng.ctx
        _, off = run(ctx, off_d)
        S = off.shape[1]
        ctx.trap_state_reset((0.0, 0.0))                          # nothing held, nothing trapped: nothing released either
        _, on = run(ctx, on_d)
        assert ctx.ramp_variant(0).startswith("k_ramp_hist<")
        np.testing.assert_array_equal(on, off)
        assert not ctx.trap_state_download().any()
        state0 = random_state(model, S, 3)
        ctx.trap_state_upload(state0)
        run(ctx, on_d)
        got = ctx.trap_state_download()
        inner = ~border(S)
        assert (got[inner] <= state0[inner]).all() and (got[inner] < state0[inner]).any() and (got >= 0).all()
        # ... by the gap and the exposure, in the dark: E e^{-(gap + exptime) / tau}
        decay = np.exp(-(60.0 + float(pg._read_dt.sum())) / model.array("lifetime_s"))
        np.testing.assert_allclose(got[inner], state0[inner] * decay[None, :], rtol=1e-5, atol=1e-4)


def test_a_chain_of_four_exposures_across_an_orbit_boundary():
    model = strong_traps()
    Nsum = float(model.array("n_traps").sum())
    over = dict(PLAIN, cosmic_rate=30.0)
    v0 = helpers.make_visit("small256")
    exptime = float(v0.read_times[-1])
    t = np.array([0.0, exptime + 60.0, 5760.0, 5760.0 + exptime + 60.0]) / 86400.0
    plan = model.history_plan({"exp_start_times": t, "orbit_start_index": [0, 2]}, exptime, staring=False)
    assert plan["fill"][2].tolist() == [150.0, 20.0] and plan["gap_s"][2] > 5000.0
    state = None
    for k in range(4):
        ct = model.carried(plan, k)
        v, pg, eng, off_d = prepare("small256", i=k, **over)
        _, _, _, on_d = prepare("small256", traps=ct, i=k, **over)
        ctx = eng.ctx
        if k == 0:
            ctx.trap_state_reset(model.array("initial"))
            S = ctx.S
            state = np.empty((S, S, 2), dtype=np.float32)
            state[...] = model.array("initial").astype(np.float32)
        saved = ctx.trap_state_download()                    # the twin must not touch the state
        acc, off = run(ctx, off_d)
        np.testing.assert_array_equal(ctx.trap_state_download().view(np.uint32), saved.view(np.uint32))
        acc_on, on = run(ctx, on_d)
        np.testing.assert_array_equal(acc_on, acc)
        want, state, _, trapped = oracle(v, pg, off_d, state, off, acc, ct)
        assert np.abs(trapped).max() > 2.0
        np.testing.assert_allclose(on, want, rtol=0, atol=1e-9 + k * Nsum * ULP / to.GAIN)
        got = ctx.trap_state_download()
        if k == 0:       # the reset reaches the border too, which no exposure touches
            np.testing.assert_array_equal(got[border(S)], state[border(S)])
        assert_state(got, state, model, k + 1)


def _mini_observation(history="carried"):
    import yaml
    mini = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
    cfg = yaml.safe_load(open(os.path.join(mini, "params.yml")))
    cfg["charge_traps"] = {"history": history, "slow": {"initial": 200.0, "orbit_fill": 100.0}, "fast": {"initial": 30.0}}
    return run_visit.build_observation(cfg, base_dir=mini)


def _reads(frames, n):
    return [np.stack([r[0] for r in frames[i + 1].reads]) for i in range(n)]


def test_the_pipeline_carries_the_state_through_a_visit():
    obs = _mini_observation()
    n = len(obs.exp_start_times)
    assert n >= 4 and len(obs.visit_plan["orbit_start_index"]) >= 2
    two = _reads(obs.run_observation(write_fits=False), n)
    state_two = obs.trap_state.copy()
    assert state_two.dtype == np.float32 and state_two.shape[2] == 2
    # a second run after the reset repeats the bytes
    again = _reads(obs.run_observation(write_fits=False), n)
    for a, b in zip(again, two):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(obs.trap_state.view(np.uint32), state_two.view(np.uint32))
    # one stream
    _lib.set_knob_all("streams", 1)
    try:
        one_obs = _mini_observation()
        one = _reads(one_obs.run_observation(write_fits=False), n)
    finally:
        _lib.set_knob_all("streams", None)
    for a, b in zip(one, two):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(one_obs.trap_state.view(np.uint32), state_two.view(np.uint32))
    # the exposures one at a time on slot 0
    alone = _mini_observation()
    ctx = alone._generate_exposure(alone.exp_start_times[0], 1, write_fits=False, prepare_only=True)._prepared[0].ctx
    ctx.trap_state_reset(alone.charge_traps.array("initial"))
    for i in range(n):
        frame = alone._generate_exposure(alone.exp_start_times[i], i + 1, write_fits=False)
        np.testing.assert_array_equal(np.stack([r[0] for r in frame.reads]), two[i])
    np.testing.assert_array_equal(ctx.trap_state_download().view(np.uint32), state_two.view(np.uint32))
    # the state has left `initial` (the reset reaches the border, which no exposure touches) ...
    S = state_two.shape[0]
    assert np.abs(state_two[~border(S)][:, 0] - 200.0).max() > 1.0
    np.testing.assert_array_equal(state_two[border(S)], np.broadcast_to(np.float32([200.0, 30.0]), (int(border(S).sum()), 2)))
    # ... and the history acts: the same visit after one that left every trap full (initial_state) reads differently,
    # by more than the 0.5 DN by which tests/test_traps_gpu.py tells this visit with traps from the one without
    full = np.empty((S, S, 2), dtype=np.float32)
    full[...] = alone.charge_traps.array("n_traps").astype(np.float32)
    after = _mini_observation()
    after.setup_charge_traps(after.charge_traps, initial_state=full)
    persisted = _reads(after.run_observation(write_fits=False), n)
    assert max(np.abs(a - b).max() for a, b in zip(persisted, two)) > 0.5
    assert (after.trap_state[~border(S)][:, 0] > state_two[~border(S)][:, 0]).all()      # the slow traps remember it to the end


def test_a_carried_exposure_is_never_run_a_second_time():
    model = strong_traps()
    ct = T.CarriedTraps(model, 60.0, False, (0.0, 0.0))
    v, pg, eng, plain_d = prepare("small256", out=np.float32)
    _, _, _, on_d = prepare("small256", out=np.float32, traps=ct)
    ctx = eng.ctx
    ctx.trap_state_reset(model.array("initial"))
    ctx.upload(0, on_d)
    ctx.run(0)
    want = ctx.download(0).copy()
    want_state = ctx.trap_state_download()
    ctx.set_knob("lane_reach", 5)
    try:
        n0 = ctx.reruns
        ctx.upload(0, plain_d)
        ctx.run(0)
        ctx.download(0)
        assert ctx.reruns == n0 + 1              # the knob does make a plain exposure of this descriptor run twice
        ctx.trap_state_reset(model.array("initial"))
        ctx.upload(0, on_d)
        ctx.run(0)
        got = ctx.download(0).copy()
        ctx.synchronize()
        assert ctx.reruns == n0 + 1              # ... and the carried one not
    finally:
        ctx.set_knob("lane_reach", None)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ctx.trap_state_download().view(np.uint32), want_state.view(np.uint32))


class _Hist(object):
    def __init__(self, gap_s=60.0, lit=False, fill=(0.0, 0.0)):
        self.gap_s, self.lit, self.fill = gap_s, lit, fill


def test_refusals_and_clearing():
    model = strong_traps()
    et = T.ExposureTraps(model)
    v, pg, eng, desc = prepare("small256", out=np.float32)
    _, _, _, trap_d = prepare("small256", out=np.float32, traps=et)
    ctx = eng.ctx
    ctx.upload(0, trap_d)
    ctx.run(0)
    trapped = ctx.download(0).copy()
    trap_name = ctx.ramp_variant(0)
    assert trap_name.startswith("k_ramp_trap<float, true, 1, false, ")
    # download and history before any reset or upload: the context of a configuration no other test of this file uses
    _, _, other, other_d = prepare("tiny128", out=np.float32, traps=et)
    assert other.ctx is not ctx
    with pytest.raises(_lib.WayneError) as e:
        other.ctx.trap_state_download()
    assert e.value.status == _lib.E_STATE
    other.ctx.upload(0, other_d)
    with pytest.raises(_lib.WayneError) as e:
        other.ctx.set_trap_history(0, _Hist())
    assert e.value.status == _lib.E_STATE
    assert other.ctx.ramp_variant(0).startswith("k_ramp_trap<")
    # ... and without calibration the frame size is not known
    fresh = _lib.Context(0)
    with pytest.raises(_lib.WayneError) as e:
        fresh.trap_state_reset((0.0, 0.0))
    assert e.value.status == _lib.E_STATE
    fresh.close()
    ctx.trap_state_reset(model.array("initial"))
    # history without traps
    ctx.upload(0, desc)
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_trap_history(0, _Hist())
    assert e.value.status == _lib.E_STATE
    assert ctx.ramp_variant(0).startswith("k_ramp<")
    # bad descriptors: the slot stays a plain k_ramp_trap exposure
    N = model.array("n_traps")
    bad = [_Hist(gap_s=-1.0), _Hist(gap_s=float("nan")), _Hist(gap_s=float("inf")), _Hist(fill=(N[0] * 1.001, 0.0)),
           _Hist(fill=(0.0, N[1] + 1.0)), _Hist(fill=(-1.0, 0.0)), _Hist(fill=(float("nan"), 0.0))]
    for b in bad:
        ctx.upload(0, trap_d)
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_trap_history(0, b)
        assert e.value.status == _lib.E_INVALID
        assert ctx.ramp_variant(0) == trap_name
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), trapped)
    # between the two halves it is too late: the front half chose a launch sequence that may ask for a second run
    ctx.upload(0, trap_d)
    ctx.run_front(0)
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_trap_history(0, _Hist())
    assert e.value.status == _lib.E_STATE
    ctx.run_back(0)
    np.testing.assert_array_equal(ctx.download(0), trapped)
    # set, then cleared by NULL, by set_traps and by the next upload
    ctx.set_trap_history(0, _Hist())
    assert ctx.ramp_variant(0) == trap_name.replace("k_ramp_trap", "k_ramp_hist")
    ctx.set_trap_history(0, None)
    assert ctx.ramp_variant(0) == trap_name
    ctx.set_trap_history(0, _Hist())
    ctx.set_traps(0, et)
    assert ctx.ramp_variant(0) == trap_name
    ctx.set_trap_history(0, _Hist(fill=tuple(N)))              # (a fill of exactly N_p is allowed)
    assert ctx.ramp_variant(0).startswith("k_ramp_hist<")
    ctx.upload(0, trap_d)
    assert ctx.ramp_variant(0) == trap_name
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), trapped)
    # a wrong shape never reaches the library
    with pytest.raises(ValueError):
        ctx.trap_state_upload(np.zeros((ctx.S, ctx.S), dtype=np.float32))


def test_planned_mode_is_untouched():
    import test_traps_gpu as planned
    model = strong_traps()
    et = T.ExposureTraps(model, planned.table_of(model))
    over = dict(PLAIN, cosmic_rate=30.0)
    v, pg, eng, off_d = prepare("small256", **over)
    _, _, _, on_d = prepare("small256", traps=et, **over)
    ctx = eng.ctx
    ctx.trap_state_reset((1.0, 1.0))                      # a state in the context is nothing to a planned exposure
    before = ctx.trap_state_download()
    acc, off = run(ctx, off_d)
    _, on = run(ctx, on_d)
    assert ctx.ramp_variant(0) == "k_ramp_trap<double, true, 1, false, false>"
    want, trapped, _ = planned.oracle(v, pg, off_d, off, acc, et)
    assert np.abs(trapped).max() > 5.0
    np.testing.assert_allclose(on, want, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(ctx.trap_state_download().view(np.uint32), before.view(np.uint32))
