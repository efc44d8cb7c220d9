"""GPU: per-pixel charge trapping (wayne_exposure_set_traps, k_ramp_trap) against the float64 restatement of the model
in tests/trap_oracle.py.

Traps draw nothing, so an exposure with traps and the same exposure without them share every random stream: the
collected charge of each read interval is recovered from the traps-off reads (consecutive differences x gain), the
accumulators from debug_fetch, and the oracle then predicts the trapped reads.  Tolerances (stated per test):
  * float64 variant: 1e-9 DN (fp64 throughout; the recovered charge carries ~1e-11 DN of rounding);
  * float32 production chain: its own float32 rounding -- 4 ulp of the read, plus the trap state's float32 steps
    (R x (N_s + N_f) x 2^-21 e- over the gain);
  * every detector switch on: the production-vs-float64 bound of tests/test_modes_gpu.py (rtol 2e-7, atol 0.02 DN).
"""
import os
import types

import numpy as np
import pytest

import helpers
import trap_oracle as to
from wayne_amd import _lib, run_visit, traps as T
from wayne_amd.sources import Contaminant

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = dict(add_dark=False, add_read_noise=False, add_non_linear=False, clip_values_det_limits=False,
             add_gain_variations=False)


def strong_traps(**over):
    """The default populations, with occupancies at the zero read that depend on the rate (a visit's history)."""
    return T.ChargeTraps(slow=dict(initial=300.0, orbit_fill=150.0, **over), fast=dict(initial=40.0, orbit_fill=20.0, **over))


def visit_plan(n_orbits=2, per_orbit=4, exptime=15.0, gap_s=60.0):
    t, starts = [], []
    for o in range(n_orbits):
        starts.append(len(t))
        for k in range(per_orbit):
            t.append(o * 96.0 / 1440.0 + k * (exptime + gap_s) / 86400.0)
    return {"exp_start_times": np.array(t), "orbit_start_index": starts}


def table_of(model, i=5, staring=False):
    return model.start_tables(visit_plan(), 15.0, staring)[i]


def prepare(name, out=np.float64, traps=None, contaminants=None, i=0, rng_mode=_lib.RNG_SPLIT, **over):
    v = helpers.make_visit(name, n_exposures=i + 1)
    kw = v.frame_kwargs(i, **over)
    pg = helpers.product_generator(v, i)
    pg.prepare(rng_mode=rng_mode, out_dtype=out, charge_traps=traps, contaminants=contaminants, **kw)
    eng, desc, _ = pg._prepared
    pg._prepared = None
    return v, pg, eng, desc


def run(ctx, desc, slot=0):
    """upload (+ the descriptor's sources / traps), front half, accumulators, back half -> (acc, reads)."""
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


def oracle(v, pg, desc, reads_off, acc, et):
    S = reads_off.shape[1]
    bg = (desc.sky_ct_s * pg._read_dt).astype(np.float32)
    m = et.traps
    return to.trapped_reads(reads_off, acc, sky_plane(v, S), bg, pg._read_dt, et.table, m.rate_lo, m.rate_hi,
                            m.array("efficiency"), m.array("n_traps"), m.array("lifetime_s"))


@pytest.mark.parametrize("with_contaminant", [False, True])
def test_exact_differential_against_the_oracle(with_contaminant):
    model = strong_traps()
    et = T.ExposureTraps(model, table_of(model))
    over = dict(PLAIN, cosmic_rate=30.0)
    v, pg, eng, plain = prepare("small256", **over)
    ctx = eng.ctx
    cont = None
    if with_contaminant:     # a neighbour's charge is collected, so it is trapped too
        wl, fl = plain._keep[0], plain._keep[1]
        cont = [Contaminant(18.0, -30.0, wl.copy(), fl * 0.3, 1)]
    _, _, _, off_d = prepare("small256", contaminants=cont, **over)
    _, _, _, on_d = prepare("small256", contaminants=cont, traps=et, **over)
    acc, off = run(ctx, off_d)
    assert ctx.ramp_variant(0).startswith("k_ramp")
    acc_on, on = run(ctx, on_d)
    assert ctx.ramp_variant(0) == "k_ramp_trap<double, true, 1, false, false>"
    np.testing.assert_array_equal(acc_on, acc)           # traps draw nothing: the same charge, the same streams
    want, trapped, dN = oracle(v, pg, off_d, off, acc, et)
    assert np.abs(trapped).max() > 5.0                    # the effect is there, far above the tolerance
    np.testing.assert_allclose(on, want, rtol=0, atol=1e-9)
    # the float32 production chain on the same exposure: within its own rounding
    _, _, _, off32_d = prepare("small256", out=np.float32, contaminants=cont, **over)
    _, _, _, on32_d = prepare("small256", out=np.float32, contaminants=cont, traps=et, **over)
    _, off32 = run(ctx, off32_d)
    _, on32 = run(ctx, on32_d)
    assert ctx.ramp_variant(0) == "k_ramp_trap<float, true, 1, false, false>"
    R = off.shape[0] - 1
    trap_tol = R * float(model.array("n_traps").sum()) * 2.0 ** -21 / to.GAIN
    np.testing.assert_allclose(on32, want, rtol=4 * 2.0 ** -24, atol=trap_tol + 1e-3)
    np.testing.assert_allclose(off32.astype(np.float64) - on32, off - want, rtol=0,
                               atol=trap_tol + 8 * 2.0 ** -24 * np.abs(off).max())


def test_zero_efficiency_leaves_every_read_bit_for_bit():
    model = T.ChargeTraps(slow=dict(efficiency=0.0), fast=dict(efficiency=0.0))
    for out in (np.float64, np.float32):
        v, pg, eng, off_d = prepare("small256", out=out)         # every detector switch on
        _, _, _, on_d = prepare("small256", out=out, traps=model)
        ctx = eng.ctx
        _, off = run(ctx, off_d)
        _, on = run(ctx, on_d)
        assert ctx.ramp_variant(0).startswith("k_ramp_trap<")
        np.testing.assert_array_equal(on, off)


def test_production_trap_variant_against_the_float64_one_with_every_switch_on():
    model = strong_traps()
    et = T.ExposureTraps(model, table_of(model))
    v, pg, eng, d64 = prepare("small256", traps=et)
    _, _, _, d32 = prepare("small256", out=np.float32, traps=et)
    ctx = eng.ctx
    _, a = run(ctx, d64)
    _, b = run(ctx, d32)
    assert ctx.ramp_variant(0).startswith("k_ramp_trap<float, true, 1, false, ")
    _, _, _, plain = prepare("small256", out=np.float32)
    _, c = run(ctx, plain)
    assert np.abs(c.astype(np.float64) - b).max() > 1.0        # the traps did something
    np.testing.assert_allclose(b, a, rtol=2e-7, atol=0.02)
    assert np.median(np.abs(b - a)) < 1e-3


def _mini_observation(traps_cfg):
    import copy
    import yaml
    mini = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
    cfg = yaml.safe_load(open(os.path.join(mini, "params.yml")))
    cfg["charge_traps"] = copy.deepcopy(traps_cfg)
    return run_visit.build_observation(cfg, base_dir=mini)


def test_exposures_stay_independent():
    cfg = {"slow": {"initial": 200.0, "orbit_fill": 100.0}, "fast": {"initial": 30.0}}
    obs = _mini_observation(cfg)
    whole = obs.run_observation(write_fits=False)
    n = len(obs.exp_start_times)
    assert n >= 4 and len(obs.visit_plan["orbit_start_index"]) >= 2
    reads = {i: np.stack([r[0] for r in whole[i + 1].reads]) for i in range(n)}
    # round-robin shards of a world of 2
    for rank in range(2):
        part = _mini_observation(cfg).run_observation(rank=rank, world=2, write_fits=False)
        for i in range(rank, n, 2):
            np.testing.assert_array_equal(np.stack([r[0] for r in part[i + 1].reads]), reads[i])
    # one exposure alone
    alone = _mini_observation(cfg)
    i = n - 1
    frame = alone._generate_exposure(alone.exp_start_times[i], i + 1, write_fits=False)
    np.testing.assert_array_equal(np.stack([r[0] for r in frame.reads]), reads[i])
    # and the traps did act: the same visit without them differs
    plain = _mini_observation(cfg)
    plain.setup_charge_traps(None)
    frame = plain._generate_exposure(plain.exp_start_times[i], i + 1, write_fits=False)
    assert np.abs(np.stack([r[0] for r in frame.reads]) - reads[i]).max() > 0.5


class _Loose(object):
    """An ExposureTraps-like object that skips the Python checks (the library's own refusals are tested)."""

    def __init__(self, n=(100.0, 50.0), eta=(0.01, 0.01), tau=(1e4, 300.0), G=16, lo=1e-2, hi=1e6, table=None):
        self.traps = types.SimpleNamespace(rate_lo=lo, rate_hi=hi,
                                           array=lambda k: np.array({"n_traps": n, "efficiency": eta, "lifetime_s": tau}[k],
                                                                    dtype=np.float64))
        self.table = np.zeros((2, G)) if table is None else table


def test_refusals_and_clearing():
    v, pg, eng, desc = prepare("small256", out=np.float32)
    ctx = eng.ctx
    ctx.upload(0, desc)
    ctx.run(0)
    plain = ctx.download(0).copy()
    plain_name = ctx.ramp_variant(0)
    assert plain_name.startswith("k_ramp<")
    bad = [_Loose(eta=(1.5, 0.01)), _Loose(eta=(-0.1, 0.01)), _Loose(tau=(0.0, 1.0)), _Loose(n=(0.0, 1.0)),
           _Loose(n=(float("nan"), 1.0)), _Loose(G=1), _Loose(G=4097), _Loose(lo=0.0), _Loose(lo=10.0, hi=1.0),
           _Loose(hi=float("inf")), _Loose(table=np.full((2, 16), 101.0)), _Loose(table=np.full((2, 16), -1.0)),
           _Loose(table=np.full((2, 16), float("nan")))]
    for b in bad:
        ctx.upload(0, desc)
        with pytest.raises(_lib.WayneError) as e:
            ctx.set_traps(0, b)
        assert e.value.status == _lib.E_INVALID
        assert ctx.ramp_variant(0) == plain_name                   # the slot stays usable, without traps
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), plain)
    # a slot that was never uploaded
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_traps(kslot_unused(ctx), _Loose())
    assert e.value.status == _lib.E_STATE
    # replay mode reproduces the reference, which has no traps
    _, _, _, rdesc = prepare("small256", out=np.float32, rng_mode=_lib.RNG_REPLAY)
    ctx.upload(1, rdesc)
    with pytest.raises(_lib.WayneError) as e:
        ctx.set_traps(1, _Loose())
    assert e.value.status == _lib.E_INVALID
    # set, then cleared by NULL and by the next upload
    ctx.upload(0, desc)
    ctx.set_traps(0, T.ExposureTraps(strong_traps()))
    assert ctx.ramp_variant(0).startswith("k_ramp_trap<float, true, 1, false, ")
    ctx.set_traps(0, None)
    assert ctx.ramp_variant(0) == plain_name
    ctx.set_traps(0, T.ExposureTraps(strong_traps()))
    ctx.run(0)
    assert np.abs(ctx.download(0).astype(np.float64) - plain).max() > 1.0
    ctx.upload(0, desc)
    assert ctx.ramp_variant(0) == plain_name
    ctx.run(0)
    np.testing.assert_array_equal(ctx.download(0), plain)


def kslot_unused(ctx):
    return int(ctx._L.wayne_ctx_slots(ctx._h)) - 1      # (no test uploads into the last slot)


def test_science_check_a_scanned_visit_shows_the_ramp_the_model_predicts():
    # 3 orbits x 4 exposures of a 256^2 scan, hook trend off (scale_factor 1): traps on against traps off, paired
    model = T.ChargeTraps()
    n_orbits, per = 3, 4
    plan = visit_plan(n_orbits, per, exptime=14.971, gap_s=40.0)
    tables = model.start_tables(plan, 14.971, staring=False)
    n = n_orbits * per
    v = helpers.make_visit("small256", n_exposures=n)
    ratio, pred, col_loss = [], [], []
    for i in range(n):
        kw = v.frame_kwargs(i, planet_signal=np.zeros((v.K, v.wl.size)), scale_factor=1.0, cosmic_rate=None, **PLAIN)
        descs = []
        for tr in (None, T.ExposureTraps(model, tables[i])):
            pg = helpers.product_generator(v, i)
            pg.prepare(rng_mode=_lib.RNG_SPLIT, out_dtype=np.float64, charge_traps=tr, **kw)
            eng, d, _ = pg._prepared
            pg._prepared = None
            descs.append(d)
        acc, off = run(eng.ctx, descs[0])
        _, on = run(eng.ctx, descs[1])
        want, trapped, dN = oracle(v, pg, descs[0], off, acc, descs[1]._traps)
        np.testing.assert_allclose(on, want, rtol=0, atol=1e-9)
        S = off.shape[1]
        box = (slice(5, S - 5), slice(5, S - 5))
        w_off = (off[-1] - off[0])[box].sum()
        w_on = (on[-1] - on[0])[box].sum()
        ratio.append(w_on / w_off)
        pred.append(1.0 - trapped[-1][box].sum() / dN.sum(axis=0)[box].sum())
        cols_off = (off[-1] - off[0])[box].sum(axis=0)
        cols_on = (on[-1] - on[0])[box].sum(axis=0)
        col_loss.append((cols_off, cols_on))
    ratio, pred = np.array(ratio), np.array(pred)
    np.testing.assert_allclose(ratio, pred, rtol=1e-9)
    r = ratio.reshape(n_orbits, per)
    assert (r[:, 0] < r[:, -1]).all()                    # a hook in every orbit: its first exposure comes out lowest
    assert r[0, 0] < r[1:, 0].min()                      # ... and the first orbit's is the deepest
    assert ratio.max() < 1.0
    # flux-dependent: the faintest spectral channel of the trace loses a larger fraction than the brightest
    cols_off, cols_on = col_loss[0]
    sky_level = np.median(cols_off)
    lit = np.where(cols_off > sky_level + 0.2 * (cols_off.max() - sky_level))[0]
    bright = lit[np.argmax(cols_off[lit])]
    faint = lit[np.argmin(cols_off[lit])]
    loss = 1.0 - cols_on / cols_off
    assert loss[faint] > loss[bright] > 0
