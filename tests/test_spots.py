"""Star spots, host side: the lens rule of wayne_amd/spots.py against its converged form and against closed forms, the
law's signs, the library's own host arithmetic (wayne_spot_lens_basis: the inline function k_lightcurve_spots compiles)
against the numpy law, the orbit's track, and the bookkeeping (refusals, YAML forms, cards, --resume, digest).
The device kernel is compared with this law in tests/test_spots_gpu.py.

Bounds:
  * RULE: 4 x the worst |Q_n - Q_n(48 nodes)| / lens area over spots.rule_check_lenses() (seed 1, 300 lenses, p, r in
    [0.03, 0.3], spots wholly inside 0.98, every third pinned at |C| + r = 0.98, every fifth with d scaled by 1e-3) as
    recorded in profiles/spots.json (1.8e-7); the factor covers another libm's sin / acos; it must stay below 1e-6;
  * ABI: 256 * 2^-52 * Q_0 -- the rule has 200 non-negative terms, each <= its area weight since mu <= 1; recursive
    summation of n such terms errs by at most n - 1 units of rounding of the sum, each term carries about a dozen
    roundings of its own and a few units from sin / cos / acos."""
import copy
import json
import os

import numpy as np
import pytest
import yaml

from wayne_amd import _lib, exposure, lightcurve as lc, run_visit, spots, visit
from wayne_amd.exposure_generator import ExposureGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
LD = [0.800627, -0.757066, 0.897268, -0.384804]
with open(os.path.join(ROOT, "profiles", "spots.json")) as _f:
    RECORDED = json.load(_f)["rule"]["worst_error_over_area"]
RULE = 4.0 * RECORDED
ABI = 256 * 2.0 ** -52


def lens_area(d, p, r):
    if d >= p + r:
        return 0.0
    if d <= abs(p - r):
        return np.pi * min(p, r) ** 2
    return (p * p * np.arccos((d * d + p * p - r * r) / (2 * d * p)) + r * r * np.arccos((d * d + r * r - p * p) / (2 * d * r)) -
            0.5 * np.sqrt((-d + p + r) * (d + p - r) * (d - p + r) * (d + p + r)))


def test_rule_against_the_converged_rule():
    assert RULE < 1e-6                                   # (else: raise the node count, do not widen)
    lenses = spots.rule_check_lenses(seed=1, n=300)
    assert len(lenses) == 300
    assert all(np.hypot(*C) + r <= spots.LIMB * (1 + 1e-15) for (_, C, _, r) in lenses)
    assert sum(abs(np.hypot(*C) + r - spots.LIMB) < 1e-12 for (_, C, _, r) in lenses) >= 100
    worst = spots.rule_error(lenses)
    print("lens rule: worst |Q_n - Q_n(48)| / area = %.3e (recorded %.3e)" % (worst, RECORDED))
    assert worst <= RULE


@pytest.mark.parametrize("eps", [1e-4, 1e-8, 1e-12])
def test_rule_through_both_tangencies(eps):
    """Either side of d = p + r and of d = r - p the rule is finite, within RULE of the converged rule relative to the
    lens area, and its step across the boundary is the converged rule's step within RULE of the smaller circle's area."""
    p, r, C, u = 0.1, 0.2, (0.3, -0.2), (0.6, 0.8)

    def at(d, nodes=None):
        return spots.lens_basis((C[0] - d * u[0], C[1] - d * u[1]), C, p, r, nodes=nodes)

    small = np.pi * min(p, r) ** 2
    for below, above in (((p + r) * (1 - eps), (p + r) * (1 + eps)), ((r - p) * (1 - eps), (r - p) * (1 + eps))):
        q = [at(below), at(above)]
        ref = [at(below, 48), at(above, 48)]
        for a, b in zip(q, ref):
            assert np.all(np.isfinite(a)) and np.all(a >= 0.0)
            assert np.abs(a - b).max() <= RULE * b[0]
        assert np.abs((q[0] - q[1]) - (ref[0] - ref[1])).max() <= RULE * small
    assert np.all(at((p + r) * (1 + eps)) == 0.0) and at((p + r) * (1 - eps))[0] > 0.0
    # the swapped pair: a small spot and a large planet
    q_in = spots.lens_basis((0.1, 0.1), (0.1 + (r - p) * (1 - eps), 0.1), r, p)
    q_out = spots.lens_basis((0.1, 0.1), (0.1 + (r - p) * (1 + eps), 0.1), r, p)
    assert np.all(np.isfinite(q_out)) and np.abs(q_in - q_out).max() <= RULE * small + 4 * eps * small


def test_closed_forms_on_a_uniform_star():
    flat = [0.0, 0.0, 0.0, 0.0]
    # Q_0 is the lens area
    for (P, C, p, r) in spots.rule_check_lenses(seed=1, n=60):
        d = float(np.hypot(C[0] - P[0], C[1] - P[1]))
        area = lens_area(d, p, r)
        assert abs(spots.lens_basis(P, C, p, r)[0] - area) <= RULE * area
    # unocculted: depth' = depth / (1 - sum (1 - c) r^2)
    cx, cy, rad = np.array([0.5, -0.4]), np.array([0.3, -0.5]), np.array([0.2, 0.1])
    con = np.array([[0.6, 0.7, 0.8], [1.1, 1.2, 1.3]])
    spec = np.array([0.01, 0.0144, 0.02])
    p = np.sqrt(spec)
    X, Y = np.array([-0.5, 0.0]), np.array([0.4, 0.8])                    # far from both spots
    z = np.hypot(X, Y)
    depth = lc.planet_depths(flat, spec, z, np.zeros(2))
    np.testing.assert_allclose(depth, np.tile(spec, (2, 1)), rtol=1e-9)
    got = spots.apply_law(depth, X, Y, z, None, spec, flat, cx, cy, rad, con)
    want = depth / (1.0 - ((1.0 - con) * rad[:, None] ** 2).sum(axis=0))
    assert np.abs(got / want - 1.0).max() <= RULE
    # planet inside a spot: depth' = c p^2 / (1 - (1 - c) r^2)
    X, Y = np.array([0.45]), np.array([0.33])
    z = np.hypot(X, Y)
    depth = lc.planet_depths(flat, spec, z, np.zeros(1))
    got = spots.apply_law(depth, X, Y, z, None, spec, flat, cx[:1], cy[:1], rad[:1], con[:1])
    want = con[0] * p * p / (1.0 - (1.0 - con[0]) * rad[0] ** 2)
    assert np.abs(got[0] / want - 1.0).max() <= RULE + 1e-9                # (1e-9: planet_depths' own p^2)
    # spot inside the planet: Q_n = S_n (limb-darkened too)
    S = spots.spot_basis([0.3], [0.2], [0.05])[0]
    Q = spots.lens_basis((0.31, 0.22), (0.3, 0.2), np.array([0.12]), 0.05)[:, 0]
    assert np.abs(Q - S).max() <= RULE * S[0]


def _one_spot_case(contrast):
    spec = np.array([0.0144, 0.015])
    X = np.array([0.3, -0.6, 3.0])            # crossing the spot, in transit far from it, out of transit
    Y = np.array([0.25, 0.1, 0.2])
    z = np.hypot(X, Y)
    depth = lc.planet_depths(LD, spec, z, np.zeros(3))
    return depth, spots.apply_law(depth, X, Y, z, None, spec, LD, [0.35], [0.2], [0.15], np.full((1, 2), contrast))


def test_signs():
    depth, dark = _one_spot_case(0.6)
    assert np.all(dark[0] < depth[0]) and np.all(dark[1] > depth[1]) and np.all(dark[2] == 0.0) and np.all(depth[2] == 0.0)
    _, bright = _one_spot_case(1.2)
    assert np.all(bright[0] > depth[0]) and np.all(bright[1] < depth[1])
    _, same = _one_spot_case(1.0)
    np.testing.assert_allclose(same, depth, rtol=2.0 ** -52, atol=0)       # one rounding: depth F0 / F0


def test_c_abi_against_numpy():
    g, w = _lib.spot_rule()
    G, W = spots.gauss_legendre()
    assert g.tobytes() == G.tobytes() and w.tobytes() == W.tobytes()       # the same bits on both sides
    cases = spots.rule_check_lenses(seed=2, n=200)
    p, r, C = 0.1, 0.2, (0.3, -0.2)
    for eps in (1e-4, 1e-8, 1e-12):
        for d in ((p + r) * (1 - eps), (p + r) * (1 + eps), (r - p) * (1 - eps), (r - p) * (1 + eps)):
            cases.append(((C[0] - 0.6 * d, C[1] - 0.8 * d), C, p, r))
    cases += [((0.2, 0.1), (0.2, 0.1), 0.1, 0.1), ((0.2, 0.1), (0.2, 0.1), 0.05, 0.1), ((0.0, 0.0), (0.5, 0.5), 0.1, 0.1)]
    worst = 0.0
    for (P, C_, p_, r_) in cases:
        want = spots.lens_basis(P, C_, p_, r_)
        got = _lib.spot_lens_basis(P, C_, p_, r_)
        assert np.all(np.abs(got - want) <= ABI * want[0]), (P, C_, p_, r_)
        if want[0] > 0:
            worst = max(worst, np.abs(got - want).max() / want[0])
    print("wayne_spot_lens_basis: worst |C - numpy| / Q_0 = %.2f x 2^-52" % (worst * 2.0 ** 52))


def test_track_reproduces_the_orbit_to_the_bit():
    orbit = (3.524746, 8.81, 0.0, 86.71, 0.0, 2456196.28836)
    for t in (2456196.2 + np.arange(448) * 25e-3 / 86400.0,        # the Chebyshev route
              2456196.2 + np.arange(9) * 1e-3,                     # few samples
              2456196.2 + np.arange(100) * 1e-2):                  # a long span
        z, los = lc.planet_orbit_short_span(*(orbit + (t,)))
        X, Y, Z = lc.planet_track_short_span(*(orbit + (t,)))
        assert np.sqrt(X * X + Y * Y).tobytes() == z.tobytes() and Z.tobytes() == los.tobytes()
        z_tr, hidden = lc.depth_inputs(*(orbit + (t, 0.12)))
        z_tr2, hidden2, X2, Y2 = lc.depth_inputs_track(*(orbit + (t, 0.12)))
        assert z_tr.tobytes() == z_tr2.tobytes() and hidden.tobytes() == hidden2.tobytes()
        assert X2.tobytes() == X.tobytes() and Y2.tobytes() == Y.tobytes()


def test_contrast_on_a_grid():
    wl = np.array([1.1, 1.4, 1.7])
    s = spots.StarSpots([spots.Spot(0.1, 0.2, 0.1, temperature=4200.0), spots.Spot(-0.4, 0.2, 0.1, contrast=0.75)],
                        photosphere_temperature=5000.0)
    c = s.on_grid(wl)
    assert c.shape == (2, 3) and np.all(c[1] == 0.75)
    np.testing.assert_allclose(c[0], [0.59, 0.65, 0.68], atol=0.006)      # the Planck ratios of a 4200 K spot on 5000 K
    geo = s.geometry([0.0, 0.1], [0.5, 0.5], wl)
    assert geo.n == 2 and geo.crop(1, 3).contrast.shape == (2, 2)
    np.testing.assert_array_equal(geo.crop(1, 3).contrast, c[:, 1:3])


def test_refusals():
    ok = dict(cx=[0.1, -0.4], cy=[0.2, 0.2], radius=[0.1, 0.1])
    spots.check_geometry(**ok)
    bad = [dict(cx=[0.0] * 9, cy=list(np.linspace(-0.9, 0.9, 9)), radius=[0.01] * 9),      # more than 8
           dict(ok, radius=[0.1, 0.0]), dict(ok, radius=[0.1, -0.1]), dict(ok, radius=[0.1, np.nan]),
           dict(ok, radius=[0.1, np.inf]), dict(cx=[0.9], cy=[0.0], radius=[0.081]),       # beyond 0.98
           dict(ok, cx=[0.1, 0.25]),                                                       # overlapping
           dict(ok, contrast=[[0.5, -0.1], [1.0, 1.0]]), dict(ok, contrast=[[0.5, np.nan], [1.0, 1.0]]),
           dict(ok, contrast=[[0.5, 0.5]])]
    for kw in bad:
        with pytest.raises(ValueError):
            spots.check_geometry(**kw)
    spots.check_geometry([0.9], [0.0], [0.08])                                             # 0.98 itself is allowed
    with pytest.raises(ValueError):
        spots.StarSpots([spots.Spot(0.1 * i - 0.4, 0.0, 0.01, contrast=0.5) for i in range(9)])
    for kw in (dict(), dict(contrast=0.5, temperature=4000.0), dict(contrast=-0.5), dict(contrast=np.nan),
               dict(temperature=-1.0)):
        with pytest.raises(ValueError):
            spots.Spot(0.0, 0.0, 0.1, **kw)
    with pytest.raises(ValueError):
        spots.StarSpots([spots.Spot(0.0, 0.0, 0.1, temperature=4000.0)])                   # no photosphere temperature
    with pytest.raises(ValueError):
        spots.StarSpots([spots.Spot(0.0, 0.0, 0.1, contrast=0.5)], photosphere_temperature=5000.0)
    # F0 - D <= 0: a facula bright enough ... is not possible (D < 0 then); a dark star is: limb darkening whose disc
    # flux is smaller than what the spots remove
    with pytest.raises(ValueError):
        spots.unocculted_deficit([4.9, 0.0, 0.0, 0.0], [0.0], [0.0], [0.9], np.zeros((1, 2)))
    # apply: K or W other than the matrix's, a track that is not finite on a transit row
    depth = np.zeros((3, 2))
    args = dict(depth=depth, X=np.zeros(3), Y=np.full(3, 0.5), z_tr=np.full(3, 0.5), hidden=None,
                planet_spectrum=[0.01, 0.01], ld=LD, cx=[0.1], cy=[0.2], radius=[0.1], contrast=np.full((1, 2), 0.5))
    spots.apply_law(**args)
    for change in (dict(X=np.zeros(2)), dict(contrast=np.full((1, 3), 0.5)), dict(planet_spectrum=[0.01]),
                   dict(X=np.array([0.0, np.nan, 0.0]))):
        with pytest.raises(ValueError):
            spots.apply_law(**dict(args, **change))
    # ... which is fine on a row behind the star
    spots.apply_law(**dict(args, X=np.array([0.0, np.nan, 0.0]), z_tr=np.array([0.5, 10.5, 0.5])))
    with pytest.raises(ValueError):
        lc.DeviceDepths(np.full(3, 0.5), None, [0.01, 0.01], LD,
                        spots=spots.SpotGeometry(np.zeros(2), np.zeros(2), [0.1], [0.2], [0.1], np.full((1, 2), 0.5)))


def test_eclipse_rows_and_unsized_columns_are_left_alone():
    spec = np.array([0.0144, -1.0, 0.015])
    z_tr = np.array([0.4, 10.4, 0.4])
    hidden = np.array([0.0, 1.0, 0.3])
    geo = spots.SpotGeometry([0.3, 0.3, 0.3], [0.25, 0.25, 0.25], [0.35], [0.2], [0.15], np.full((1, 3), 0.6))
    plain = lc.planet_depths(LD, spec, z_tr, hidden)
    spotted = lc.planet_depths(LD, spec, z_tr, hidden, spots=geo)
    assert np.all(spotted[1:] == plain[1:]) and np.all(spotted[:, 1] == 0.0)
    assert np.all(spotted[0, [0, 2]] < plain[0, [0, 2]])
    dd = lc.DeviceDepths(z_tr, hidden, spec, LD, spots=geo)
    np.testing.assert_array_equal(dd.host_matrix(), spotted)
    np.testing.assert_array_equal(lc.DeviceDepths(z_tr, hidden, spec, LD).host_matrix(), plain)


# -- bookkeeping ------------------------------------------------------------------------------------------------------
def base_cfg():
    with open(os.path.join(MINI, "params.yml")) as f:
        return yaml.safe_load(f)


SECTION = {"photosphere_temperature": 5000, "list": [{"x": -0.21, "y": 0.33, "radius": 0.10, "temperature": 4200},
                                                      {"at_phase": 0.0021, "radius": 0.06, "contrast": 0.75}]}


def spotted_cfg(section=None):
    cfg = base_cfg()
    cfg["target"]["spots"] = copy.deepcopy(SECTION if section is None else section)
    return cfg


def test_yaml_forms():
    obs = run_visit.build_observation(base_cfg(), base_dir=MINI)
    assert obs.spots is None and obs.planet.spot_cards is None
    t = obs.exp_start_times[0] + np.linspace(0, 2e-4, 4)
    plain = obs.generate_lightcurves(t)
    assert obs.device_depths(t).spots is None
    on = run_visit.build_observation(spotted_cfg(), base_dir=MINI)
    s = on.spots
    assert isinstance(s, spots.StarSpots) and len(s.spots) == 2 and s.photosphere_temperature == 5000.0
    assert (s.spots[0].x, s.spots[0].y, s.spots[0].radius, s.spots[0].temperature) == (-0.21, 0.33, 0.10, 4200.0)
    # at_phase: where the planet's centre is 0.0021 periods after mid-transit
    X, Y, Z = lc.planet_position(3.524746, on.planet.sma_over_rs, 0.0, 86.71, 0.0, 0.0, np.array([0.0021 * 3.524746]))
    assert (s.spots[1].x, s.spots[1].y) == (float(X[0]), float(Y[0])) and Z[0] > 0 and abs(Y[0]) > 0.4
    dd = on.device_depths(t)
    assert dd.spots.n == 2 and dd.spots.contrast.shape == (2, on.wl.size) and dd.spots.X.size == 4
    np.testing.assert_array_equal(dd.spots.contrast, s.on_grid(on.wl))
    np.testing.assert_allclose(1 - on.generate_lightcurves(t), dd.host_matrix(), rtol=0, atol=2.0 ** -52)   # (1 - (1 - x))
    in_transit = dd.host_matrix() > 0
    assert in_transit.any() and np.all((1 - on.generate_lightcurves(t))[in_transit] > (1 - plain)[in_transit])
    white = on.generate_lightcurves(t, depth=0.0146)
    assert white.shape == (4, 1)
    bad = [[1, 2], {"list": []}, {"list": "x"}, {"list": SECTION["list"]},                       # no photosphere temperature
           {"photosphere_temperature": 5000, "list": [{"x": 0.1, "y": 0.1, "radius": 0.1, "contrast": 0.5}]},
           dict(SECTION, extra=1), {"list": [{"x": 0.1, "radius": 0.1, "contrast": 0.5}]},
           {"list": [{"x": 0.1, "y": 0.1, "contrast": 0.5}]}, {"list": [{"x": 0.1, "y": 0.1, "radius": 0.1}]},
           {"list": [{"x": 0.1, "y": 0.1, "radius": 0.1, "contrast": 0.5, "colour": "red"}]},
           {"list": [{"x": 0.1, "y": 0.1, "at_phase": 0.0, "radius": 0.1, "contrast": 0.5}]},
           {"list": [{"at_phase": "soon", "radius": 0.1, "contrast": 0.5}]},
           {"list": [{"at_phase": 0.02, "radius": 0.1, "contrast": 0.5}]},                      # centred beyond the limb
           {"list": [{"x": "a", "y": 0.1, "radius": 0.1, "contrast": 0.5}]},
           {"list": [{"x": 0.9, "y": 0.0, "radius": 0.1, "contrast": 0.5}]},
           {"list": [{"x": 0.0, "y": 0.0, "radius": 0.1, "contrast": -1}]},
           {"list": [{"x": 0.0, "y": 0.0, "radius": 0.1, "contrast": 0.5}, {"x": 0.1, "y": 0.0, "radius": 0.1, "contrast": 0.5}]},
           {"list": [{"x": 0.1 * i - 0.4, "y": 0.0, "radius": 0.01, "contrast": 0.5} for i in range(9)]},
           "dark"]
    for section in bad:
        with pytest.raises(run_visit.WFC3SimConfigError):
            run_visit.build_observation(spotted_cfg(section), base_dir=MINI)
    cfg = spotted_cfg()
    cfg["target"]["planet_spectrum_file"] = False         # no transit: nothing a spot could act on
    with pytest.raises(run_visit.WFC3SimConfigError):
        run_visit.build_observation(cfg, base_dir=MINI)
    with pytest.raises(ValueError):
        obs.setup_target(obs.planet, obs.wl, None, obs.stellar_flux, spots=s)


INFO = {"SUBARRAY": 128, "NSAMP": 4, "SAMPSEQ": "RAPID", "x_ref": 460.0, "EXPSTART": 2456196.0, "filename": "0001_raw.fits"}


def test_header_cards_and_the_resume_check():
    obs = run_visit.build_observation(base_cfg(), base_dir=MINI)
    plain = exposure.Exposure(obs.detector, obs.grism, obs.planet, dict(INFO)).generate_science_header()
    assert not any(k.startswith("SPT") or k in ("SPOTS", "NSPOTS") for k, _, _ in plain.cards)
    on_obs = run_visit.build_observation(spotted_cfg(), base_dir=MINI)
    on = exposure.Exposure(on_obs.detector, on_obs.grism, on_obs.planet, dict(INFO)).generate_science_header()
    assert on.cards[:len(plain.cards)][1:] == plain.cards[1:]          # (card 0 is the date)
    assert [k for k, _, _ in on.cards[len(plain.cards):]] == ["SPOTS", "NSPOTS", "SPTX1", "SPTY1", "SPTR1", "SPTC1",
                                                              "SPTX2", "SPTY2", "SPTR2", "SPTC2", "SPTHASH"]
    s = on_obs.spots
    contrast = s.on_grid(on_obs.wl)
    assert on["SPOTS"] is True and on["NSPOTS"] == 2 and (on["SPTX1"], on["SPTY1"], on["SPTR1"]) == (-0.21, 0.33, 0.10)
    assert on["SPTC1"] == contrast[0, on_obs.wl.size // 2] and on["SPTC2"] == 0.75 and on["SPTR2"] == 0.06
    assert on["SPTHASH"] == s.hash(on_obs.wl) and len(on["SPTHASH"]) == 16 and int(on["SPTHASH"], 16) >= 0
    # --resume's comparison, both directions, and after a spot was changed, removed or added
    assert obs._spot_cards_match(plain) and not obs._spot_cards_match(on)
    assert on_obs._spot_cards_match(on) and not on_obs._spot_cards_match(plain)
    changed, removed, added = copy.deepcopy(SECTION), copy.deepcopy(SECTION), copy.deepcopy(SECTION)
    changed["list"][1]["contrast"] = 0.7500001
    del removed["list"][1]
    added["list"].append({"x": 0.5, "y": 0.5, "radius": 0.05, "contrast": 1.1})
    hashes = {on["SPTHASH"]}
    for section in (changed, removed, added):
        other = run_visit.build_observation(spotted_cfg(section), base_dir=MINI)
        assert not other._spot_cards_match(on)
        hashes.add(other.spots.hash(other.wl))
    assert len(hashes) == 4


def test_resume_regenerates_files_whose_spot_cards_differ(tmp_path):
    from wayne_amd import fitsio
    obs = run_visit.build_observation(spotted_cfg(), base_dir=MINI)
    plain_obs = run_visit.build_observation(base_cfg(), base_dir=MINI)
    S = obs.SUBARRAY + 10
    for o, sub in ((obs, "with"), (plain_obs, "without")):
        o.outdir = str(tmp_path / sub)
        os.makedirs(o.outdir)
        e = exposure.Exposure(o.detector, o.grism, o.planet, {"SUBARRAY": o.SUBARRAY, "NSAMP": o.NSAMP, "SAMPSEQ": o.SAMPSEQ,
                                                             "EXPSTART": float(o.exp_start_times[0]), "x_ref": 460.0})
        e.add_read(np.zeros((S, S)), {"cumulative_exp_time": 0.0, "read_exp_time": 0.0, "CRPIX1": 0})
        for r in range(o.NSAMP - 1):
            e.add_read(np.zeros((S, S)), {"cumulative_exp_time": 1.0 + r, "read_exp_time": 1.0, "CRPIX1": 0})
        e.generate_fits(o.outdir, "0001_raw.fits")
        assert fitsio.scan(os.path.join(o.outdir, "0001_raw.fits")) is not None
        assert o.exposure_file_is_whole(1)
    obs.outdir, plain_obs.outdir = plain_obs.outdir, obs.outdir
    assert not obs.exposure_file_is_whole(1) and not plain_obs.exposure_file_is_whole(1)


def _descriptor(obs, t0):
    gen = ExposureGenerator(obs.detector, obs.grism, obs.NSAMP, obs.SAMPSEQ, obs.SUBARRAY, calibration=obs.calibration,
                            seed=obs.seed, exposure_index=0)
    _, mid, dur, ri = gen._gen_scanning_sample_times(obs.sample_rate)
    dd = obs.device_depths(t0 + mid / 86400e3)
    return gen.build_descriptor(None, float(obs.x_ref[0]), float(obs.y_ref[0]), 0.0, 0.0, obs.wl, obs.stellar_flux, dd,
                                obs.scan_speed, obs.sample_rate, mid, dur, ri), dd


def test_descriptor_carries_the_cropped_spots_and_the_digest_follows_them():
    from wayne_amd import tools
    plain_obs = run_visit.build_observation(base_cfg(), base_dir=MINI)
    t0 = float(plain_obs.exp_start_times[0])
    plain, _ = _descriptor(plain_obs, t0)
    assert plain._spots is None
    digests = {visit.descriptor_digest(plain)}
    moved = copy.deepcopy(SECTION)
    moved["list"][0]["x"] += 1e-12
    for section in (SECTION, moved):
        obs = run_visit.build_observation(spotted_cfg(section), base_dir=MINI)
        d, dd = _descriptor(obs, t0)
        i0, i1 = tools.crop_spectrum_ind(obs.grism.wl_limits[0], obs.grism.wl_limits[1], obs.wl)
        assert d._spots.contrast.shape == (2, d.n_wl) == (2, i1 - i0) and d._spots.X.size == d.n_samples
        np.testing.assert_array_equal(d._spots.contrast, dd.spots.contrast[:, i0:i1])
        assert visit.descriptor_digest(d) == visit.descriptor_digest(_descriptor(obs, t0)[0])
        digests.add(visit.descriptor_digest(d))
    assert len(digests) == 3


def test_synthetic_visit_passes_spots_through():
    import helpers
    v = helpers.make_visit("tiny")
    plain = v.device_depths(0)
    assert plain.spots is None
    v.spots = spots.StarSpots([spots.Spot(0.1, -0.5, 0.1, contrast=0.7)])
    dd = v.device_depths(0)
    assert dd.spots.n == 1 and dd.spots.contrast.shape == (1, v.wl.size) and dd.spots.X.size == dd.z_tr.size
    assert dd.z_tr.tobytes() == plain.z_tr.tobytes()
    runner = visit.VisitRunner(v, device_lc=True)
    d = runner.descriptor(0)
    assert d._spots.contrast.shape == (1, d.n_wl)
