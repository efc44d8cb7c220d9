"""Limb darkening per wavelength bin, host side: the basis form of the law (lightcurve.transit_basis), the table
(lightcurve.LimbDarkening), the YAML forms, the header cards and --resume's comparison, the descriptor digest.
The device kernel (k_lightcurve_ld) is compared with this law in tests/test_ld_table_gpu.py.

The table used throughout: s = clip((wl - 1.1) / 0.6, 0, 1), a = (0.55 + 0.25 s, -0.2 - 0.55 s, 0.5 + 0.4 s,
-0.25 - 0.13 s) -- physical profiles (min I(mu) = 0.40 over the band)."""
import copy
import hashlib
import os

import numpy as np
import pytest
import yaml

from oracle import clib
from wayne_amd import exposure, lightcurve as lc, run_visit, visit
from wayne_amd.exposure_generator import ExposureGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")
LD = [0.800627, -0.757066, 0.897268, -0.384804]


def table_at(wl):
    s = np.clip((np.asarray(wl, dtype=float) - 1.1) / 0.6, 0.0, 1.0)
    return np.stack([0.55 + 0.25 * s, -0.2 - 0.55 * s, 0.5 + 0.4 * s, -0.25 - 0.13 * s], axis=1)


def lens_area(z, p):
    z, p = np.broadcast_arrays(np.asarray(z, dtype=float), np.asarray(p, dtype=float))
    out = np.zeros(z.shape)
    inside = z <= 1 - p
    out[inside] = np.pi * p[inside] ** 2
    part = (z > 1 - p) & (z < 1 + p)
    zz, pp = z[part], p[part]
    k0 = np.arccos(np.clip((pp ** 2 + zz ** 2 - 1) / (2 * pp * zz), -1, 1))
    k1 = np.arccos(np.clip((1 - pp ** 2 + zz ** 2) / (2 * zz), -1, 1))
    out[part] = pp ** 2 * k0 + k1 - 0.5 * np.sqrt(np.maximum(4 * zz ** 2 - (1 + zz ** 2 - pp ** 2) ** 2, 0.0))
    return out


def grid():
    # the z / p grid of test_lightcurve.test_host_model_against_oracle
    rp = np.sqrt(0.0146)
    z = np.concatenate([np.linspace(0, 1.2, 61), [1 - rp, 1 + rp, rp, 1.0]])
    return z, rp * np.array([0.9, 1.0, 1.1])


def test_basis_combination_is_the_existing_law():
    z, p = grid()
    B = lc.transit_basis(z[:, None], p[None, :])
    assert len(B) == 5 and all(b.shape == (z.size, p.size) for b in B)
    want = 1 - lc.transit_flux(z[:, None], p[None, :], LD)
    # the two differ only in the order of about 125 float64 terms of magnitude <= pi p^2
    np.testing.assert_allclose(lc.deficit_from_basis(B, LD), want, rtol=0, atol=1e-13)
    # ... and [W, 4] with the same row for every wavelength is the same matrix through transit_flux itself
    np.testing.assert_allclose(1 - lc.transit_flux(z[:, None], p[None, :], np.tile(LD, (p.size, 1))), want, rtol=0, atol=1e-13)
    assert all(b[z >= 1 + p.max()].max() == 0.0 for b in B)


@pytest.fixture(scope="module")
def per_wavelength():
    W = 40
    wl = np.linspace(1.1, 1.7, W)
    p = np.sqrt(0.0146) * (1 + 0.004 * np.sin(np.arange(W) / 3.0))
    z, _ = grid()
    table = table_at(wl)
    got = 1 - lc.transit_flux(z[:, None], p[None, :], table)
    return wl, p, z, table, got


def test_per_wavelength_law_against_the_oracle(per_wavelength):
    wl, p, z, table, got = per_wavelength
    want = np.stack([clib.lc_deficit(z, p[w:w + 1], table[w])[:, 0] for w in range(wl.size)], axis=1)
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-10)
    # with an eclipse row, through planet_depths and DeviceDepths.host_matrix
    spec = p * p
    z_tr, hidden = np.array([0.3, 1.05, 11.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0])
    want = np.stack([clib.lc_depths(z_tr, hidden, spec[w:w + 1], table[w])[:, 0] for w in range(wl.size)], axis=1)
    np.testing.assert_allclose(lc.planet_depths(table, spec, z_tr, hidden), want, rtol=0, atol=5e-10)
    np.testing.assert_array_equal(lc.DeviceDepths(z_tr, hidden, spec, table).host_matrix(),
                                  lc.planet_depths(table, spec, z_tr, hidden))
    # [4] stays today's code path
    one = lc.DeviceDepths(z_tr, hidden, spec, LD)
    assert one.ld_table is None and one.ld == LD
    np.testing.assert_array_equal(one.host_matrix(), lc.planet_depths(LD, spec, z_tr, hidden))
    with pytest.raises(ValueError):
        lc.DeviceDepths(z_tr, hidden, spec, table[:-1])
    with pytest.raises(ValueError):
        lc.transit_flux(z[:, None], p[None, :], table[:-1])


def test_the_test_input_bites(per_wavelength):
    wl, p, z, table, got = per_wavelength
    single = 1 - lc.transit_flux(z[:, None], p[None, :], LD)
    assert np.abs(got - single).max() > 1e-4


def test_closed_forms():
    z, p = grid()
    B = lc.transit_basis(z[:, None], p[None, :])
    # B_0 is the lens area (2e-9: the 24-node rule at the contacts, as test_uniform_star_matches_lens_formula)
    np.testing.assert_allclose(B[0], lens_area(z[:, None], p[None, :]), rtol=0, atol=2e-9 * np.pi)
    # mu^2 = 1 - r^2: over a planet wholly inside the disk int (1 - r^2) dA = pi p^2 (1 - z^2 - p^2 / 2)
    zi = np.array([0.0, 0.2, 0.5, 0.85])
    B4 = lc.transit_basis(zi[:, None], p[None, :])[4]
    np.testing.assert_allclose(B4, np.pi * p[None, :] ** 2 * (1 - zi[:, None] ** 2 - p[None, :] ** 2 / 2), rtol=0, atol=1e-10)
    # the other laws, through claret_intensity, against their own formulas
    mu = np.linspace(0, 1, 21)
    u1, u2, u = 0.4, 0.25, 0.6
    q = lc.LimbDarkening([1.1, 1.7], [[u1, u2], [u1, u2]], "quadratic")
    np.testing.assert_allclose(lc.claret_intensity(mu, q.claret[0]), 1 - u1 * (1 - mu) - u2 * (1 - mu) ** 2, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(q.claret[0], [0.0, u1 + 2 * u2, 0.0, -u2])
    for coeffs in ([[u], [u]], [u, u]):
        lin = lc.LimbDarkening([1.1, 1.7], coeffs, "linear")
        np.testing.assert_allclose(lc.claret_intensity(mu, lin.claret[1]), 1 - u * (1 - mu), rtol=0, atol=1e-15)
    # on_grid at, between and beyond the nodes
    nodes = np.array([1.1, 1.3, 1.7])
    t = lc.LimbDarkening(nodes, table_at(nodes))
    np.testing.assert_array_equal(t.on_grid(nodes), table_at(nodes))
    np.testing.assert_allclose(t.on_grid([1.2, 1.5]), table_at([1.2, 1.5]), rtol=0, atol=1e-15)    # (the table is linear in wl)
    np.testing.assert_array_equal(t.on_grid([0.9, 2.0]), table_at(nodes)[[0, 2]])
    assert t.on_grid(np.linspace(1, 2, 7)).shape == (7, 4)


def test_table_refusals():
    nodes = [1.1, 1.4, 1.7]
    good = table_at(nodes)
    lc.LimbDarkening(nodes, good)
    for wl in ([1.1, 1.1, 1.7], [1.1, 1.0, 1.7], [1.1, np.nan, 1.7], [1.1, np.inf, 1.7], []):
        with pytest.raises(ValueError):
            lc.LimbDarkening(wl, good[:len(wl)])
    for coeffs, law in ((good[:, :3], "claret4"), (good, "quadratic"), (good[:, :2], "linear"), (good[:2], "claret4"),
                        (good, "power2")):
        with pytest.raises(ValueError):
            lc.LimbDarkening(nodes, coeffs, law)
    bad = good.copy()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError):
        lc.LimbDarkening(nodes, bad)
    bad = good.copy()
    bad[2] = [5.0, 0.0, 0.0, 0.0]              # disk flux pi (1 - 5/5) = 0
    with pytest.raises(ValueError):
        lc.LimbDarkening(nodes, bad)
    with pytest.raises(ValueError):
        lc.LimbDarkening(nodes, [[3.5], [0.1], [0.1]], "linear")     # 1 - 3.5/3 < 0


def base_cfg():
    return yaml.safe_load(open(os.path.join(MINI, "params.yml")))


def inline(nodes, law="claret4", coeffs=None):
    coeffs = table_at(nodes) if coeffs is None else coeffs
    return {"law": law, "wl_um": [float(x) for x in nodes], "coeffs": [[float(x) for x in row] for row in coeffs]}


def test_yaml_forms(tmp_path):
    nodes = np.linspace(1.05, 1.75, 8)
    want = lc.LimbDarkening(nodes, table_at(nodes))
    obs = run_visit.build_observation(base_cfg(), base_dir=MINI)
    assert obs.ld_table is None and obs.planet.ld_table is None
    t = obs.exp_start_times[0] + np.linspace(0, 2e-4, 4)
    plain = obs.generate_lightcurves(t)
    assert obs.device_depths(t).ld_table is None
    # inline
    cfg = base_cfg()
    cfg["target"]["ld_table"] = inline(nodes)
    on = run_visit.build_observation(cfg, base_dir=MINI)
    assert on.ld_table == want and on.ldcoeffs == LD and on.planet.ldcoeffs == LD
    dd = on.device_depths(t)
    np.testing.assert_array_equal(dd.ld_table, want.on_grid(on.wl))
    np.testing.assert_array_equal(1 - on.generate_lightcurves(t), dd.host_matrix())
    assert np.abs(on.generate_lightcurves(t) - plain).max() > 1e-5
    white = on.generate_lightcurves(t, depth=0.0146)
    assert white.shape == (4, 1) and np.all(white < 1)
    del cfg["target"]["ld_table"]["law"]             # the law defaults to claret4
    assert run_visit.build_observation(cfg, base_dir=MINI).ld_table == want
    # file, resolved beside the parameter file like the section's other files
    work = tmp_path / "visit"
    import shutil
    shutil.copytree(MINI, str(work))
    np.savetxt(str(work / "ld.txt"), np.column_stack([nodes, table_at(nodes)]), fmt="%.17g")
    cfg = base_cfg()
    cfg["target"]["ld_table_file"] = "ld.txt"
    assert run_visit.build_observation(cfg, base_dir=str(work)).ld_table == want
    np.savetxt(str(work / "quad.txt"), np.column_stack([nodes, np.full(8, 0.4), np.full(8, 0.25)]))
    cfg["target"].update(ld_table_file="quad.txt", ld_law="quadratic")
    q = run_visit.build_observation(cfg, base_dir=str(work)).ld_table
    assert q.law == "quadratic" and q == lc.LimbDarkening(nodes, np.tile([0.4, 0.25], (8, 1)), "quadratic")
    # bad files and bad sections
    (work / "text.txt").write_text("wl a1 a2 a3 a4\nnot numbers\n")
    np.savetxt(str(work / "unsorted.txt"), np.column_stack([nodes[::-1], table_at(nodes)]))
    bad_targets = [dict(ld_table_file="missing.txt"), dict(ld_table_file="text.txt"), dict(ld_table_file="unsorted.txt"),
                   dict(ld_table_file="quad.txt"),                      # three columns are not claret4
                   dict(ld_table_file="ld.txt", ld_law="quadratic"), dict(ld_table_file="ld.txt", ld_law="power2"),
                   dict(ld_table_file=3), dict(ld_law="linear"),
                   dict(ld_table=inline(nodes), ld_table_file="ld.txt"), dict(ld_table=[1, 2, 3]),
                   dict(ld_table={"wl_um": [1.1, 1.7]}), dict(ld_table=dict(inline(nodes), nodes=3)),
                   dict(ld_table=inline(nodes, law="quadratic")), dict(ld_table=inline(nodes[::-1])),
                   dict(ld_table=inline(nodes, coeffs=np.tile([5.0, 0, 0, 0], (8, 1)))),
                   dict(ld_table={"wl_um": ["a", "b"], "coeffs": [[0, 0, 0, 0]] * 2})]
    for n, extra in enumerate(bad_targets):
        cfg = base_cfg()
        cfg["target"].update(copy.deepcopy(extra))
        with pytest.raises(run_visit.WFC3SimConfigError):
            # (the section's reader itself; through the whole builder for a bad file and a bad inline table)
            if n in (1, 14):
                run_visit.build_observation(cfg, base_dir=str(work))
            else:
                run_visit.ld_table_from_config(cfg["target"], lambda p: os.path.join(str(work), p))
    cfg = base_cfg()
    cfg["target"]["ld_table"] = inline(nodes)
    cfg["target"]["planet_spectrum_file"] = False        # no transit: nothing a table could act on
    with pytest.raises(run_visit.WFC3SimConfigError):
        run_visit.build_observation(cfg, base_dir=MINI)


INFO = {"SUBARRAY": 128, "NSAMP": 4, "SAMPSEQ": "RAPID", "x_ref": 460.0, "EXPSTART": 2456196.0, "filename": "0001_raw.fits"}
# sha1 over the cards (keyword, value, comment) of that header as the commit before the table wrote it, without the date
# and the version cards
CARDS_WITHOUT_TABLE = (84, "84af0fc7c12a90d8b1b06e84eb8759fb74be8088")


def test_header_cards_and_the_resume_check():
    obs = run_visit.build_observation(base_cfg(), base_dir=MINI)
    plain = exposure.Exposure(obs.detector, obs.grism, obs.planet, dict(INFO)).generate_science_header()
    keep = [(k, v, c) for k, v, c in plain.cards if k not in ("DATE", "V-PY", "V-NP", "V-SP", "SIM-VER")]
    assert (len(keep), hashlib.sha1(repr(keep).encode()).hexdigest()) == CARDS_WITHOUT_TABLE
    nodes = np.linspace(1.05, 1.75, 8)
    table = lc.LimbDarkening(nodes, table_at(nodes))
    cfg = base_cfg()
    cfg["target"]["ld_table"] = inline(nodes)
    on_obs = run_visit.build_observation(cfg, base_dir=MINI)
    on = exposure.Exposure(on_obs.detector, on_obs.grism, on_obs.planet, dict(INFO)).generate_science_header()
    assert on.cards[:len(plain.cards)][1:] == plain.cards[1:]          # (card 0 is the date)
    assert [k for k, _, _ in on.cards[len(plain.cards):]] == ["LDTABLE", "LDLAW", "LDNODES", "LDWLLO", "LDWLHI", "LDHASH"]
    assert on["LDTABLE"] is True and on["LDLAW"] == "CLARET4" and on["LDNODES"] == 8
    assert (on["LDWLLO"], on["LDWLHI"]) == (1.05, 1.75) and on["LDHASH"] == table.hash
    assert len(table.hash) == 16 and int(table.hash, 16) >= 0
    assert [on["LD%d" % n] for n in (1, 2, 3, 4)] == LD                # the fallback set stays in the header
    # the hash follows nodes and coefficients
    moved = table_at(nodes)
    moved[3, 1] += 1e-9
    assert lc.LimbDarkening(nodes, moved).hash != table.hash
    assert lc.LimbDarkening(nodes + 1e-9, table_at(nodes)).hash != table.hash
    # --resume's comparison, both directions
    assert obs._ld_cards_match(plain) and not obs._ld_cards_match(on)
    assert on_obs._ld_cards_match(on) and not on_obs._ld_cards_match(plain)
    cfg["target"]["ld_table"] = inline(nodes, coeffs=moved)
    other = run_visit.build_observation(cfg, base_dir=MINI)
    assert not other._ld_cards_match(on)


def test_resume_regenerates_files_whose_table_cards_differ(tmp_path):
    from wayne_amd import fitsio
    nodes = np.linspace(1.05, 1.75, 8)
    cfg = base_cfg()
    cfg["target"]["ld_table"] = inline(nodes)
    obs = run_visit.build_observation(cfg, base_dir=MINI)
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


def test_descriptor_carries_the_cropped_table_and_the_digest_follows_it():
    from wayne_amd import tools
    nodes = np.linspace(1.05, 1.75, 8)
    plain_obs = run_visit.build_observation(base_cfg(), base_dir=MINI)
    t0 = float(plain_obs.exp_start_times[0])
    plain, _ = _descriptor(plain_obs, t0)
    assert plain._ld_table is None and list(plain.lc_ld) == LD
    digests = {visit.descriptor_digest(plain)}
    for coeffs in (None, table_at(nodes) + 1e-12):
        cfg = base_cfg()
        cfg["target"]["ld_table"] = inline(nodes, coeffs=coeffs)
        obs = run_visit.build_observation(cfg, base_dir=MINI)
        d, dd = _descriptor(obs, t0)
        i0, i1 = tools.crop_spectrum_ind(obs.grism.wl_limits[0], obs.grism.wl_limits[1], obs.wl)
        assert d._ld_table.shape == (d.n_wl, 4) == (i1 - i0, 4)
        np.testing.assert_array_equal(d._ld_table, dd.ld_table[i0:i1])
        assert visit.descriptor_digest(d) == visit.descriptor_digest(_descriptor(obs, t0)[0])
        digests.add(visit.descriptor_digest(d))
    assert len(digests) == 3


def test_synthetic_visit_passes_a_table_through():
    import helpers
    v = helpers.make_visit("tiny")
    assert v.device_depths(0).ld_table is None
    v.ld_table = lc.LimbDarkening([1.1, 1.7], table_at([1.1, 1.7]))
    dd = v.device_depths(0)
    np.testing.assert_allclose(dd.ld_table, table_at(v.wl), rtol=0, atol=1e-15)
    runner = visit.VisitRunner(v, device_lc=True)
    d = runner.descriptor(0)
    assert d._ld_table.shape == (d.n_wl, 4)
