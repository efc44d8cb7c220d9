"""CPU: the inter-pixel capacitance law (tests/ipc_law.py) against Python big integers, its weights against the library's
wayne_ipc_weights, the refusals, the YAML forms, the header cards and the digest; and what the law does to a Poisson
field's noise.  (The device is held to the law in tests/test_ipc_gpu.py.)"""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import yaml

import helpers
import ipc_law as law
from wayne_amd import _lib, ipc, run_visit, visit as visit_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "fixtures", "mini_visit")

# every neighbour different: a transposed or flipped stencil is another kernel
ASYM = [[0.011, 0.023, 0.004], [0.031, None, 0.017], [0.002, 0.027, 0.008]]
IDENTITY = [[0, 0, 0], [0, 1, 0], [0, 0, 0]]


def shift_weights():
    w = np.zeros((3, 3), dtype=np.int64)
    w[1, 2] = law.UNIT
    return w


def test_the_law_against_big_integers():
    rng = np.random.default_rng(11)
    S = 23
    w = law.weights(ipc.InterpixelCapacitance(kernel=ASYM).kernel)
    assert len(set(w.ravel().tolist())) == 9 and int(w.sum()) == law.UNIT
    for scale in (2 ** 20, 2 ** 40, 2 ** 54, 2 ** 62):
        q = rng.integers(-scale, scale, size=(S, S), dtype=np.int64)
        q[7, 9] = 2 ** 53
        q[0, 0], q[0, -1], q[-1, 0], q[-1, -1] = 2 ** 53, -(2 ** 53) + 1, scale - 1, -scale     # the frame's corners
        q[5, :] = rng.integers(0, scale, size=S)        # ... and the first light-sensitive row
        for border in (law.BORDER, 0):                  # (border 0: the frame's edges take part, q = 0 beyond them)
            want = law.couple_bigint(q, w, border=border)
            got = law.couple(q, w, border=border)
            assert all(int(g) == int(x) for g, x in zip(got.ravel().tolist(), want.ravel().tolist())), (scale, border)
    # the extremes of int64 under the identity: nothing overflows on the way
    q = np.array([[np.iinfo(np.int64).max, np.iinfo(np.int64).min], [-1, 0]], dtype=np.int64)
    np.testing.assert_array_equal(law.couple(q, law.weights(IDENTITY), border=0), q)


def test_the_identity_kernel_returns_its_input():
    rng = np.random.default_rng(12)
    q = rng.integers(-2 ** 50, 2 ** 50, size=(3, 20, 20), dtype=np.int64)
    got = law.couple(q, law.weights(IDENTITY))
    np.testing.assert_array_equal(got[:, 5:-5, 5:-5], q[:, 5:-5, 5:-5])
    assert not got[:, :5].any() and not got[:, -5:].any() and not got[:, :, :5].any() and not got[:, :, -5:].any()


def test_a_weight_on_the_right_hand_neighbour_shifts_by_one_column():
    rng = np.random.default_rng(13)
    q = rng.integers(-2 ** 45, 2 ** 45, size=(18, 21), dtype=np.int64)
    got = law.couple(q, shift_weights())
    np.testing.assert_array_equal(got[5:-5, 5:-5], q[5:-5, 6:-4])


def test_charge_is_conserved_to_a_unit_per_pixel():
    rng = np.random.default_rng(14)
    q = np.zeros((40, 40), dtype=np.int64)
    q[12:26, 14:30] = rng.integers(0, 30000 << 28, size=(14, 16))        # an interior blob: nothing reaches the border
    for k in (ipc.InterpixelCapacitance().kernel, ipc.InterpixelCapacitance(kernel=ASYM).kernel):
        got = law.couple(q, law.weights(k))
        assert abs(int(got.sum()) - int(q.sum())) <= int((got != 0).sum())
        assert (got != 0).sum() == 16 * 18


@pytest.mark.parametrize("kernel", [ipc.InterpixelCapacitance().kernel, ipc.InterpixelCapacitance(alpha=0.0131).kernel,
                                    ipc.InterpixelCapacitance(kernel=ASYM).kernel, np.array(IDENTITY, dtype=float)])
def test_the_librarys_weights_are_the_laws(kernel):
    want = law.weights(kernel)
    np.testing.assert_array_equal(_lib.ipc_weights(kernel), want)
    np.testing.assert_array_equal(ipc.InterpixelCapacitance(kernel=kernel.tolist()).weights(), want)
    assert int(want.sum()) == law.UNIT


def test_the_default_kernel():
    d = ipc.InterpixelCapacitance()
    w = d.weights()
    assert w[0, 1] == w[1, 0] == w[1, 2] == w[2, 1] == round(0.025 * 65536) == 1638
    assert w[0, 0] == w[0, 2] == w[2, 0] == w[2, 2] == round(0.0007 * 65536) == 46
    assert w[1, 1] == 65536 - 4 * 1638 - 4 * 46
    assert abs(d.kernel[1, 1] - 0.8972) < 1e-12
    a = ipc.InterpixelCapacitance(alpha=0.02)
    np.testing.assert_array_equal(a.weights(), law.weights([[0, 0.02, 0], [0.02, 0, 0.02], [0, 0.02, 0]]))
    assert ipc.InterpixelCapacitance.from_config({}) == d and ipc.InterpixelCapacitance.from_config(None) == d
    assert ipc.as_ipc(True) == d and ipc.as_ipc(None) is None and ipc.as_ipc(d) is d


def _desc(k):
    d = _lib.IpcDesc()
    for i in range(3):
        for j in range(3):
            d.k[i][j] = k[i][j]
    return d


def test_every_refusal():
    L = _lib.load()
    w = (C.c_int32 * 9)()
    good = [[0.01, 0.02, 0.01], [0.02, 0.88, 0.02], [0.01, 0.02, 0.01]]
    assert L.wayne_ipc_weights(C.byref(_desc(good)), w) == 0
    for bad_value in (float("nan"), float("inf"), -1e-3, 0.95):         # (0.95: the neighbours then sum to more than 1)
        for (i, j) in ((0, 0), (1, 2), (2, 1)):
            k = copy.deepcopy(good)
            k[i][j] = bad_value
            assert L.wayne_ipc_weights(C.byref(_desc(k)), w) == _lib.E_INVALID, (bad_value, i, j)
            with pytest.raises(ValueError):
                law.weights(k)
            with pytest.raises(ipc.IpcConfigError):
                ipc.InterpixelCapacitance(kernel=k)
    # the centre is not the library's business ...
    k = copy.deepcopy(good)
    k[1][1] = float("nan")
    assert L.wayne_ipc_weights(C.byref(_desc(k)), w) == 0
    assert L.wayne_ipc_weights(None, w) == _lib.E_INVALID
    # ... an exactly full kernel passes, one unit more does not
    assert L.wayne_ipc_weights(C.byref(_desc([[0.125] * 3, [0.125, 0, 0.125], [0.125] * 3])), w) == 0 and w[4] == 0
    assert L.wayne_ipc_weights(C.byref(_desc([[0.125] * 3, [0.125, 0, 0.125 + 1.0 / 65536], [0.125] * 3])), w) == _lib.E_INVALID
    # Python: a centre that is given must be what the neighbours leave, to 0.01 -- else the kernel is not normalised
    ipc.InterpixelCapacitance(kernel=good)
    k = copy.deepcopy(good)
    k[1][1] = 0.88 + 0.009
    ipc.InterpixelCapacitance(kernel=k)
    for centre in (1.0, 0.86, 0.88 + 0.011):
        k[1][1] = centre
        with pytest.raises(ipc.IpcConfigError):
            ipc.InterpixelCapacitance(kernel=k)
    for kw in (dict(alpha=-0.01), dict(alpha=0.3), dict(alpha=float("nan")), dict(alpha="a"), dict(alpha=True),
               dict(kernel=[[0, 0], [0, 0]]), dict(kernel="abc"), dict(kernel=good, alpha=0.02)):
        with pytest.raises(ipc.IpcConfigError):
            ipc.InterpixelCapacitance(**kw)
    for section in ([1, 2], "x", {"beta": 1}, {"alpha": 0.02, "kernel": good}):
        with pytest.raises(ipc.IpcConfigError):
            ipc.InterpixelCapacitance.from_config(section)
    with pytest.raises(TypeError):
        ipc.as_ipc(0.02)


def _mini_cfg(section="absent"):
    cfg = yaml.safe_load(open(os.path.join(MINI, "params.yml")))
    if section != "absent":
        cfg["interpixel_capacitance"] = copy.deepcopy(section)
    return cfg


def test_the_yaml_forms():
    assert run_visit.build_observation(_mini_cfg(), base_dir=MINI).ipc is None
    assert run_visit.build_observation(_mini_cfg({}), base_dir=MINI).ipc == ipc.InterpixelCapacitance()
    assert run_visit.build_observation(_mini_cfg(None), base_dir=MINI).ipc == ipc.InterpixelCapacitance()
    obs = run_visit.build_observation(_mini_cfg({"alpha": 0.02}), base_dir=MINI)
    assert obs.ipc == ipc.InterpixelCapacitance(alpha=0.02)
    text = yaml.safe_load("interpixel_capacitance:\n  kernel: [[0.011, 0.023, 0.004], [0.031, null, 0.017], [0.002, 0.027, 0.008]]\n")
    obs = run_visit.build_observation(_mini_cfg(text["interpixel_capacitance"]), base_dir=MINI)
    assert obs.ipc == ipc.InterpixelCapacitance(kernel=ASYM)
    for bad in ({"alpha": -1}, {"gamma": 2}, [0.02]):
        with pytest.raises(run_visit.WFC3SimConfigError):
            run_visit.build_observation(_mini_cfg(bad), base_dir=MINI)


def test_the_cards_and_the_resume_check():
    m = ipc.InterpixelCapacitance(kernel=ASYM)
    cards = m.cards()
    assert [c[0] for c in cards] == ["IPC", "IPCUNIT"] + ["IPCW%d%d" % (i, j) for i in range(3) for j in range(3)]
    assert cards[0][1] is True and cards[1][1] == 65536
    assert [c[1] for c in cards[2:]] == m.weights().ravel().tolist() and all(type(c[1]) is int for c in cards[1:])
    assert all(len(c[0]) <= 8 for c in cards)
    # the header of an exposure carries them only with the option
    v = helpers.make_visit("tiny")
    for model in (None, m):
        gen = helpers.product_generator(v, 0)
        gen.build_descriptor(None, ipc=model, **v.frame_kwargs(0))
        hdr = gen.exposure.generate_science_header()
        keys = [c[0] for c in hdr.cards]
        assert ("IPC" in keys) == (model is not None) and ("IPCW12" in keys) == (model is not None)
    # --resume: a file is this visit's only when its cards are this visit's kernel, in both directions
    p_with = {c[0]: c[1] for c in cards}
    p_other = {c[0]: c[1] for c in ipc.InterpixelCapacitance().cards()}
    obs = run_visit.build_observation(_mini_cfg(), base_dir=MINI)
    assert obs._ipc_cards_match({}) and not obs._ipc_cards_match(p_with)
    obs.setup_ipc(m)
    assert obs._ipc_cards_match(p_with) and not obs._ipc_cards_match({}) and not obs._ipc_cards_match(p_other)
    obs.setup_ipc(None)
    assert obs._ipc_cards_match({})


def test_the_digest_and_the_descriptor():
    v = helpers.make_visit("tiny")
    digests = {}
    for name, model in (("none", None), ("default", True), ("asym", ipc.InterpixelCapacitance(kernel=ASYM)),
                        ("default again", ipc.InterpixelCapacitance())):
        gen = helpers.product_generator(v, 0)
        desc = gen.build_descriptor(None, ipc=model, **v.frame_kwargs(0))
        assert (desc._ipc is None) == (model is None)
        digests[name] = visit_mod.descriptor_digest(desc)
    assert digests["default"] == digests["default again"]
    assert len({digests["none"], digests["default"], digests["asym"]}) == 3
    with pytest.raises(ValueError):
        helpers.product_generator(v, 0).build_descriptor(None, ipc=True, rng_mode=_lib.RNG_REPLAY, **v.frame_kwargs(0))
    # a kernel's digest is its integer weights: two kernels that round alike are one law
    a, b = ipc.InterpixelCapacitance(alpha=0.025), ipc.InterpixelCapacitance(alpha=0.025 + 1e-9)
    assert a.digest_bytes() == b.digest_bytes() and a == b
    runner = visit_mod.VisitRunner(v, ipc=True)
    assert runner.frame_kwargs(0)["ipc"] == ipc.InterpixelCapacitance()
    assert "ipc" not in visit_mod.VisitRunner(v).frame_kwargs(0)


def test_the_struct_and_the_symbols_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "wayne_hip.h")).read()
    assert "typedef struct wayne_ipc_desc {\n  double k[3][3];" in header
    assert C.sizeof(_lib.IpcDesc) == 72
    for name in ("wayne_ipc_weights", "wayne_exposure_set_ipc", "wayne_ipc_profile"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name) and ("int %s(" % name) in header
    assert _lib.load().wayne_abi_version() == _lib.ABI_VERSION == 7


def test_a_poisson_fields_noise_under_the_default_kernel():
    """512^2 pixels of Poisson(1000) e-: a pixel keeps sum W^2 = 0.8075 of its variance and gains a correlation of 0.0556
    with each edge neighbour (the law's own numbers: sum_ij W_ij^2 and sum_ij W_ij W_i,j+1 / sum W^2 of the default
    kernel).  Bounds: the variance of n samples is known to sqrt(2 / n) of itself, a correlation to 1 / sqrt(n); 4 sigma."""
    rng = np.random.default_rng(15)
    S = 512 + 2 * law.BORDER
    q = rng.poisson(1000.0, size=(S, S)).astype(np.int64) << 28
    w = law.weights(ipc.InterpixelCapacitance().kernel)
    # (the border holds the same field: the light-sensitive pixels beside it receive from it like any other)
    got = law.couple(q, w)[law.BORDER:-law.BORDER, law.BORDER:-law.BORDER].astype(np.float64) / 2.0 ** 28
    n = got.size
    assert n == 512 * 512
    ratio = got.var() / 1000.0                       # (a Poisson field's variance is its mean)
    assert abs(ratio - 0.8075) <= 4 * 0.8075 * np.sqrt(2.0 / n), ratio
    d = got - got.mean()
    for a, b in ((d[:, :-1], d[:, 1:]), (d[:-1, :], d[1:, :])):
        corr = (a * b).mean() / d.var()
        assert abs(corr - 0.0556) <= 4.0 / np.sqrt(n), corr
    # the stated numbers are the kernel's
    wf = w.astype(np.float64) / law.UNIT
    assert abs((wf ** 2).sum() - 0.8075) < 5e-4
    assert abs((wf[:, :-1] * wf[:, 1:]).sum() / (wf ** 2).sum() - 0.0556) < 5e-4
