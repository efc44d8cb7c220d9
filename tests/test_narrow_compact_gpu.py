"""GPU: k_narrow's compacted pooled row chains (knob narrow_compact, the default) against the per-group chains
(narrow_compact = 0).

A pooled chain is a function of its own stream, its start count and its group's tables, none of which depends on the
lane that runs it, and its deposits are integer atomics: the two settings must give the SAME frame, bit for bit, with
the fast and with the exact samplers.  The exact-sampler frame is also held to oracle/split_oracle.c on the same
counters, within helpers.split_moved_bound.

What decides the length of a workgroup's list: a slot is live when its pooled column received an electron.  A group's
window has 16 columns, X0 .. X0 + 15, X0 = (leftmost bin's column) - 6, and a pooling group's bins span at most three
columns, so the column chain reaches X0 .. X0 + 14: slot 15 of a group never holds electrons and the longest possible
list has 32 x 15 = 480 entries, not 512.  Bins wider than sigma_l = 6 / 6.5 px do not take the multinomial at all
(k_prep, so_bin: 6.5 sigma must fit the window), so the list is fullest at sigma_l = 0.92 with as many electrons as a
group may pool (2^24): ~13 live columns per group, ~416 entries -- `test_fullest_list`.
"""
import numpy as np
import pytest

import helpers
from wayne_amd import _lib

pytestmark = pytest.mark.gpu


def on_off_and_oracle(ctx, counts, x, y, ratio, sl, sh, N, seed, exp=0, sub=0, bound_counts=None):
    """The frame with the knob on == the frame with it off, fast and exact samplers; the exact one against the oracle.
    Returns the fast-sampler frame (N x N)."""
    from oracle import clib
    counts = np.asarray(counts, dtype=np.int32)
    frames = {}
    for exact in (False, True):
        for knob in (1, 0):
            _lib.set_knob_all("narrow_compact", knob)
            frames[exact, knob] = ctx.psf_apply(counts, x, y, ratio, sl, sh, N, N, seed, rng_mode=_lib.RNG_SPLIT,
                                                exposure=exp, subsample=sub, exact_samplers=exact)
        assert np.array_equal(frames[exact, 1], frames[exact, 0]), "exact_samplers=%s: %d pixels differ" % (
            exact, int((frames[exact, 1] != frames[exact, 0]).sum()))
    want = clib.psf_split_oracle(counts, x, y, ratio, sl, sh, N, seed, exp, sub)
    total = int(want.sum())
    got = frames[True, 1]
    assert abs(int(got.sum()) - total) <= 2 + total // 100000
    moved = int(np.abs(got.astype(np.int64) - want).sum()) // 2
    bound = helpers.split_moved_bound(counts if bound_counts is None else bound_counts, total, exact=True)
    print("moved %d of %d electrons (bound %.1f)" % (moved, total, bound))
    assert moved <= bound, "%d of %d electrons moved" % (moved, total)
    return frames[False, 1].reshape(N, N)


def test_every_pooling_rule_in_one_launch(gpu_ctx):
    # the geometry of test_split_gpu.test_pooled_row_groups_against_oracle_same_counters: pooling and non-pooling
    # groups in one wave, a ragged last group, windows clipped by the frame's corners, far-off positions, a group
    # disqualified by its total
    rng = np.random.default_rng(17)
    G, N = 16, 192
    W = 16 * G + 5
    g = np.arange(W) // G
    j = np.arange(W) % G
    counts = rng.integers(900, 2600, W).astype(np.int64)
    x = 30.3 + 0.04 * np.arange(W)
    y = 90.7 + 0.0007 * np.arange(W)
    sl = 0.66 + 0.0002 * np.arange(W)
    sh = np.full(W, 4.0)
    ratio = np.full(W, 0.2)
    m = g == 4; x[m], y[m], sl[m] = 70.25, 91.5, 0.7
    m = g == 5; y[m] = 60.1 + 0.24 * 0.7 * j[m] / 15.0; sl[m] = 0.7
    m = g == 6; y[m] = 60.1 + 0.27 * 0.7 * j[m] / 15.0; sl[m] = 0.7
    m = g == 7; sl[m] = 0.6 * (1 + 0.12 * j[m] / 15.0)
    m = g == 8; x[m] = 100.2 + 0.21 * j[m]
    m = g == 9; counts[m] = np.where(j[m] == 7, 5000, rng.integers(0, 20, m.sum()))
    m = g == 10; counts[m] = np.where(j[m] % 3 == 0, rng.integers(0, 30, m.sum()), counts[m])
    m = g == 11; x[m] = 1.4 + 0.04 * j[m]; y[m] = 2.2 + 0.001 * j[m]
    m = g == 12; x[m] = 150.0 + 0.04 * j[m]; y[m] = N - 1.6 + 0.001 * j[m]
    m = g == 13; sl[m] = np.where(j[m] < 8, 0.0505, 0.92)
    m = g == 14; counts[m] = np.where(j[m] == 3, (1 << 24) + 77, counts[m]); ratio[m] = 0.0
    m = g == 15; x[m] = np.where(j[m] % 2 == 0, 5e7, x[m]); y[m] = np.where(j[m] % 4 == 1, -3e8, y[m])
    counts = counts.astype(np.int32)
    # (bin 14/3 holds 2^24 + 77 electrons, but it is thrown one by one: the largest CHAIN is an ordinary group's)
    on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 42, 5, 99, bound_counts=np.minimum(counts, 5000))


def test_trace_over_three_workgroups(gpu_ctx):
    # 2 x 512 + 40 trace-like bins: three workgroups, the last ragged; ~200 live chains in a full one, so the list
    # spans several waves and ends inside one
    rng = np.random.default_rng(5)
    W, N = 2 * 512 + 40, 128
    counts = rng.integers(1400, 1600, W).astype(np.int32)
    x = 30.3 + 0.04 * np.arange(W)
    y = 60.7 + 0.0007 * np.arange(W)
    sl, sh, ratio = np.full(W, 0.6), np.full(W, 4.0), np.full(W, 0.2)
    f = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 77, 3, 11)
    assert f.sum() == counts.sum()                               # (the trace is far from every edge)


def test_fullest_list(gpu_ctx):
    # the longest list a workgroup can have (module docstring): 512 bins of 10^6 narrow electrons -- a group's total is
    # 1.6e7 <= 2^24 --, sigma_l = 0.92, x spread over three columns per group.  Each group sits in rows of its own and
    # its bins share one height and one sigma (no residual electrons), ratio = 0 (nothing thrown one by one): a column
    # of a group's rows holds electrons exactly when its chain was live.
    W, N = 512, 32 * 16 + 16
    g, j = np.arange(W) // 16, np.arange(W) % 16
    counts = np.full(W, 1000000, np.int32)
    x = 100.05 + 2.9 * j / 15.0
    y = 8.5 + 16.0 * g
    sl, sh, ratio = np.full(W, 0.92), np.full(W, 4.0), np.zeros(W)
    f = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 9, 1, 2)
    live = sum(int(np.count_nonzero(f[16 * k:16 * k + 16].sum(axis=0))) for k in range(32))
    print("live chains:", live)
    # (12 columns of a group expect hundreds of electrons or more, the 13th ~10: the list reaches into the seventh wave)
    assert live > 6 * 64


def test_one_live_column_and_idle_workgroups(gpu_ctx):
    # workgroup 0: every bin below kSplitMin except two neighbours of 40 electrons, so narrow that one column takes
    # them all -- one pooling group, one live chain, seven waves without a multinomial bin; workgroup 1: lone
    # multinomial bins, no pooling group at all; workgroup 2 (ragged): nothing for k_narrow.  Everyone must get past
    # the barriers.
    rng = np.random.default_rng(3)
    W, N = 3 * 512 - 7, 96
    counts = rng.integers(0, 12, W).astype(np.int32)
    x = 20.5 + 0.03 * np.arange(W)
    y = np.full(W, 40.5)
    sl, sh, ratio = np.full(W, 0.7), np.full(W, 3.0), np.zeros(W)
    counts[100:102] = 40
    x[100:102], y[100:102], sl[100:102] = 30.5, 70.5, 0.06
    for b in (512 + 50, 512 + 300, 512 + 301 + 16):
        counts[b] = 600
    f = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 21, 0, 4)
    assert f[70, 30] == 80 and f[64:77].sum() == 80              # the one chain: 80 electrons, one pixel


@pytest.mark.parametrize("length", [64, 65])
def test_list_ends_at_a_wave_boundary_or_one_past_it(gpu_ctx, length):
    # 22 groups in rows of their own, bins of a group identical (no residuals), ratio = 0.  21 groups at sigma_l = 0.3
    # in mid-pixel: 1600 electrons over the columns -1, 0, +1 with masses 0.048, 0.904, 0.048 (the next ones 3e-7):
    # three live chains each.  The last group at sigma_l = 0.06: every electron in its bin's own column -- one column
    # (list of 64: exactly one wave) or two (65: one chain in the second wave).
    G = 22
    W, N = 16 * G, 16 * G + 16
    g, j = np.arange(W) // 16, np.arange(W) % 16
    counts = np.full(W, 100, np.int32)
    x = np.full(W, 100.5)
    y = 8.5 + 16.0 * g
    sl, sh, ratio = np.full(W, 0.3), np.full(W, 3.0), np.zeros(W)
    sl[g == G - 1] = 0.06
    if length == 65:
        x[(g == G - 1) & (j >= 8)] = 101.5
    f = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 12, 2, 7)
    assert f.sum() == counts.sum()
    live = [int(np.count_nonzero(f[16 * k:16 * k + 16].sum(axis=0))) for k in range(G)]
    assert live[:-1] == [3] * (G - 1) and sum(live) == length, live


def test_whole_exposure_is_the_same_with_the_knob_on_and_off():
    # one exposure of a small configuration (SUBARRAY 256, K = 9 sub-samples), split mode, float32 reads: bit-identical
    # with the knob on and off, and from run to run
    v = helpers.make_visit("small256")
    pg = helpers.product_generator(v, 0)
    kw = v.frame_kwargs(0)
    reads = []
    rec = {}
    for knob in (1, 0, 1):
        _lib.set_knob_all("narrow_compact", knob)
        e = pg.scanning_frame(rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, record=rec if not reads else None, **kw)
        reads.append(np.stack([r[0] for r in e.reads]))
    assert reads[0].dtype == np.float32
    # (bins of >= 64 electrons take the multinomial -- kSplitMin = 32 narrow ones, the wide fraction is below a half --
    # and neighbours on a trace pool: k_narrow's pooled phase has work)
    assert (np.asarray(rec["counts"]) >= 64).sum() > 100
    np.testing.assert_array_equal(reads[0], reads[1])
    np.testing.assert_array_equal(reads[0], reads[2])
