"""GPU: k_lane's test-free tiles sized for the 16-bit radius (knob lane_tight_tile, the default) against tiles sized
for the refined radius (lane_tight_tile = 0).

An electron's word, radius, direction and pixel do not depend on the tile; only the route of the one electron in 65536
whose radius is refined (h = 0, up to 6.87 sigma) does: LDS tile or checked deposit, and integer accumulation commutes.
So the two settings must give the SAME frame, bit for bit, with the fast and with the exact samplers, and the
exact-sampler frame is held to oracle/split_oracle.c on the same counters, within helpers.split_moved_bound.

Every bin here holds at most 4000 one-by-one electrons (kLaneMax = 4096), so that k_lane, not k_throw, throws them.
The tile rule (k_narrow.h, lane_body): the bins' bounding box +- ceil(reach x sigma_max + 1) px, test-free when that is
at most kLaneReachMax = 48, fits kLaneTile = 9216 cells and lies inside the frame; reach = kLaneR16 = 4.63 or 6.9.
"""
import math

import numpy as np
import pytest

import helpers
from wayne_amd import _lib

pytestmark = pytest.mark.gpu

R16, R34, TILE, REACH_MAX = 4.63, 6.9, 9216, 48


def tile_is_test_free(x, y, smax, N, reach):
    """The tile rule for one workgroup's bins (positions in frame pixels)."""
    m = math.ceil(np.float32(reach) * np.float32(smax) + np.float32(1.0))
    ix, iy = np.floor(x).astype(int), np.floor(y).astype(int)
    x0, x1, y0, y1 = ix.min() - m, ix.max() + m + 1, iy.min() - m, iy.max() + m + 1
    return m <= REACH_MAX and x0 >= 1 and y0 >= 1 and x1 <= N and y1 <= N and (x1 - x0) * (y1 - y0) <= TILE


def on_off_and_oracle(ctx, counts, x, y, ratio, sl, sh, N, seed, exp=0, sub=0, want=None):
    """The frame with the knob on == the frame with it off, fast and exact samplers; the exact one against the oracle.
    Returns the fast-sampler frame and the oracle's (N x N)."""
    from oracle import clib
    counts = np.asarray(counts, dtype=np.int32)
    assert counts.max() <= 4000
    if want is None:
        want = clib.psf_split_oracle(counts, x, y, ratio, sl, sh, N, seed, exp, sub)
    frames = {}
    for exact in (False, True):
        for knob in (1, 0):
            _lib.set_knob_all("lane_tight_tile", knob)
            frames[exact, knob] = ctx.psf_apply(counts, x, y, ratio, sl, sh, N, N, seed, rng_mode=_lib.RNG_SPLIT,
                                                exposure=exp, subsample=sub, exact_samplers=exact)
        assert np.array_equal(frames[exact, 1], frames[exact, 0]), "exact_samplers=%s: %d pixels differ" % (
            exact, int((frames[exact, 1] != frames[exact, 0]).sum()))
    total = int(want.sum())
    got = frames[True, 1]
    assert abs(int(got.sum()) - total) <= 2 + total // 100000
    moved = int(np.abs(got.astype(np.int64) - want).sum()) // 2
    bound = helpers.split_moved_bound(counts, total, exact=True)
    print("moved %d of %d electrons (bound %.1f)" % (moved, total, bound))
    assert moved <= bound, "%d of %d electrons moved" % (moved, total)
    return frames[False, 1].reshape(N, N), np.asarray(want).reshape(N, N)


def trace(W, x0, y0, rng):
    counts = rng.integers(1400, 1600, W).astype(np.int32)
    x = x0 + 0.04 * np.arange(W)
    y = y0 + 0.0007 * np.arange(W)
    return counts, x, y, np.ones(W), np.full(W, 0.7), np.full(W, 6.5)


def test_a_tile_that_was_tested_and_is_now_test_free(gpu_ctx):
    # 2 x 512 + 40 trace-like bins, every electron wide (ratio 1): three workgroups, the last ragged.  At sigma_h = 6.5
    # the margin is 32 px with the knob on (tile ~87 x 66) and 46 px with it off (114 x 94 > kLaneTile: bounds-tested)
    W, N = 2 * 512 + 40, 256
    counts, x, y, ratio, sl, sh = trace(W, 100.3, 128.7, np.random.default_rng(5))
    for lo in range(0, W, 512):
        s = slice(lo, lo + 512)
        assert tile_is_test_free(x[s], y[s], 6.5, N, R16)
        # (the 40 bins of the ragged workgroup span two pixels: their tile fits under either rule)
        assert tile_is_test_free(x[s], y[s], 6.5, N, R34) == (lo == 1024)
    f, _ = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 77, 3, 11)
    assert f.sum() == counts.sum()                               # (the trace is far from every edge)


_far = {}


def far_tail_case():
    """4096 all-wide bins of 4000 electrons at one position, sigma_h = 6.8, and the oracle's frame (computed once)."""
    if not _far:
        from oracle import clib
        W, N = 4096, 128
        counts = np.full(W, 4000, np.int32)
        x, y = np.full(W, 64.3), np.full(W, 64.6)
        ratio, sl, sh = np.ones(W), np.full(W, 0.7), np.full(W, 6.8)
        want = clib.psf_split_oracle(counts, x, y, ratio, sl, sh, N, 2024, 1, 5)
        _far.update(args=(counts, x, y, ratio, sl, sh, N, 2024, 1, 5), want=want)
    return _far["args"], _far["want"]


def outside_square(frame, cx, cy, half):
    """Electrons of `frame` (N x N, [row = y, column = x]) outside the pixels within `half` of (cx, cy)."""
    inside = frame[cy - half:cy + half + 1, cx - half:cx + half + 1].sum()
    return int(frame.sum() - inside)


def test_far_tail_out_of_the_tile(gpu_ctx):
    # 1.6e7 electrons from one pixel: 1.5e-5 of them have a refined radius and ~11 % of those land outside the square of
    # half-side ceil(4.63 sigma + 1) = 33 px that is the workgroups' test-free tile: they take the global path
    args, want = far_tail_case()
    N = args[6]
    half = math.ceil(R16 * 6.8 + 1)
    assert half == 33 and tile_is_test_free(args[1][:512], args[2][:512], 6.8, N, R16)
    w2 = np.asarray(want).reshape(N, N)
    n_out_oracle = outside_square(w2, 64, 64, half)
    print("oracle: %d electrons outside the tile" % n_out_oracle)
    assert n_out_oracle >= 20                                    # settled on the CPU, before any GPU run
    f, _ = on_off_and_oracle(gpu_ctx, *args, want=want)
    n_out = outside_square(f, 64, 64, half)
    print("device: %d electrons outside the tile" % n_out)
    assert n_out > 0
    assert f.sum() == args[0].sum()
    # nothing beyond 6.87 sigma + 1
    assert outside_square(f, 64, 64, math.ceil(6.87 * 6.8 + 1)) == 0


def test_frame_edge(gpu_ctx):
    # the same trace 10 px from a corner: no tile lies inside the frame, both rules keep the bounds test, electrons off
    # the frame are dropped as in the oracle
    W, N = 2 * 512 + 40, 128
    counts, x, y, ratio, sl, sh = trace(W, 10.3, 10.7, np.random.default_rng(6))
    assert not tile_is_test_free(x[:512], y[:512], 6.5, N, R16) and not tile_is_test_free(x[:512], y[:512], 6.5, N, R34)
    f, want = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 78, 0, 2)
    assert 0.5 * counts.sum() < f.sum() < 0.999 * counts.sum()   # a good part fell off the frame
    assert f[0].sum() == 0 and f[:, 0].sum() == 0                # (:93: row and column 0 take nothing)


def test_two_sigmas_in_one_wave(gpu_ctx):
    # thin bins below kSplitMin (all their electrons one by one, narrow and wide) beside multinomial bins (only the
    # wide fifth one by one) in every wave: sigma is chosen per electron in a test-free workgroup
    rng = np.random.default_rng(8)
    W, N = 512 + 200, 192
    counts = np.where(np.arange(W) % 3 == 0, rng.integers(1, 31, W), rng.integers(1400, 1600, W)).astype(np.int32)
    x = 80.3 + 0.04 * np.arange(W)
    y = 96.7 + 0.0007 * np.arange(W)
    ratio, sl, sh = np.full(W, 0.2), np.full(W, 0.7), np.full(W, 6.5)
    assert tile_is_test_free(x[:512], y[:512], 6.5, N, R16) and not tile_is_test_free(x[:512], y[:512], 6.5, N, R34)
    f, _ = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 79, 2, 3)
    assert f.sum() == counts.sum()


def test_a_lane_that_is_not_live(gpu_ctx):
    # workgroup 0: mostly empty bins and one bin whose sigma_h is not finite -- its reach is not finite either, the
    # workgroup is never test-free and its waves take the general loop; workgroup 1: an ordinary trace with empty bins
    # among the populated ones (lanes that run out before their neighbours in a test-free tile)
    rng = np.random.default_rng(9)
    W, N = 512 + 300, 192
    counts = rng.integers(1400, 1600, W).astype(np.int32)
    counts[:512][np.arange(512) % 4 != 1] = 0
    counts[512:][np.arange(300) % 5 == 2] = 0
    x = 80.3 + 0.04 * np.arange(W)
    y = 96.7 + 0.0007 * np.arange(W)
    ratio, sl, sh = np.full(W, 0.5), np.full(W, 0.7), np.full(W, 6.5)
    sh[37] = np.inf
    assert counts[37] > 0
    f, _ = on_off_and_oracle(gpu_ctx, counts, x, y, ratio, sl, sh, N, 80, 4, 1)
    assert f.sum() < counts.sum()                                # (the wide electrons of bin 37 are kept nowhere)


def exposure_reads(pg, kw, knobs, **more):
    reads = []
    for knob in knobs:
        _lib.set_knob_all("lane_tight_tile", knob)
        e = pg.scanning_frame(rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **dict(kw, **more))
        reads.append(np.stack([r[0] for r in e.reads]))
    return reads


def test_whole_exposure_is_the_same_with_the_knob_on_and_off():
    # one exposure of a small configuration (SUBARRAY 256, K = 9 sub-samples), split mode, float32 reads: bit-identical
    # with the knob on and off, and from run to run
    v = helpers.make_visit("small256")
    pg = helpers.product_generator(v, 0)
    reads = exposure_reads(pg, v.frame_kwargs(0), (1, 0, 1))
    assert reads[0].dtype == np.float32 and reads[0].max() > 0
    np.testing.assert_array_equal(reads[0], reads[1])
    np.testing.assert_array_equal(reads[0], reads[2])


def test_whole_thin_exposure_through_the_fused_kernel():
    # the same visit fifty times fainter: a few electrons per bin and sub-sample, thrown by k_lane_fused (THIN + BATCH;
    # tests/test_soak_gpu.py, test_fused_thin_path_equals_the_three_kernel_path, holds that path to the unfused one)
    v = helpers.make_visit("small256")
    pg = helpers.product_generator(v, 0)
    kw = v.frame_kwargs(0, scale_factor=0.02)
    rec = {}
    pg.scanning_frame(rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, record=rec, **kw)
    assert rec["counts"].max() < 32 and rec["counts"].sum() > 1000
    reads = exposure_reads(pg, kw, (1, 0, 1))
    np.testing.assert_array_equal(reads[0], reads[1])
    np.testing.assert_array_equal(reads[0], reads[2])
    # and unfused, with the first-touch list and batches forced (k_lane<.., THIN, BATCH>)
    _lib.set_knob_all("no_fuse", 1)
    _lib.set_knob_all("thin", 1)
    _lib.set_knob_all("batch", 4)
    unfused = exposure_reads(pg, kw, (1, 0))
    np.testing.assert_array_equal(unfused[0], unfused[1])
    np.testing.assert_array_equal(unfused[0], reads[0])
