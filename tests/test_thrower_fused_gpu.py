"""GPU: k_lane and k_narrow of the production pair as ONE grid (k_thrower, knob fuse_thrower, the default) against the
two launches (fuse_thrower = 0).

Both roles run the code they run alone -- the same bodies on the same LDS buffer, the same streams keyed by bin and
sub-sample, not by workgroup -- and every deposit is an integer add into the frame or the accumulators: the two
settings must give the SAME frame and the SAME reads, bit for bit (np.array_equal, no tolerance), in whatever order the
hardware hands out the workgroups.

FLUSH 0 (ctx.psf_apply) is launched as one grid when the call has a bin for each kernel; FLUSH 1 (whole exposures) when
k_lane and k_narrow would follow each other on the slot's stream in their production form.  Which launch sequence a case
took is read off the profile slots where the case is about that: k_narrow's slot records nothing under one grid.
"""
import numpy as np
import pytest

import helpers
from wayne_amd import _lib

pytestmark = pytest.mark.gpu


def launches(ctx, call):
    """(result of call(), launches recorded per profile slot while it ran)"""
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = call()
        p = ctx.profile_get()
    finally:
        ctx.profile_enable(False)
    return out, {k: int(v["launches"]) for k, v in p.items() if isinstance(v, dict) and "launches" in v}


def fused_and_split(ctx, counts, x, y, ratio, sl, sh, N, seed, exp=0, sub=0, exact=False, one_grid=True):
    """The frame of one psf_apply call with the knob on == with it off (and on again).  `one_grid`: whether the call is
    expected to take the combined launch with the knob on.  Returns the frame (N x N)."""
    counts = np.asarray(counts, dtype=np.int32)
    frames, seen = [], []
    for knob in (1, 0, 1):
        _lib.set_knob_all("fuse_thrower", knob)
        f, n = launches(ctx, lambda: ctx.psf_apply(counts, x, y, ratio, sl, sh, N, N, seed, rng_mode=_lib.RNG_SPLIT,
                                                   exposure=exp, subsample=sub, exact_samplers=exact))
        frames.append(f)
        seen.append(n)
    assert np.array_equal(frames[0], frames[1]), "%d pixels differ" % int((frames[0] != frames[1]).sum())
    assert np.array_equal(frames[0], frames[2])
    if one_grid:
        assert seen[0]["k_narrow"] == 0 and seen[0]["k_lane"] == 1, seen[0]
        assert seen[1]["k_narrow"] == 1 and seen[1]["k_lane"] == 1, seen[1]
    else:
        assert seen[0] == seen[1], (seen[0], seen[1])
    return frames[0].reshape(N, N)


def trace(W, seed, lo=1400, hi=1600):
    rng = np.random.default_rng(seed)
    counts = rng.integers(lo, hi, W).astype(np.int32)
    x = 30.3 + 0.04 * np.arange(W)
    y = 60.7 + 0.0007 * np.arange(W)
    return counts, x, y, np.full(W, 0.2), np.full(W, 0.6), np.full(W, 4.0)


def test_trace_over_three_workgroups_per_role(gpu_ctx):
    # the trace of test_narrow_compact_gpu.test_trace_over_three_workgroups: 2 x 512 + 40 bins, three chunks per role,
    # the last ragged
    W, N = 2 * 512 + 40, 128
    counts, x, y, ratio, sl, sh = trace(W, 5)
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 77, 3, 11)
    assert f.sum() == counts.sum()                               # (the trace is far from every edge)


@pytest.mark.parametrize("W", [1, 513])
def test_one_bin_and_one_bin_past_a_chunk(gpu_ctx, W):
    N = 128
    counts, x, y, ratio, sl, sh = trace(W, 6)
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 13, 1, 2)
    assert f.sum() == counts.sum()


def test_every_bin_thin_the_narrow_role_finds_nothing(gpu_ctx):
    # bins of 20-30 narrow electrons (below kSplitMin = 32): no bin for k_narrow, the call launches k_lane alone under
    # either setting ...
    W, N = 2 * 512 + 40, 128
    counts, x, y, ratio, sl, sh = trace(W, 7, 25, 38)
    assert ((counts - (counts * ratio).astype(np.int32)) < 32).all()
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 5, 0, 1, one_grid=False)
    assert f.sum() == counts.sum()
    # ... and with ONE multinomial bin, in the last chunk, the combined grid is launched: the narrow workgroups of the
    # first two chunks find nothing and leave at their first barrier
    counts[2 * 512 + 7] = 900
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 5, 0, 1)
    assert f.sum() == counts.sum()


def test_ratio_zero_the_lane_role_finds_nothing(gpu_ctx):
    # ratio = 0 with large counts: every electron is narrow and goes to the multinomials, no bin for k_lane; the call
    # launches k_narrow alone under either setting ...
    W, N = 2 * 512 + 40, 128
    counts, x, y, ratio, sl, sh = trace(W, 8, 20000, 30000)
    ratio[:] = 0.0
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 6, 2, 3, one_grid=False)
    assert f.sum() == counts.sum()
    # ... and with a wide fraction in the first chunk only, the lane workgroups of the other two find nothing
    ratio[:512] = 0.1
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 6, 2, 3)
    assert f.sum() == counts.sum()


def test_a_chunk_at_the_frames_corner(gpu_ctx):
    # the first chunk hugs the corner (1, 1), the second the opposite one: tiles clipped by the frame, bounds-tested
    # lanes, electrons lost off the frame -- the same ones either way
    W, N = 2 * 512, 96
    counts, x, y, ratio, sl, sh = trace(W, 9)
    x[:512] = 1.2 + 0.01 * np.arange(512); y[:512] = 1.4 + 0.001 * np.arange(512)
    x[512:] = N - 6.5 + 0.01 * np.arange(512); y[512:] = N - 1.3 - 0.001 * np.arange(512)
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 31, 4, 5)
    assert 0 < f.sum() < counts.sum()
    assert f[0].sum() == 0 and f[:, 0].sum() == 0                # (pixel row / column 0 is never hit)


def test_exact_samplers_take_the_two_launches(gpu_ctx):
    W, N = 2 * 512 + 40, 128
    counts, x, y, ratio, sl, sh = trace(W, 5)
    f = fused_and_split(gpu_ctx, counts, x, y, ratio, sl, sh, N, 77, 3, 11, exact=True, one_grid=False)
    assert f.sum() == counts.sum()


# ---- FLUSH 1: whole exposures ----

def exposure_reads(name, dtype, knobs=(1, 0), contaminants=None, other_knob=None):
    """The reads of exposure 0 of visit `name` under each setting of fuse_thrower (uploaded afresh each time), the
    launches recorded per profile slot for each, and the re-runs each caused."""
    v = helpers.make_visit(name)
    pg = helpers.product_generator(v, 0)
    pg.prepare(rng_mode=_lib.RNG_SPLIT, out_dtype=dtype, **v.frame_kwargs(0))
    eng, desc, _ = pg._prepared
    pg._prepared = None
    ctx = eng.ctx
    if other_knob:
        _lib.set_knob_all(*other_knob)
    reads, seen, reruns = [], [], []

    def once():
        ctx.upload(0, desc)
        if contaminants is not None:
            ctx.set_sources(0, contaminants(desc))
        ctx.run(0)
        return ctx.download(0).copy()
    for knob in knobs:
        _lib.set_knob_all("fuse_thrower", knob)
        n0 = ctx.reruns
        r, n = launches(ctx, once)
        reads.append(r)
        seen.append(n)
        reruns.append(ctx.reruns - n0)
    assert reads[0].dtype == dtype
    return reads, seen, reruns


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["small256", "stare256"])
def test_whole_exposures_scanning_and_staring(name, dtype):
    reads, seen, _ = exposure_reads(name, dtype, knobs=(1, 0, 1))
    np.testing.assert_array_equal(reads[0], reads[1])
    np.testing.assert_array_equal(reads[0], reads[2])
    assert reads[0][-1].max() > 5
    # one grid per exposure with the knob on (k_narrow's slot records nothing), two launches with it off
    assert seen[0]["k_narrow"] == 0 and seen[0]["k_lane"] == 1, seen[0]
    assert seen[1]["k_narrow"] == 1 and seen[1]["k_lane"] == 1, seen[1]


def test_whole_exposure_with_a_contaminant():
    from wayne_amd.sources import Contaminant

    def stars(desc):
        wl, fl = desc._keep[0], desc._keep[1]      # (make_desc keeps the cropped wl and flux first)
        return [Contaminant(25.0, -30.0, wl.copy(), fl * 0.5 * (1.0 + 1.0 * (wl - wl.mean())), 1)]
    reads, seen, _ = exposure_reads("small256", np.float32, contaminants=stars)
    np.testing.assert_array_equal(reads[0], reads[1])
    assert seen[0]["k_narrow"] == 0 and seen[0]["k_lane"] == 2, seen[0]       # target and contaminant: a grid each
    assert seen[1]["k_narrow"] == 2 and seen[1]["k_lane"] == 2, seen[1]


def test_whole_exposure_without_compacted_chains_takes_the_two_launches():
    reads, seen, _ = exposure_reads("small256", np.float32, other_knob=("narrow_compact", 0))
    np.testing.assert_array_equal(reads[0], reads[1])
    assert seen[0] == seen[1] and seen[0]["k_narrow"] == 1, (seen[0], seen[1])


def test_the_rerun_with_k_throw_is_the_same():
    # lane_reach = 5: the first run meets a bin beyond the lanes' reach and the exposure is run again, with k_throw, when
    # its status is read -- the same reads, and as many re-runs, with one grid as with two launches
    reads, seen, reruns = exposure_reads("small256", np.float32, other_knob=("lane_reach", 5))
    np.testing.assert_array_equal(reads[0], reads[1])
    assert reruns[0] == reruns[1] and reruns[0] >= 1, reruns
    _lib.set_knob_all("lane_reach", None)
    plain, _, none = exposure_reads("small256", np.float32, knobs=(1,))
    np.testing.assert_array_equal(reads[0], plain[0])
    assert none == [0]
