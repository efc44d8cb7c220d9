"""wayne_amd.pipeline.run_pipelined on the CPU: a stand-in context that records the calls it gets."""
import sys
import threading

import pytest

from wayne_amd.pipeline import run_pipelined


class RecordingCtx(object):
    """upload / run / fetch_async / wait and nothing else: all the loop may use."""

    def __init__(self):
        self.calls, self.slots, self.threads = [], {}, set()

    def upload(self, slot, desc):
        assert slot not in self.slots, "slot %d uploaded again before its reads were waited for" % slot
        self.slots[slot] = desc
        self.calls.append(("upload", slot))
        self.threads.add(threading.get_ident())

    def run(self, slot):
        self.calls.append(("run", slot))

    def fetch_async(self, slot):
        self.calls.append(("fetch_async", slot))

    def wait(self, slot):
        self.calls.append(("wait", slot))
        return "reads of %s" % self.slots.pop(slot)


@pytest.mark.parametrize("depth,n_slots", [(3, 4), (4, 4), (1, 2)])
def test_every_job_is_launched_in_order_and_finished_oldest_first(depth, n_slots):
    ctx, finished, prepared_on, most = RecordingCtx(), [], set(), [0]
    jobs = [7, 3, 0, 2, 4, 9, 1, 8, 5]

    def prepare(job):
        prepared_on.add(threading.get_ident())
        return "desc %d" % job, {"job": job}

    def finish(job, state, reads):
        most[0] = max(most[0], len(ctx.slots) + 1)
        assert state == {"job": job} and reads == "reads of desc %d" % job
        finished.append(job)

    before, n_threads = sys.getswitchinterval(), threading.active_count()
    run_pipelined(ctx, iter(jobs), prepare, finish, depth, n_slots)
    assert finished == jobs
    assert [c for c in ctx.calls if c[0] != "wait"] == [
        (what, n % n_slots) for n in range(len(jobs)) for what in ("upload", "run", "fetch_async")]
    assert [s for what, s in ctx.calls if what == "wait"] == [n % n_slots for n in range(len(jobs))]
    assert most[0] == depth and not ctx.slots
    assert ctx.threads == {threading.get_ident()} and prepared_on.isdisjoint(ctx.threads)
    assert sys.getswitchinterval() == before and threading.active_count() == n_threads


def test_no_jobs():
    ctx = RecordingCtx()
    run_pipelined(ctx, [], None, None, 3, 4)
    assert ctx.calls == []


def test_an_error_of_prepare_is_raised_in_the_caller_after_the_jobs_before_it():
    ctx, finished = RecordingCtx(), []

    def prepare(job):
        if job == 2:
            raise KeyError("job 2")
        return job, None

    before, n_threads = sys.getswitchinterval(), threading.active_count()
    with pytest.raises(KeyError, match="job 2"):
        run_pipelined(ctx, range(10), prepare, lambda job, state, reads: finished.append(job), 3, 4)
    assert [c for c in ctx.calls if c[0] == "upload"] == [("upload", 0), ("upload", 1)]
    assert sys.getswitchinterval() == before and threading.active_count() == n_threads


def test_an_error_of_finish_stops_the_producer():
    ctx, prepared = RecordingCtx(), []

    def prepare(job):
        prepared.append(job)
        return job, None

    def finish(job, state, reads):
        raise RuntimeError("disk full")

    before, n_threads = sys.getswitchinterval(), threading.active_count()
    with pytest.raises(RuntimeError, match="disk full"):
        run_pipelined(ctx, range(1000), prepare, finish, 2, 2)
    # the producer was at most a full queue and the job in its hands ahead of the 3 jobs the consumer took
    assert len(prepared) <= 3 + 2 + 2
    assert sys.getswitchinterval() == before and threading.active_count() == n_threads
