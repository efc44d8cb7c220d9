"""The exposure loop of a visit, shared by Observation.run_observation and VisitRunner.run.

Two host threads.  A producer runs the host half of every exposure (sample times, orbit phases, the Philox host draws,
the descriptor -- no GPU call, no context state); the calling thread uploads, launches and finishes.  The C calls on
both sides release the interpreter lock (ctypes), so a descriptor's host draws and an upload's table building overlap
the other thread's Python: a visit is then paced by the device, not by the host.
"""
import collections
import queue
import sys
import threading


def run_pipelined(ctx, jobs, prepare, finish, depth, n_slots):
    """For every job: `prepare(job) -> (desc, state)` on the producer thread; on this one the descriptor is uploaded
    into context slot n % n_slots (n counts the jobs: neighbouring slots run on different HIP streams), its kernels and
    the copy of its reads to pinned host memory are enqueued, and -- oldest first, whenever `depth` jobs are in flight,
    and at the end -- `finish(job, state, reads)` gets what ctx.wait(slot) returned: a VIEW of the slot's pinned
    buffer, which the job `n_slots` later overwrites (copy it to keep it).  An exception of `prepare` is raised here."""
    ahead = queue.Queue(maxsize=n_slots)
    stop = threading.Event()            # set by this thread when it leaves the loop, for whatever reason

    def put(item):
        """Queue.put that gives up when the consumer has gone (returns False)."""
        while not stop.is_set():
            try:
                ahead.put(item, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def produce():
        try:
            for job in jobs:
                if stop.is_set() or not put((job,) + tuple(prepare(job))):
                    return
        except BaseException as e:      # surfaced in the consuming thread
            put(e)
            return
        put(None)

    in_flight = collections.deque()     # (job, state, slot), oldest first

    def finish_oldest():
        job, state, slot = in_flight.popleft()
        finish(job, state, ctx.wait(slot))

    producer = threading.Thread(target=produce, daemon=True)
    old_interval = sys.getswitchinterval()
    sys.setswitchinterval(min(old_interval, 2e-4))   # hand the lock over promptly between the two
    producer.start()
    try:
        n = 0
        while True:
            item = ahead.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            job, desc, state = item
            slot = n % n_slots
            if len(in_flight) >= depth:     # (with depth == n_slots: the slot about to be reused is drained first)
                finish_oldest()
            ctx.upload(slot, desc)
            ctx.run(slot)                   # asynchronous on the slot's stream
            ctx.fetch_async(slot)           # ... followed by its copy to pinned host memory
            in_flight.append((job, state, slot))
            n += 1
        while in_flight:
            finish_oldest()
    finally:
        stop.set()                  # an error or Ctrl-C on this side: the producer stops after the descriptor it is
        producer.join()             # building, not after the rest of the visit's host work
        sys.setswitchinterval(old_interval)
