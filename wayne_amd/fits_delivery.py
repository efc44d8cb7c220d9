"""Delivery of an exposure's FITS words: raw files written straight from pinned memory.

With `device_fits` the device forms the data sections of an exposure's NNNN_raw.fits (k_fits_words: big-endian words in
file order, each with its padding) and they are copied into a pinned mirror of the slot.  A writer thread then hands
os.writev the header blocks it renders and views of that mirror: no numpy pass over the samples, no copy out of the
pinned buffer.  What it costs is that the mirror belongs to the file until the file is out -- the LEASE of a slot:

    FitsDelivery.wait(slot)      hands `finish` the payload view and notes the slot
    FitsDelivery.lease()         marks that slot's mirror as in use by a file; returns the `done` callback of
                                 FitsWriterPool.submit, which releases it (file out, or write failed)
    FitsDelivery.upload(slot)    blocks until the slot's lease has been released

so pipeline.run_pipelined needs no change and no buffer is overwritten under a writer: the loop simply runs over more
slots than it has exposures in flight (slots_for).
"""
import threading


class FitsDelivery(object):
    """What pipeline.run_pipelined sees of a context when an exposure's FITS words are delivered: fetch_async / wait are
    the FITS calls, and wait hands `finish` the payload -- a uint8 view of the slot's pinned mirror, (R + 1) * stride bytes.
    `extraction`: an extraction.Delivery over the same context -- the spectra (and, with its `reads`, the reads) are then
    delivered beside the payload and wait returns (payload, spectra, sky).  `reads`: without an extraction, fetch the
    reads too.  Either way `self.reads_view` is the reads' view of the last wait (None: not fetched) and `self.layout`
    its (plane_bytes, stride, bitpix)."""

    def __init__(self, ctx, extraction=None, reads=False):
        self.ctx, self.extraction = ctx, extraction
        self.reads = bool(reads) and extraction is None
        self.reads_view = None
        self.layout = None
        self._cv = threading.Condition()
        self._leased = set()          # slots whose pinned mirror a file is being written from
        self._last = None             # slot of the last wait

    # -- the lease ------------------------------------------------------------
    def lease(self):
        """The slot of the last wait is in use by a file from now on -> the callback that releases it (call it exactly
        when the file is out or has failed: FitsWriterPool.submit(..., done=...))."""
        slot = self._last
        with self._cv:
            self._leased.add(slot)
        return lambda: self.release(slot)

    def release(self, slot):
        with self._cv:
            self._leased.discard(slot)
            self._cv.notify_all()

    def leased(self, slot):
        with self._cv:
            return slot in self._leased

    # -- what run_pipelined calls ------------------------------------------------
    def upload(self, slot, desc):
        with self._cv:
            while slot in self._leased:      # the file written from this slot's mirror is not out yet
                self._cv.wait()
        self.ctx.upload(slot, desc)

    def run(self, slot):
        self.ctx.run(slot)

    def fetch_async(self, slot):
        if self.reads:
            self.ctx.fetch_async(slot)
        if self.extraction is not None:
            self.extraction.fetch_async(slot)      # (its reads, if any, in front of the payload; then the spectra)
        self.ctx.fetch_fits_async(slot)

    def wait(self, slot):
        # the payload first: a second run (a bin beyond the lanes' reach) then fetches everything beside it again
        payload = self.ctx.wait_fits(slot)
        self._last = slot
        self.layout = self.ctx.fits_layout_of(slot)
        self.reads_view = self.ctx.wait(slot) if self.reads else None
        if self.extraction is None:
            return payload
        reads, spectra, sky = self.extraction.wait(slot)
        self.reads_view = reads
        return payload, spectra, sky

    def __getattr__(self, name):
        # rejected / channels / variances / optimal / ... of the last wait: the extraction's
        extraction = self.__dict__.get("extraction")
        if extraction is not None and not name.startswith("_"):
            return getattr(extraction, name)
        raise AttributeError(name)


def slots_for(depth, writers, limit=32):
    """Context slots of a device_fits loop with `depth` exposures in flight and `writers` writer threads: one per exposure
    in flight plus one per file that can be under a writer at a time -- with fewer the loop waits in upload for a file
    although a writer is idle; more would only queue finished payloads in pinned memory -- rounded up to an even number
    (neighbouring slots keep alternating streams) and capped at `limit` (a full-array float32 slot holds 134 MB of
    pinned memory and as much of HBM for its payload)."""
    n = int(depth) + max(1, int(writers))
    n += n & 1
    return max(2, min(n, limit - (limit & 1)))


def stored_pieces(payload, layout, n_reads):
    """The payload as the file's pieces: [memoryview of plane f, f = 0 .. n_reads - 1] -- plane f is the data section and
    padding of the SCI image of read n_reads - 1 - f."""
    stride = layout[1]
    mv = memoryview(payload).cast("B")        # (a view: nothing is copied)
    if len(mv) != n_reads * stride:
        raise ValueError("payload of %d bytes for %d reads of stride %d" % (len(mv), n_reads, stride))
    return [mv[f * stride:(f + 1) * stride] for f in range(n_reads)]
