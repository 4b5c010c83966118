"""The order of the row pipeline of picaso_amd/opacity_factory.py (``_UploadRing.run``), on the host: the device blocks,
the asynchronous copy, the stream-to-stream wait and the synchronise are replaced by recorders.  What makes the two slots
safe is an order of events -- a slot is staged again only after the wait that follows the consumer that read it -- and that
order, the one-ahead reading of rows, the teardown and the row-length message are asserted here."""
import numpy as np
import pytest

from picaso_amd import opacity_factory as of

CTX, AUX = "ctx", "aux"


class Recorder:
    """The events of one run, in order, and the stand-ins that write them."""

    def __init__(self, monkeypatch):
        self.events = events = []
        addrs = iter(range(1000, 2000))

        class Block:
            def __init__(self, shape, ctx=None):
                self.shape, self.addr = tuple(np.atleast_1d(shape)), next(addrs)
                self.array = np.empty(self.shape)

            def free(self):
                events.append(("free", self.addr))

        class Lib:
            @staticmethod
            def picaso_memcpy_h2d_async(ctx, dst, src, nbytes):
                assert ctx == AUX
                events.append(("stage", dst))
                return 0

        monkeypatch.setattr(of, "DeviceArray", Block)
        monkeypatch.setattr(of, "PinnedArray", Block)
        monkeypatch.setattr(of, "_sync", lambda ctx: events.append(("wait", ctx)))
        monkeypatch.setattr(of._lib, "ctx_wait", lambda waiter, signaller: events.append(("landed", waiter, signaller)))
        monkeypatch.setattr(of._lib, "load", lambda: Lib)

    def rows(self, n, length=7, fail_at=None):
        events = self.events

        class Rows:
            def __len__(self):
                return n

            def __getitem__(self, i):
                events.append(("load", i))
                if i == fail_at:
                    raise OSError("row %d cannot be read" % i)
                return np.full(length, float(i))

        return Rows()

    def run(self, n, expect=7, fail_at=None, consumer_fails_at=None):
        rows = self.rows(n, fail_at=fail_at)

        def consume(row, d_row, n_row):
            self.events.append(("consume", row.index, d_row.addr))
            assert n_row == 7
            if row.index == consumer_fails_at:
                raise RuntimeError("the consumer fails on row %d" % row.index)

        of._UploadRing(CTX, AUX, "who").run((of._Row("row %d" % i, rows, i, expect) for i in range(n)), consume)

    def names(self):
        return [e[0] if e[0] != "wait" else "wait " + e[1] for e in self.events if e[0] != "load"]


def check_teardown(events):
    """both slots (two pinned blocks, two device buffers) are freed, and every free follows a wait for both streams that
    itself follows everything else"""
    frees = [k for k, e in enumerate(events) if e[0] == "free"]
    assert len(frees) == 4 and len({events[k][1] for k in frees}) == 4
    assert frees == list(range(len(events) - 4, len(events)))
    assert events[frees[0] - 2:frees[0]] == [("wait", CTX), ("wait", AUX)]


def test_three_rows_run_in_the_order_that_keeps_both_slots_safe(monkeypatch):
    rec = Recorder(monkeypatch)
    rec.run(3)
    ev = rec.events
    assert rec.names() == ["stage", "landed", "stage", "consume", "wait ctx", "landed", "stage", "consume", "wait ctx",
                           "landed", "consume", "wait ctx", "wait aux", "free", "free", "free", "free"]
    assert all(e == ("landed", CTX, AUX) for e in ev if e[0] == "landed")
    stages = [e[1] for e in ev if e[0] == "stage"]
    consumes = [e for e in ev if e[0] == "consume"]
    assert [c[1] for c in consumes] == [0, 1, 2]
    assert [c[2] for c in consumes] == stages and stages[0] == stages[2] != stages[1]        # slot k & 1
    # a slot is never staged between the consume that reads it and the following wait
    for k, e in enumerate(ev):
        if e[0] == "consume":
            until = next(j for j in range(k, len(ev)) if ev[j] == ("wait", CTX))
            assert ("stage", e[2]) not in ev[k:until]
    # rows are read one ahead, never further: row k + 2 is asked for after row k is consumed
    for i in range(3):
        assert ev.count(("load", i)) == 1
    assert ev.index(("load", 2)) > ev.index(consumes[0]) and ev.index(("load", 1)) < ev.index(consumes[0])
    check_teardown(ev)


def test_a_failing_consumer_or_loader_still_waits_then_frees_both_slots(monkeypatch):
    rec = Recorder(monkeypatch)
    with pytest.raises(RuntimeError, match="the consumer fails on row 1"):
        rec.run(3, consumer_fails_at=1)
    assert rec.names()[:8] == ["stage", "landed", "stage", "consume", "wait ctx", "landed", "stage", "consume"]
    check_teardown(rec.events)
    rec = Recorder(monkeypatch)
    with pytest.raises(OSError, match="row 2 cannot be read"):
        rec.run(3, fail_at=2)
    assert rec.names()[:6] == ["stage", "landed", "stage", "consume", "wait ctx", "landed"]
    assert [e[1] for e in rec.events if e[0] == "consume"] == [0]
    check_teardown(rec.events)


def test_a_row_of_another_length_than_its_grid_says_is_named(monkeypatch):
    rec = Recorder(monkeypatch)
    with pytest.raises(Exception, match="who: row 0 has 7 points, its wavenumber grid 9"):
        rec.run(2, expect=9)
    assert not [e for e in rec.events if e[0] == "consume"]
    check_teardown(rec.events)
