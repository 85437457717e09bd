"""The shapes tests/retain_cases.py promises to the limited-read tests, asserted on the
reference alone (tests/retain_ref.py; no GPU, no harness): the prefix sizes, where the limits
cut -- inside a run, on a run's last id, on a 64-position boundary of a clipped run, on the
base-to-delta boundary, next to deleted and expired positions -- and the suite vectors."""
import pytest

import retain_cases as RC
import retain_ref as RR


class RefDev:
    """retain_ref.Retainer behind emqx_amd.Retainer's method names (no device state)."""

    def __init__(self, specs):
        self.ref = RR.Retainer(specs)

    def set_max_retained(self, limit):
        self.ref.max_retained = limit

    def store_retained(self, topic, expiry_ms=0, ts_ms=0):
        return 0 if self.ref.store_retained(topic, expiry_ms, ts_ms) else None

    def delete_message(self, topic):
        self.ref.delete_message(topic)

    def match_messages(self, topic, now):
        return self.ref.match_messages(topic, now)

    def page_read(self, topic, page, limit, now):
        return self.ref.page_read(topic, page, limit, now)

    def clear_expired(self, now):
        return self.ref.clear_expired(now)

    def size(self):
        return self.ref.size()

    def match_messages_cursor(self, topic, cursor, batch, now):
        return self.ref.match_messages_cursor(topic, now, cursor, batch)


@pytest.fixture(scope="module")
def store():
    """The reference after build()'s steps, and the stores' sorted positions: base (every
    topic of the build, dead ones too) and delta."""
    ref = RR.Retainer([])
    for t, e in RC.base_topics():
        ref.store_retained(t, e)
    for t in RC.late_deletes():
        ref.delete_message(t)
    for t, e in RC.delta_topics():
        ref.store_retained(t, e)
    base = sorted((t for t, _ in RC.base_topics()), key=RR.wkey)
    delta = sorted((t for t, _ in RC.delta_topics()), key=RR.wkey)
    return ref, base, delta


def _live(ref, t):
    return ref.match_messages(t, RC.NOW) == [t]


def test_topics_are_distinct_and_prefix_sizes(store):
    ref, base, delta = store
    assert len(set(base)) == len(base) and not set(base) & set(delta)
    for k in RC.KS:
        assert len(ref.match_messages(b"p%d/#" % k, RC.NOW)) == k
        assert len(ref.match_messages(b"p%d/+" % k, RC.NOW)) == k
    assert set(RC.LIMITS) == {1, 2, 63, 64, 65, 128, 0} and RC.BATCHES == (1, 255, 256, 257)


def test_dead_positions_next_to_cuts(store):
    ref, base, _ = store
    run = [t for t in base if t.startswith(b"dead/")]
    assert len(run) == RC.N_DEAD
    live = [_live(ref, t) for t in run]
    dead = sorted(RC.DEAD_EXPIRED + RC.DEAD_DELETED)
    assert [i for i, l in enumerate(live) if not l] == dead
    pos = [i for i, l in enumerate(live) if l]  # position of each live rank
    # limit 2 cuts inside the run; limit 1 and 2 end a page on position 2, right before dead 3
    assert pos[1] == 1 and pos[2] == 2 and not live[3]
    # limit 63: the page's last id is position 63, right before three dead positions
    assert pos[62] == 63 and not any(live[64:67])
    # limit 64: the page's last id (position 67) comes right after them
    assert pos[63] == 67
    # limits 63, 64, 65: the second page (ranks up from 63 .. 65) reads across dead 130
    assert pos[125] == 129 and pos[126] == 131


def test_run_shapes(store):
    ref, base, delta = store
    # p200/#: one run of 200 live positions -- with limit 64 the second page is a clipped run
    # that ends on its first 64-position boundary (64 .. 127), the last is a partial chunk
    assert ref.match_messages(b"p200/#", RC.NOW).__len__() == 200 and 200 % 64 == 8
    # q/+/x, dead/+: one-id runs -- every limit ends on a run's last id
    assert len(ref.match_messages(b"q/+/x", RC.NOW)) == 70
    assert len(ref.match_messages(b"dead/+", RC.NOW)) == 195
    # +/#: runs of many sizes in one filter; limits cut inside them
    firsts = sorted({t.split(b"/")[0] for t in base})
    sizes = [sum(_live(ref, t) for t in base if t.split(b"/")[0] == w) for w in firsts]
    assert firsts[:3] == [b"dead", b"p1", b"p129"] and sizes[:3] == [195, 1, 129]
    # pd/#: the base part is 64 ids, then the delta's 4 live ones (pd/dx is expired)
    pd_base = [t for t in base if t.startswith(b"pd/")]
    pd_delta = [t for t in delta if t.startswith(b"pd/") and _live(ref, t)]
    assert len(pd_base) == RC.PD_BASE == 64 and len(pd_delta) == 4
    assert len(ref.match_messages(b"pd/#", RC.NOW)) == 68
    # filters that select nothing stand between filters that select many
    n = [len(ref.match_messages(f, RC.NOW)) for f in RC.FILTERS[:6]]
    assert n[0] > 800 and n[1] == 0 and n[2] == 200 and n[3] == 0 and n[4] > 800 and n[5] == 0


def test_mixed_batches_mix_limits():
    for n in RC.BATCHES:
        fs, ls = RC.mixed_batch(n)
        assert len(fs) == len(ls) == n
        if n > 1:
            assert set(ls) == set(RC.LIMITS)
            assert all(l not in (1, 2) for f, l in zip(fs, ls) if f in RC.BIG)


def test_cursor_reads_deliver_the_same_rows(store):
    """{Cursor, BatchNum} (:185-202): the reads concatenated are the unlimited answer; when
    exactly N answers remain qlc_next_answers/2 needs one more, empty, read to close."""
    ref = store[0]
    for f, batch in ((b"pd/#", 3), (b"pd/#", 4), (b"p64/#", 64), (b"nope/#", 5)):
        want = ref.match_messages(f, RC.NOW)
        rows, cur, reads = [], None, 0
        while True:
            got, cur = ref.match_messages_cursor(f, RC.NOW, cur, batch)
            rows += got
            reads += 1
            if cur is None:
                break
        assert rows == want
        assert reads == len(want) // batch + 1  # (an empty last read when batch divides)


@pytest.mark.parametrize("name", sorted(RC.golden()))
def test_suite_vectors_on_the_reference(name):
    RC.run_golden(RefDev(RC.DEFAULT), RC.golden()[name])


def test_host_checks_on_the_reference_pair():
    """The reference against itself through the checks' own reads: they are well-formed."""
    for limit in (1, 3):
        ref = RR.Retainer(RC.DEFAULT)

        class Dev(RefDev):
            def __init__(self):
                self.ref = RR.Retainer(RC.DEFAULT)

            def read_message(self, t, now):
                return self.ref.read_message(t, now)

        RC.check_table_full(Dev(), ref, limit)
