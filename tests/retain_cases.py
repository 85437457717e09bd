"""Shared inputs and checks of the retainer's limited reads and host calls: used on the device
(tests/test_gpu_retain_pages.py) and, unchanged, on the CPU gate (tests/test_retain_dev_host.py,
the same store driven through tests/host_harness/retain_dev_main.cpp).  The shapes these inputs
promise are asserted on the reference alone by tests/test_retain_cases_cpu.py.

A `dev` below is anything with emqx_amd.Retainer's methods; `ref` is retain_ref.Retainer."""
import json
import os

import retain_ref as RR

DEFAULT = [[1, 2, 3], [1, 3], [2, 3], [3]]  # emqx_retainer_schema.erl:24-29
NOW = 100
RC_START, RC_BASE, RC_DELTA, RC_DONE, RC_STALE = range(5)

KS = (0, 1, 63, 64, 65, 129, 200)  # pK/# selects exactly K topics
# dead/t000 .. t199: positions of the sorted topics that are not live at NOW -- expired (expiry
# 50) or deleted after the base was built (a patched expiry word).  With them a page of 3 ends
# right before a dead position (2 | 3), a page of 63 before three (63 | 64 65 66), and the
# 64th live id (position 67) comes right after them.
N_DEAD = 200
DEAD_EXPIRED = (3, 64, 130)
DEAD_DELETED = (65, 66)
PD_BASE = 64  # pd/#: 64 base topics, then 4 live delta topics: a page of 64 ends on the boundary
LIMITS = (1, 2, 63, 64, 65, 128, 0)
BATCHES = (1, 255, 256, 257)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "retainer_backend_vectors.json")


def base_topics():
    """(topic, expiry) stored before the base is built."""
    out = []
    for k in KS:
        out += [(b"p%d/t%03d" % (k, i), 0) for i in range(k)]
    out += [(b"dead/t%03d" % i, 50 if i in DEAD_EXPIRED else 0) for i in range(N_DEAD)]
    out += [(b"pd/b%02d" % i, 0) for i in range(PD_BASE)]  # base part of pd/#
    out += [(b"q/%02d/x" % i, 0) for i in range(70)]       # q/+/x: 70 one-id runs
    out += [(b"q/%02d/x/deep" % i, 0) for i in range(0, 70, 7)]
    return out


def late_deletes():
    return [b"dead/t%03d" % i for i in DEAD_DELETED]


def delta_topics():
    """Stored after the base is built, with delta_max = 10**9: the delta store."""
    return [(b"pd/d%d" % i, 0) for i in range(4)] + [(b"q/%02d/y" % i, 0) for i in range(3)] + [
        (b"pd/dx", 50)]  # an expired delta topic


FILTERS = [b"#", b"nope/#", b"p200/#", b"zz/+", b"+/#", b"p0/#", b"p1/#", b"p63/#", b"p64/#",
           b"p65/#", b"p129/#", b"pd/#", b"q/+/x", b"p200/+", b"q/+/#", b"+/+", b"q/+/x/deep",
           b"p129/t100", b"+/t001", b"dead/#", b"dead/+"]
BIG = (b"#", b"+/#", b"+/+", b"p200/#", b"p200/+", b"p129/#", b"q/+/#", b"dead/#",
       b"dead/+")  # more than 70 ids


def build(dev, ref, specs):
    """The store of the page tests: base topics, a forced full build, then patches and a
    delta."""
    dev.set_index_specs(specs)
    dev.tune("timing", 1)  # the event code of the limited read runs too
    for t, e in base_topics():
        dev.store_retained(t, e)
        ref.store_retained(t, e)
    dev.tune("delta_max", 0)
    dev.commit()
    dev.tune("delta_max", 10**9)
    for t in late_deletes():
        dev.delete_message(t)
        ref.delete_message(t)
    for t, e in delta_topics():
        dev.store_retained(t, e)
        ref.store_retained(t, e)
    dev.commit()
    st = dev.stats()
    assert st["delta_topics"] == len(delta_topics()) and st["base_topics"] == len(base_topics()), st


def drain(dev, filters, limits, now=NOW, max_calls=5000):
    """Page every filter until DONE; -> (concatenated rows, pages per filter, ids in all)."""
    n = len(filters)
    cur = [None] * n
    rows = [[] for _ in range(n)]
    pages = [0] * n
    total = 0
    for _ in range(max_calls):
        got, cur = dev.match_pages_batch(filters, limits, cur, now)
        for k in range(n):
            lim = limits[k]
            assert lim == 0 or len(got[k]) <= lim, (filters[k], lim, len(got[k]))
            if got[k]:
                pages[k] += 1
            rows[k] += got[k]
            total += len(got[k])
            assert cur[k][1] in (RC_BASE, RC_DELTA, RC_DONE), cur[k]
            # not DONE: the page is full
            assert cur[k][1] == RC_DONE or (lim and len(got[k]) == lim), (filters[k], cur[k])
        if all(c[1] == RC_DONE for c in cur):
            # a DONE entry yields an empty row and stays DONE
            again, cur2 = dev.match_pages_batch(filters, limits, cur, now)
            assert all(r == [] for r in again) and cur2 == cur
            return rows, pages, total
    raise AssertionError("the cursors never finished")


def check_page_identity(dev, ref, filters, limits, now=NOW):
    """Pages concatenated until DONE == the unlimited row, order included; the set is the
    reference's; the ids over all pages are the unlimited n_ids."""
    full = dev.match_messages_batch(filters, now)
    rows, pages, total = drain(dev, filters, limits, now)
    for f, lim, want, got, np_ in zip(filters, limits, full, rows, pages):
        assert got == want, (f, lim, got[:5], want[:5])
        assert sorted(got, key=RR.wkey) == sorted(ref.match_messages(f, now), key=RR.wkey), f
        assert np_ == (-(-len(want) // lim) if lim else min(len(want), 1)), (f, lim, np_)
    assert total == sum(len(r) for r in full)


def mixed_batch(n):
    """n filters with different limits (and, after the first page, different cursor phases)."""
    fs = [FILTERS[k % len(FILTERS)] for k in range(n)]
    ls = [LIMITS[(k // len(FILTERS) + k) % len(LIMITS)] for k in range(n)]
    if n > 1:
        # the whole batch is read again for every page: the filters with hundreds of ids take
        # the limits from 63 up here (test_page_identity pages them by 1 and 2 in a small batch)
        ls = [LIMITS[2 + k % 5] if l in (1, 2) and f in BIG else l
              for k, (f, l) in enumerate(zip(fs, ls))]
    return fs, ls


def check_cursors_under_change(dev, ref):
    """With delta_max = 10**9 (dev built by build()): between the pages store new topics, delete
    and re-store base and delta topics, and commit.  While no full rebuild intervenes a topic
    selected and untouched from the first page to the last comes exactly once, none twice, and
    only topics that were selected at some page's time come at all.  Then a rebuild: STALE for
    the entries of the old generation alone."""
    f, lim = b"#", 50
    before = set(ref.match_messages(f, NOW))
    ever = set(before)
    touched = set()
    changes = [
        [("store", b"aa/new0"), ("store", b"zz/new1"), ("delete", b"p200/t150"),
         ("delete", b"pd/d1")],
        [("store", b"p200/t150"), ("store", b"pd/d1"), ("delete", b"p64/t010"),
         ("store", b"p63/t000")],
        [("delete", b"q/03/y"), ("store", b"pd/d00"), ("store", b"p64/t010"),
         ("delete", b"p129/t128")],
        [("store", b"q/03/y"), ("delete", b"zz/new1"), ("store", b"p129/zzz")],
    ]
    cur, seen, step = None, [], 0
    while True:
        rows, c = dev.match_pages_batch([f], [lim], [cur], NOW)
        seen += rows[0]
        cur = c[0]
        if cur[1] == RC_DONE:
            break
        assert cur[1] in (RC_BASE, RC_DELTA) and len(rows[0]) == lim
        if step < len(changes):
            for op, t in changes[step]:
                touched.add(t)
                if op == "store":
                    dev.store_retained(t)
                    ref.store_retained(t)
                else:
                    dev.delete_message(t)
                    ref.delete_message(t)
            dev.commit()
            ever |= set(ref.match_messages(f, NOW))
            step += 1
    assert step == len(changes)
    assert dev.stats()["full_builds"] == 2  # create + build(): no rebuild in between
    assert len(set(seen)) == len(seen), "a topic came twice"
    assert set(seen) <= ever
    untouched = (before & set(ref.match_messages(f, NOW))) - touched
    assert untouched <= set(seen) and len(untouched) > 800
    # a rebuild under two cursors; a third entry starts fresh in the same batch
    fs = [b"p200/#", b"pd/#", b"p65/#"]
    _, cur = dev.match_pages_batch(fs[:2], [10, 66], [None, None], NOW)
    assert [c[1] for c in cur] == [RC_BASE, RC_DELTA]
    dev.tune("delta_max", 0)
    dev.store_retained(b"rebuild/now")
    ref.store_retained(b"rebuild/now")
    dev.commit()
    dev.tune("delta_max", 10**9)
    rows, cur3 = dev.match_pages_batch(fs, [10, 66, 0], cur + [None], NOW)
    assert [c[1] for c in cur3] == [RC_STALE, RC_STALE, RC_DONE]
    assert rows[0] == [] and rows[1] == [] and len(rows[2]) == 65
    rows, cur4 = dev.match_pages_batch(fs[:1], [10], cur3[:1], NOW)
    assert rows == [[]] and cur4[0][1] == RC_STALE  # stays STALE until restarted
    # clean/1 invalidates too
    _, cur = dev.match_pages_batch(fs[:1], [10], [None], NOW)
    dev.clean()
    ref.clean()
    dev.commit()
    rows, cur = dev.match_pages_batch(fs[:1], [10], cur, NOW)
    assert rows == [[]] and cur[0][1] == RC_STALE


def forged_cursors(dev):
    """-> the cursors that must be refused (-EINVAL), for a dev built by build()."""
    st = dev.stats()
    gen = st["full_builds"]
    n_topics = len(base_topics()) + len(delta_topics())
    return [(gen, RC_BASE, st["base_topics"] + 1), (gen, RC_BASE, 0xFFFFFFFF),
            (gen, RC_DELTA, n_topics), (gen, RC_DELTA, 0xFFFFFFFF), (gen, 5, 0), (0, 77, 0)]


def check_forged(dev, raises):
    """`raises`: a context manager factory expecting the backend's -EINVAL error."""
    st = dev.stats()
    for c in forged_cursors(dev):
        with raises():
            dev.match_pages_batch([b"p1/#", b"#"], [1, 1], [None, c], NOW)
    # the valid edge: a BASE cursor at the base's size goes on with the delta store
    rows, cur = dev.match_pages_batch([b"pd/#"], [0], [(st["full_builds"], RC_BASE,
                                                        st["base_topics"])], NOW)
    assert rows == [[b"pd/d%d" % i for i in range(4)]] and cur[0][1] == RC_DONE


# ---- host calls ----
def check_clear_expired(dev, ref):
    now = 1000
    topics = [(b"e/before", now - 1), (b"e/at", now), (b"e/after", now + 1), (b"e/never", 0),
              (b"e/old", 1), (b"f/x", 0)]
    for t, e in topics:
        dev.store_retained(t, e)
        ref.store_retained(t, e)
    assert dev.size() == 6
    got = dev.clear_expired(now)
    assert sorted(got) == sorted(ref.clear_expired(now)) == [b"e/before", b"e/old"]
    assert dev.size() == ref.size() == 4
    for t, _ in topics:
        assert dev.read_message(t, now) == ref.read_message(t, now), t
    for f in (b"e/+", b"#", b"e/before", b"e/at"):
        for at in (0, now - 1, now, now + 1):
            assert sorted(dev.match_messages(f, at)) == sorted(ref.match_messages(f, at)), (f, at)
    assert dev.clear_expired(now) == []  # nothing left to clear
    dev.store_retained(b"e/before", 0)   # a cleared topic can be stored again
    ref.store_retained(b"e/before", 0)
    assert dev.size() == ref.size() == 5 and dev.read_message(b"e/before", now) == [b"e/before"]


def check_table_full(dev, ref, limit):
    dev.set_max_retained(limit)
    ref.max_retained = limit
    now = 1000

    def store(t, e=0):
        got = dev.store_retained(t, e) is not None
        assert got == ref.store_retained(t, e), (t, e, got)
        return got

    for i in range(limit):
        assert store(b"full/%d" % i, 10 if i == 0 else 0)  # full/0 is expired at `now`
    assert not store(b"full/new")
    assert store(b"full/%d" % (limit - 1), 7)   # a stored topic again: always
    assert store(b"full/0", 10)                 # an expired, uncleared one too (it counts)
    assert dev.size() == ref.size() == limit
    assert dev.read_message(b"full/new", now) == []
    assert sorted(dev.clear_expired(now)) == sorted(ref.clear_expired(now)) != []
    assert store(b"full/new")                   # room again
    dev.delete_message(b"full/new")
    ref.delete_message(b"full/new")
    k = 0
    while dev.size() < limit:
        assert store(b"full/fill%d" % k)
        k += 1
    assert k >= 1 and not store(b"full/new")
    dev.set_max_retained(0)
    ref.max_retained = 0
    assert store(b"full/new")
    assert sorted(dev.match_messages(b"full/+", now)) == sorted(ref.match_messages(b"full/+", now))


def check_page_read(dev, ref):
    now = 1000
    n = 23
    order = [(7 * i) % n for i in range(n)]  # distinct timestamps, not in topic order
    for i in range(n):
        t = b"pg/%02d" % i
        dev.store_retained(t, 0, order[i] + 1)
        ref.store_retained(t, 0, order[i] + 1)
    dev.store_retained(b"pg/expired", 5, 3)
    ref.store_retained(b"pg/expired", 5, 3)
    dev.store_retained(b"other/x/y", 0, 999)
    ref.store_retained(b"other/x/y", 0, 999)
    for limit in (1, 5, 23, 24):
        for page in range(1, n // limit + 3):
            assert dev.page_read(b"pg/+", page, limit, now) == ref.page_read(b"pg/+", page, limit, now), (page, limit)
    assert dev.page_read(b"pg/+", 6, 5, now) == []  # a page past the end
    # NULL filter: everything, '#' on the full scan
    assert dev.page_read(None, 1, 100, now) == ref.page_read(None, 1, 100, now)
    assert len(dev.page_read(None, 1, 100, now)) == n + 1
    assert dev.page_read(None, 3, 10, now) == ref.page_read(None, 3, 10, now) != []
    # ties: the timestamp sequence and the union over all pages
    ts = {}
    for i in range(17):
        t = b"tie/%02d" % i
        ts[t] = i % 3
        dev.store_retained(t, 0, i % 3)
        ref.store_retained(t, 0, i % 3)
    got, want = [], []
    for page in range(1, 6):
        got += dev.page_read(b"tie/+", page, 4, now)
        want += ref.page_read(b"tie/+", page, 4, now)
    assert [ts[t] for t in got] == [ts[t] for t in want] == sorted(ts.values())
    assert sorted(got) == sorted(want) == sorted(ts)


def check_page_read_invalid(dev, raises):
    for page, limit in ((0, 5), (1, 0), (0, 0)):
        with raises():
            dev.page_read(b"pg/+", page, limit, 1)


def check_delete_matching(dev, ref, specs):
    dev.set_index_specs(specs)
    topics = [b"a", b"a/x", b"a/x/y", b"a/x/y/z", b"b/x", b"b/x/y", b"x/b/c", b"a/+x", b""]
    for i, t in enumerate(topics):
        dev.store_retained(t, 5 if i % 3 == 0 else 0)  # Now = 0: expired ones go too
        ref.store_retained(t, 5 if i % 3 == 0 else 0)
    for f in (b"a/+", b"nope/#", b"+/x", b"b/x", b"a/#/c", b"#"):
        dev.delete_message(f)
        ref.delete_message(f)
        assert dev.size() == ref.size(), f
        assert sorted(dev.match_messages(b"#", 0)) == sorted(ref.match_messages(b"#", 0)), f
        for t in topics:
            assert dev.read_message(t, 0) == ref.read_message(t, 0), (f, t)


def golden():
    return json.load(open(GOLDEN))["cases"]


def run_golden(dev, case):
    """One case of tests/golden/retainer_backend_vectors.json on a fresh store."""
    dev.set_max_retained(case["max_retained_messages"])
    for st in case["steps"]:
        op = st[0]
        if op == "store":
            assert (dev.store_retained(st[1].encode(), st[2], st[3]) is not None) == st[4], st
        elif op == "delete":
            dev.delete_message(st[1].encode())
        elif op == "match":
            assert len(dev.match_messages(st[1].encode(), st[2])) == st[3], st
        elif op == "page":
            assert len(dev.page_read(st[1].encode(), st[2], st[3], st[4])) == st[5], st
        elif op == "clear":
            assert len(dev.clear_expired(st[1])) == st[2], st
        elif op == "size":
            assert dev.size() == st[1], st
        elif op == "cursor":
            _, f, batch, now, per_read, total = st
            cur, reads = None, []
            while True:
                rows, cur = dev.match_messages_cursor(f.encode(), cur, batch, now)
                reads.append(len(rows))
                if cur is None:
                    break
            assert [r for r in reads if r] == per_read and sum(reads) == total, (st, reads)
        else:
            raise AssertionError(op)
