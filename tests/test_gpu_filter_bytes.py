"""The filter-byte gather on the device (emqxgm_match_batch_submit_filters / _wait_filters:
k_filter_len, k_filter_gather, k_fb_pack, k_fb_small, copy_filter and the device-counted length
scan in emqx_amd/csrc/gm_kernels.hip; host_pipe_enqueue_gather, host_pipe_gather and
host_pipe_complete in gm_engine.cpp), exactly equal to the reference of tests/fb_cases.py over
its edge filters and window plans, on every packing path: the synchronous gather, the enqueued
gather with pageable input (the block goes by DMA) and with input in pinned memory (the block is
written straight into pinned memory), on k_fb_small and on k_fb_pack, and with host_out 1.

What is compared, for every window: the row pointers, each row's filter ids (sorted) and the
exact ids against oracle.emqx_ref over the filters and route keys this test inserted; then the
byte offsets and every byte against this test's own id -> bytes table, for the pairs in the order
the device returned them.  No expected byte comes from a device result.

Which path a window took is read from stats()["sync_gathers"] (it rises by one when the block was
too small and the wait gathered synchronously).  The per-pipe estimates are decaying maxima and
the pipes rotate by ticket, so every case that depends on a pipe's history uses a fresh Engine,
whose first HOST_PIPES windows each meet a pipe without history.

No zero-length filter: the oracle never returns one (fb_cases docstring)."""
import ctypes

import numpy as np
import pytest

import fb_cases as F

pytestmark = pytest.mark.gpu

RECENTRE = ("the fresh-pipe sizing of host_pipe_enqueue_gather (gm_engine.cpp) no longer is "
            "fb_cases.fresh_caps: restate it there, which re-centres the sweeps and the "
            "fresh-pipe windows")


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


@pytest.fixture(scope="module")
def ref():
    """{filter: id}, {route key: id} as the engines will number them (a filter's id is its
    position, a new route key takes the next id), and the expected result of every plan: all of
    it worked out on the oracle before the first device call."""
    fid = {f: i for i, f in enumerate(F.all_filters())}
    keys, nxt = {}, len(fid)
    for k in F.route_keys():
        keys[k] = fid[k] if k in fid else nxt
        nxt += k not in fid
    tab = F.table(fid)
    exp = {}
    for name, (topics, pairs) in F.plans().items():
        e = F.expected(topics, fid, keys)
        assert int(e[0][-1]) == len(e[1]) == pairs, name
        for a in e:
            a.setflags(write=False)
        exp[name] = e
    return fid, keys, tab, exp


def _new_engine(emqx, ref, rot=0):
    """An engine with all_filters() and route_keys() committed (rot: edge_set(rot) alone); the
    ids are the ones `ref` was computed for, read back with lookup_id."""
    eng = emqx.Engine()
    fs = list(F.all_filters()) if rot == 0 else [f for f, _ in F.edge_set(rot)]
    fb, fo = F.pack(fs, np.uint64)
    assert np.array_equal(eng.trie_insert_many(fb, fo), np.arange(len(fs)))
    if rot == 0:
        fid, keys = ref[0], ref[1]
        assert {k: eng.route_ref(k) for k in F.route_keys()} == keys
        assert all(eng.lookup_id(f) == i for f, i in fid.items())
        assert all(eng.lookup_id(k) == i for k, i in keys.items())
    eng.commit()
    return eng


@pytest.fixture(scope="module")
def engine(emqx, ref):
    eng = _new_engine(emqx, ref)
    yield eng
    eng.close()


def _mapped(a) -> bool:
    """Whether the runtime gives the host array a device address (pinned, mapped memory)."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipHostGetDevicePointer.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                            ctypes.c_uint]
    d = ctypes.c_void_p()
    return hip.hipHostGetDevicePointer(ctypes.byref(d), a.ctypes.data, 0) == 0 and bool(d.value)


def _input(eng, topics, pinned):
    tb, to = F.pack(list(topics))
    if not pinned:
        return tb, to
    hb, ho = eng.pinned(len(tb)), eng.pinned(len(to), np.uint32)
    hb[:], ho[:] = tb, to
    if len(topics):
        # the engine's own conditions for reading a window in place and writing its block into
        # pinned memory (batch_submit): both buffers have a device address, the bytes are 16-byte
        # aligned, the window is small
        assert _mapped(hb) and _mapped(ho) and hb.ctypes.data % 16 == 0
        assert len(topics) <= 65536 and int(to[-1]) <= 8 << 20
    return hb, ho


def _run(eng, topics, how, pinned=False):
    """One window; how = "sync" (submit, then the gather in the wait) or "enqueued".  Returns
    (result, foff, bytes, rise of sync_gathers)."""
    buf, off = _input(eng, topics, pinned)
    before = eng.stats()["sync_gathers"]
    t = eng.match_batch_submit(buf, off, filters=how == "enqueued")
    res, foff, fbytes = eng.match_batch_wait_filters(t)
    return res, foff, fbytes, eng.stats()["sync_gathers"] - before


def _rows_sorted(row_ptr, ids):
    seg = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr.astype(np.int64)))
    return ids[np.lexsort((ids, seg))]


def _check(what, topics, got, exp, tab):
    res, foff, fbytes, _ = got
    row, ids, exact, _, _ = exp
    assert np.array_equal(res.row_ptr.astype(np.uint64), row), (what, "row pointers")
    got_ids = _rows_sorted(row, res.filter_id)
    for j in np.flatnonzero(got_ids != ids)[:1]:
        i = int(np.searchsorted(row, j, side="right")) - 1
        raise AssertionError((what, "filter ids of topic", i, topics[i][:60], int(got_ids[j]), int(ids[j])))
    for i in np.flatnonzero(res.exact_id != exact)[:1]:
        raise AssertionError((what, "exact id of topic", int(i), topics[i][:60],
                              int(res.exact_id[i]), int(exact[i])))
    # the bytes of the pairs as the device ordered them, from the test's own table
    want_off, want_bytes = F.pair_bytes(res.filter_id, *tab)
    assert foff[0] == 0 and len(foff) == len(ids) + 1 and int(foff[-1]) == len(fbytes), what
    for j in np.flatnonzero(foff.astype(np.int64) != want_off)[:1]:
        raise AssertionError((what, "byte offset of pair", int(j), int(foff[j]), int(want_off[j])))
    for b in np.flatnonzero(fbytes != want_bytes)[:1]:
        j = int(np.searchsorted(want_off, b, side="right")) - 1
        f = int(res.filter_id[j])
        raise AssertionError((what, "byte", int(b) - int(want_off[j]), "of pair", j, "filter", f,
                              "of", int(want_off[j + 1] - want_off[j]), "bytes: got",
                              int(fbytes[b]), "want", int(want_bytes[b])))
    # (the canonical order's total is the same: every pair's bytes are there)
    assert len(fbytes) == len(exp[4]), what


def _enqueued_until_block(what, eng, topics, exp, tab, pinned):
    """The window enqueued until its block held it: the first window on a pipe that expects
    less falls back to the synchronous gather and raises the pipe's estimates; the same window
    on that pipe again (HOST_PIPES windows later) then fits.  Every run is checked.  Returns the
    rises of sync_gathers."""
    rises = []
    for k in range(eng.HOST_PIPES + 1):
        got = _run(eng, topics, "enqueued", pinned)
        _check((what, "run", k, "rise", got[3]), topics, got, exp, tab)
        assert got[3] in (0, 1), (what, got[3])
        rises.append(got[3])
        if got[3] == 0:
            break
    assert rises[-1] == 0, (what, rises, "the window never travelled in its block")
    return rises


def test_alignment_coverage(emqx, engine, ref):
    """Every length class lies at all four pool offsets mod 4: from the pointers
    emqxgm_filter_bytes returns, relative to filter 0's (offset 0; the device pool mirrors the
    host pool).  The one-byte class has three members ('#', '+', '$'); its fourth residue comes
    from edge_set(1), committed alone and run through the gather here."""
    def residues(eng, rot):
        lib, out = eng._lib, {}
        p, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint32()

        def at(i):
            assert lib.emqxgm_filter_bytes(eng._h, i, ctypes.byref(p), ctypes.byref(n)) == 0
            return ctypes.cast(p, ctypes.c_void_p).value, n.value
        base = at(0)[0]
        for i, (f, info) in enumerate(F.edge_set(rot)):
            a, ln = at(i)
            assert ctypes.string_at(a, ln) == f
            if info:
                assert (a - base) % 4 == info[2], (f[:20], a - base, info)
                out.setdefault(info[0], set()).add((a - base) % 4)
        return out
    seen = residues(engine, 0)
    eng1 = _new_engine(emqx, ref, rot=1)
    for L, rs in residues(eng1, 1).items():
        seen[L] |= rs
    assert set(seen) == set(F.LENS)
    assert all(rs == {0, 1, 2, 3} for rs in seen.values()), seen
    # the rotated set through the gather: every filter at another residue than in `engine`
    fid1 = {f: i for i, (f, _) in enumerate(F.edge_set(1))}
    topics = F.edge_topics()
    exp = F.expected(topics, fid1, rot=1)
    assert len(exp[1]) == F.plans()["lengths"][1]
    tab1 = F.table(fid1)
    got = _run(eng1, topics, "sync")
    _check("rot1 sync", topics, got, exp, tab1)
    assert got[3] == 0
    for pinned in (False, True):
        _enqueued_until_block(("rot1", pinned), eng1, topics, exp, tab1, pinned)
    eng1.close()


@pytest.mark.parametrize("plan", list(F.plans()))
def test_sync_gather_vs_reference(engine, ref, plan):
    """submit(filters=False) then wait_filters: k_filter_len, launch_scan over 0 / 1 / 2 / 3
    tiles with vector and ragged ends, k_filter_gather."""
    topics = F.plans()[plan][0]
    got = _run(engine, topics, "sync")
    _check((plan, "sync"), topics, got, ref[3][plan], ref[2])
    assert got[3] == 0  # nothing was enqueued: nothing fell back


# small and sparse windows first: a pipe's estimates only decay by a tenth per window, and a
# large window sized by a dense one's pairs per topic would ask for a block of gigabytes
ORDER = ("empty", "sparse-big", "sparse-small", "p0", "p1", "p15", "p16", "p17", "lengths",
         "p4095", "p4096", "p4097", "p8193", "small-4096", "small-4097", "pack-4097", "dense")


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "zero-copy"])
def test_enqueued_gather_vs_reference(emqx, ref, pinned):
    """Every plan through submit_filters on a fresh engine, each until it travelled in its block;
    both outcomes (block, fallback to the synchronous gather) must have occurred."""
    assert sorted(ORDER) == sorted(F.plans())
    eng = _new_engine(emqx, ref)
    eng.tune("zc_topics", 65536)
    seen = set()
    for plan in ORDER:
        topics = F.plans()[plan][0]
        seen |= set(_enqueued_until_block((plan, pinned), eng, topics, ref[3][plan], ref[2], pinned))
    assert seen == {0, 1}, seen
    eng.close()


def _fresh_windows(emqx, ref, windows, pinned):
    """Each window enqueued on a pipe without history: a new engine every HOST_PIPES windows.
    Yields (name, rise of sync_gathers) after checking the result.

    A pass that is redone (a walk lane's item stack outgrew the variant an index starts with;
    the next variant is then kept for the committed index) is finished in the wait as well,
    whatever its block held.  So each pipe first carries one window of the most branching topics
    through submit / wait without the gather, which settles the variant and leaves the pipe's
    estimates untouched (host_pipe_complete updates them for a gather only), and no measured
    window may count a rerun."""
    eng = None
    for k, (name, topics, exp) in enumerate(windows):
        if k % emqx.Engine.HOST_PIPES == 0:
            if eng:
                eng.close()
            eng = _new_engine(emqx, ref)
            wb, wo = F.pack([F.m_topic(9), F.k_topic(len(F.K_SWEEP) - 1)])
            for _ in range(eng.HOST_PIPES):
                warm = eng.match_batch_wait(eng.match_batch_submit(wb, wo))
                assert len(warm.filter_id) == 511 + F.K_SWEEP[-1]
        reruns = eng.stats()["reruns"]
        got = _run(eng, topics, "enqueued", pinned)
        _check((name, "fresh pipe", pinned, "rise", got[3]), topics, got, exp, ref[2])
        assert eng.stats()["reruns"] == reruns, (name, "the pass was redone: not a sizing outcome")
        yield name, got[3]
    if eng:
        eng.close()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "zero-copy"])
def test_fresh_pipe_takes_both_kernels(emqx, ref, pinned):
    """On a pipe without history the block has room for fresh_caps(n): windows of up to 800
    topics go to k_fb_small (small-4096 fills its FB_SMALL_PAIRS exactly, small-4097 is one pair
    beyond it), larger ones to launch_filter_len_dev + k_fb_pack (pack-4097: two scan tiles
    counted on the device; sparse-big: more topics than pairs and than a tile)."""
    names = ("small-4096", "sparse-big", "small-4097", "sparse-small", "pack-4097", "lengths")
    plans = F.plans()
    want = {}
    for nm in names:
        cap_p, cap_b = F.fresh_caps(len(plans[nm][0]))
        want[nm] = int(plans[nm][1] > cap_p or F.bytes_of(plans[nm][0]) > cap_b)
    assert want == {"small-4096": 0, "sparse-big": 0, "small-4097": 1, "sparse-small": 0,
                    "pack-4097": 0, "lengths": 1}
    got = dict(_fresh_windows(emqx, ref, [(nm, plans[nm][0], ref[3][nm]) for nm in names], pinned))
    assert got == want, (got, RECENTRE)


def _one_switch(rises, sweep, cap):
    assert rises[0] == 0 and rises[-1] == 1, (rises, RECENTRE)
    assert sum(a != b for a, b in zip(rises, rises[1:])) == 1, (rises, "more than one switch")
    # the block holds a window up to the capacity, that value included
    assert [int(v > cap) for v in sweep] == rises, (sweep, rises, cap, RECENTRE)


def test_fallback_boundary_pairs(emqx, ref):
    """One-topic windows on fresh pipes, the topic matching K0 .. K0 + 9 filters around the
    fresh pipe's pair capacity: want_p = floor(1.2 * 4.0 * 1) + 256 = 260 in
    host_pipe_enqueue_gather (fb_cases.fresh_caps).  The pairs' bytes stay below the byte
    capacity, so the pair count alone moves the outcome."""
    fid = ref[0]
    windows = []
    for d, k in enumerate(F.K_SWEEP):
        topics = (F.k_topic(d),)
        exp = F.expected(topics, fid, ref[1])
        assert len(exp[1]) == k and len(exp[4]) < F.fresh_caps(1)[1]
        windows.append((("pairs", k), topics, exp))
    rises = [r for _, r in _fresh_windows(emqx, ref, windows, False)]
    _one_switch(rises, F.K_SWEEP, F.fresh_caps(1)[0])


def test_fallback_boundary_bytes(emqx, ref):
    """One-topic windows of two pairs on fresh pipes (zero-copy input), one long filter's length
    moving the pairs' bytes over B0 .. B0 + 8 around the fresh pipe's byte capacity: want_b =
    floor(1.2 * 32 * 4.0 * 1) + 4096 = 4249 in host_pipe_enqueue_gather."""
    windows = []
    for j, b in enumerate(F.B_SWEEP):
        topics = (F.b_topic(j),)
        exp = F.expected(topics, ref[0], ref[1])
        assert len(exp[1]) == 2 and len(exp[4]) == b
        windows.append((("bytes", b), topics, exp))
    rises = [r for _, r in _fresh_windows(emqx, ref, windows, True)]
    _one_switch(rises, F.B_SWEEP, F.fresh_caps(1)[1])


def test_host_out_1(emqx, ref):
    """eng.tune("host_out", 1): the copy kernel brings rows, exact ids and filter ids to the host
    behind the pass, the gather's block follows; both gathers, on the plan with every edge filter
    across a tile edge."""
    eng = _new_engine(emqx, ref)
    eng.tune("host_out", 1)
    for plan in ("sparse-big", "p17", "p4097"):
        topics = F.plans()[plan][0]
        got = _run(eng, topics, "sync")
        _check((plan, "host_out 1 sync"), topics, got, ref[3][plan], ref[2])
        assert got[3] == 0
        _enqueued_until_block((plan, "host_out 1"), eng, topics, ref[3][plan], ref[2], False)
    eng.close()


def test_after_a_delta_commit(emqx, ref):
    """Further edge filters inserted and committed after the first windows: the appended device
    pool and offset mirror serve the old ids and the new ones."""
    eng = _new_engine(emqx, ref)
    old = F.plans()["lengths"][0]
    _check("before", old, _run(eng, old, "sync"), ref[3]["lengths"], ref[2])
    _enqueued_until_block("before", eng, old, ref[3]["lengths"], ref[2], True)
    fb, fo = F.pack(list(F.delta_filters()), np.uint64)
    new_ids = eng.trie_insert_many(fb, fo)
    key = F.delta_topics()[5]
    keys = dict(ref[1])
    keys[key] = eng.route_ref(key)
    eng.commit()
    fid = dict(ref[0])
    for f, i in zip(F.delta_filters(), new_ids):
        assert eng.lookup_id(f) == int(i) and f not in fid and int(i) not in fid.values()
        fid[f] = int(i)
    topics = tuple(t for pair in zip(F.delta_topics(), old) for t in pair) + old[len(F.delta_topics()):]
    exp = F.expected(topics, fid, keys, delta=True)
    assert len(exp[1]) == F.plans()["lengths"][1] + 3 * len(F.delta_topics())
    tab = F.table(fid)
    got = _run(eng, topics, "sync")
    _check("delta sync", topics, got, exp, tab)
    for pinned in (False, True):
        _enqueued_until_block(("delta", pinned), eng, topics, exp, tab, pinned)
    eng.close()
