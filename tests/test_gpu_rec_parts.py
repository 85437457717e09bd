"""Topic records stored and loaded in the parts the index can read (gm_common.h rec_parts; k_tok's
store_rec, k_walk's load_rec) on the device.

A pass over an index whose deepest filter has fewer than seven levels stores three of a record's
four 16-B parts and a 4-B header word per topic; from seven levels on it stores full records.
tune "rec_parts" 4 forces full records.  Every row here is compared, by filter name, with the
Python restatement of emqx_trie (oracle/emqx_ref.py): indexes of 5, 6, 7 and 8 levels (both sides
of the 3 | 4 boundary), topics of 1 to 9 levels, batches at the edges of the 64-topic blocks of the
parts and of the header line, rec_parts 0 / 4 x walk_pair 0 / 1 / 2, the entry paths that stage the
bytes elsewhere, delta commits that deepen a six-level index, and a batch large enough for the
non-temporal stores."""
import ctypes
import random

import numpy as np
import pytest

import closed_cases
import walk_rule_cases as W
from oracle import emqx_ref as R

pytestmark = pytest.mark.gpu

TOK_NT_MIN = 2 << 20  # gm_tok.inc


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _chain(n):
    return ["w%d" % i for i in range(n)]


def _filters(depth):
    """An index whose deepest filters have `depth` levels: literal chains, '+' at every level,
    '#' ends, an empty level, and at the last level a 7-byte (packed) word, an 8-byte (hashed)
    word and the empty word (token 0, what a token not stored reads as)."""
    c = _chain(depth)
    fs = {"#", "+/w1/#", "w0/#", "w0/+", "w0/w1", "w0//w2", "$SYS/#", "$SYS/+", "$w0/w1", "+", "w0"}
    for last in (c[-1], "seven77", "eight888", "", "+"):
        fs.add("/".join(c[:-1] + [last]))
        fs.add("/".join(["+"] + c[1:-1] + [last]))  # (a wildcard filter: the trie's match returns it)
    for i in range(depth):  # one '+' at level i
        fs.add("/".join(c[:i] + ["+"] + c[i + 1:]))
    for i in range(1, depth):  # shorter chains, plain and with '#'
        fs.add("/".join(c[:i]) + "/#")
        fs.add("/".join(c[:i]))
    fs.add("/".join(["+"] * depth))
    assert max(len(f.split("/")) - (f.endswith("/#") or f == "#") for f in fs) == depth
    return sorted(fs)


def _topics(depth):
    """Topics of 1 to 9 levels around the chains of _filters(depth)."""
    ts = ["", "/", "$", "$SYS", "$SYS/x", "$w0/w1", "$w0", "+", "#", "w0/+/w2", "w0/#", "w0//w2",
          "w0///w3", "/w1"]
    c = _chain(9)
    for n in range(1, 10):
        for last in (c[n - 1], "seven77", "eight888", "", "absent", "sevenXX", "eightXXX"):
            ts.append("/".join(c[:n - 1] + [last]))
        if n > 2:
            ts.append("/".join(c[:1] + ["other"] + c[2:n]))
            ts.append("/".join(c[:n - 2] + ["", c[n - 1]]))
    # the levels right behind the index's last one, and a topic far deeper than any filter
    ts.append("/".join(_chain(depth) + ["seven77"]))
    ts.append("/".join(_chain(depth) + [""]))
    ts.append("/".join(_chain(depth - 1) + ["eight888", "w%d" % depth]))
    ts.append("/".join(_chain(30)))
    return ts


def _rows(eng, topics):
    """The engine's rows by filter name, sorted."""
    res = eng.match(W._bytes(topics))
    names = {}

    def name(f):
        if f not in names:
            names[f] = eng.filter_bytes(f)
        return names[f]

    return [sorted(name(int(f)) for f in res.row(i)) for i in range(len(topics))]


def _check(eng, py, topics, what, pairs=(0, 1, 2), parts=(0, 4)):
    """Rows equal the oracle's through rec_parts x walk_pair; the defaults are back afterwards."""
    tb = W._bytes(topics)
    want = [sorted(py.match(t)) for t in tb]
    for rp in parts:
        eng.tune("rec_parts", rp)
        for pair in pairs:
            eng.tune("walk_pair", pair)
            got = _rows(eng, tb)
            for i, t in enumerate(tb):
                assert got[i] == want[i], (what, rp, pair, t)
    eng.tune("rec_parts", 0)
    eng.tune("walk_pair", 1)
    return want


@pytest.mark.parametrize("depth", [5, 6, 7, 8])
def test_index_depths_topic_depths_and_block_edges(emqx, depth):
    eng, py = W.load(emqx, _filters(depth))
    assert eng.stats()["max_depth"] == depth
    topics = _topics(depth)
    _check(eng, py, topics, "all topics")
    for k, n in enumerate((1, 63, 64, 65, 129)):
        batch = [topics[(7 * k + i) % len(topics)] for i in range(n)]
        _check(eng, py, batch, "batch of %d" % n)
    eng.close()


def test_rec_parts_tune_values(emqx):
    eng = emqx.Engine()
    for ok in (0, 4, 0):
        eng.tune("rec_parts", ok)
    for bad in (-1, 1, 2, 3, 5):
        with pytest.raises(Exception):
            eng.tune("rec_parts", bad)
    eng.close()


def test_miniature_cfg3_rows_and_census(emqx):
    """The 2,012-topic miniature cfg3 (six levels: three parts): rows through the matrix; the
    census walk counts the same states, bucket loads, lane iterations and pairs with partial and
    with full records -- the figures tests/closed_cases.py records."""
    filters, topics = closed_cases.miniature()
    eng, py = W.load(emqx, filters)
    assert eng.stats()["max_depth"] == 6
    _check(eng, py, topics, "miniature")
    c = {}
    for rp in (0, 4):
        eng.tune("rec_parts", rp)
        c[rp] = W.census(eng, topics)
    eng.tune("rec_parts", 0)
    print({k: (v["states"], v["slot_loads"], v["lane_iters"], v["pairs"]) for k, v in c.items()})
    for key in ("states", "slot_loads", "lane_iters", "pairs"):
        assert c[0][key] == c[4][key], key
    assert (c[0]["slot_loads"], c[0]["lane_iters"]) == closed_cases.CENSUS[1]
    eng.close()


def test_spilling_walk(emqx):
    """Filters and topics of 20 levels beside a random trie, as tests/test_gpu_closed.py builds
    them: the batch is redone up to the walk whose items spill to global memory."""
    rng = random.Random(61)

    def word(lvl):
        return "w%d_%d" % (lvl, rng.randrange(3 + 2 * lvl))

    fs = set()
    for _ in range(900):
        d = 2 + rng.randrange(6)
        ws = [("+" if l > 0 and rng.random() < 0.2 else word(l)) for l in range(d)]
        fs.add("/".join(ws) + ("/#" if rng.random() < 0.33 else ""))
    ts = []
    for _ in range(1500):
        d = 2 + rng.randrange(7)
        ts.append("/".join(("absent%d" % rng.randrange(50) if rng.random() < 0.33 else word(l))
                           for l in range(d)))
    fs.add("/".join(["w0_0"] * 20))
    fs.add("/".join(["w0_0"] * 17 + ["+", "#"]))
    ts += ["/".join(["w0_0"] * 20), "/".join(["w0_0"] * 19 + ["absent1"])]
    eng, py = W.load(emqx, sorted(fs))
    r0 = eng.stats()["reruns"]
    _check(eng, py, ts, "spilling walk", pairs=(1,))
    assert eng.stats()["reruns"] > r0
    eng.close()


def test_bushy_six_level_index(emqx):
    """Every literal / '+' combination over six levels: the widest searches an index of three
    parts can ask for (the walk variants beyond the shallow one-lane walk take over if a lane's
    stack overflows)."""
    c = _chain(6)
    fs = set()
    for m in range(64):
        ws = [("+" if (m >> l) & 1 else c[l]) for l in range(6)]
        fs.add("/".join(ws))
        fs.add("/".join(ws[:5]) + "/#")
    eng, py = W.load(emqx, sorted(fs))
    assert eng.stats()["max_depth"] == 6
    ts = ["/".join(c), "/".join(c[:5] + ["x"]), "/".join(c[:5]), "/".join(c + ["deeper"]),
          "/".join(["x"] * 6), "$" + "/".join(c)] * 40
    _check(eng, py, ts, "bushy")
    print("reruns", eng.stats()["reruns"])
    eng.close()


def _dev_rows(eng, d, n):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    row, fid = np.empty(n + 1, np.uint32), np.empty(d.n_pairs, np.uint32)
    for a, p in ((row, d.row_ptr), (fid, d.filter_id)):
        if a.nbytes:
            assert hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0
    return [sorted(eng.filter_bytes(int(f)) for f in fid[int(row[i]):int(row[i + 1])])
            for i in range(n)]


def _on_device(tb, to, shift):
    import torch
    big = torch.full((len(tb) + 64,), 0x2F, dtype=torch.uint8, device="cuda")
    big[shift:shift + len(tb)].copy_(torch.from_numpy(np.array(tb)))
    do = torch.from_numpy(np.array(to).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return big, do


@pytest.mark.parametrize("depth", [6, 7])
@pytest.mark.parametrize("path", ["dev1", "dev15", "copy-through", "host-pipe-dma"])
def test_entry_paths(emqx, depth, path):
    """match_device at a shifted byte address, and the host pipes with the copy-through k_tok and
    with DMA copies (as tests/test_gpu_tok_edges.py reaches them)."""
    from emqx_amd.engine import pack
    eng, py = W.load(emqx, _filters(depth))
    topics = W._bytes(_topics(depth))
    want = [sorted(py.match(t)) for t in topics]
    tb, to = pack(topics, np.uint32)
    n = len(topics)
    if path.startswith("dev"):
        shift = int(path[3:])
        big, do = _on_device(tb, to, shift)
        got = _dev_rows(eng, eng.match_device(big.data_ptr() + shift, do.data_ptr(), n, int(to[-1])), n)
    else:
        eng.tune("zc_topics", 65536 if path == "copy-through" else 0)
        hb, ho = eng.pinned(len(tb)), eng.pinned(n + 1, np.uint32)
        hb[:], ho[:] = tb, to
        res, _, _ = eng.match_batch_wait_filters(eng.match_batch_submit(hb, ho, filters=True))
        got = [sorted(eng.filter_bytes(int(f)) for f in res.row(i)) for i in range(n)]
    for i, t in enumerate(topics):
        assert got[i] == want[i], (path, depth, t)
    eng.close()


def test_delta_commits_deepen_a_six_level_index(emqx):
    """A six-level index (three parts) grows to seven and then eight levels by delta commits
    between passes: the passes after each commit store full records and match the new filters."""
    eng, py = W.load(emqx, _filters(6))
    topics = _topics(6) + ["/".join(_chain(7)), "/".join(_chain(8)), "/".join(_chain(6) + [""]),
                           "/".join(_chain(6) + ["eight888", "w7"])]
    _check(eng, py, topics, "six levels", pairs=(0, 1))
    d0 = eng.stats()["delta_commits"]
    c = _chain(8)
    for k, new in enumerate((["/".join(c[:5] + ["+", "w6"]), "/".join(["+"] + c[1:6] + [""])],
                             ["/".join(["+"] + c[1:8]), "/".join(c[:6] + ["eight888", "+"])])):
        for f in new:
            eng.trie_insert(f.encode())
            py.insert(f.encode())
        eng.commit()
        assert eng.stats()["delta_commits"] == d0 + 1 + k
        assert eng.stats()["max_depth"] == 7 + k
        want = _check(eng, py, topics, "%d levels" % (7 + k), pairs=(0, 1))
        assert any(f.encode() in w for f in new for w in want)
    eng.close()


def test_delta_commit_with_a_pass_in_flight(emqx):
    """submit, commit, wait: the pass in flight was enqueued with three parts against the
    six-level epoch and gives that epoch's rows; the commit's patches wait for it; the next pass
    stores full records and sees the seven-level filter."""
    from emqx_amd.engine import pack
    eng, py = W.load(emqx, _filters(6))
    topics = W._bytes(_topics(6) + ["/".join(_chain(7)), "/".join(_chain(6) + [""])] * 50)
    before = [sorted(py.match(t)) for t in topics]
    tb, to = pack(topics, np.uint32)
    n = len(topics)
    big, do = _on_device(tb, to, 0)
    d0 = eng.stats()["delta_commits"]
    ticket = eng.match_device_submit(big.data_ptr(), do.data_ptr(), n, int(to[-1]))
    for f in ("/".join(_chain(5) + ["+", "w6"]), "/".join(["+"] + _chain(6)[1:] + [""])):
        eng.trie_insert(f.encode())
        py.insert(f.encode())
    eng.commit()
    got = _dev_rows(eng, eng.match_device_wait(ticket), n)
    assert eng.stats()["delta_commits"] == d0 + 1
    for i, t in enumerate(topics):
        assert got[i] == before[i], ("in flight", t)
    after = [sorted(py.match(t)) for t in topics]
    assert after != before
    got = _dev_rows(eng, eng.match_device(big.data_ptr(), do.data_ptr(), n, int(to[-1])), n)
    for i, t in enumerate(topics):
        assert got[i] == after[i], ("after the commit", t)
    eng.close()


def test_large_batch_nontemporal_partial_records(emqx):
    """From TOK_NT_MIN topics on k_tok stores its records -- three parts and the header words here
    -- non-temporally: the miniature repeated to just over that many topics against its six-level
    index; every repetition's rows are the small batch's."""
    from emqx_amd.engine import pack
    filters, topics = closed_cases.miniature()
    eng, py = W.load(emqx, filters)
    tb, to = pack(W._bytes(topics), np.uint32)
    n = len(topics)
    small = eng.match_packed(tb, to)
    want = [sorted(py.match(t)) for t in W._bytes(topics)]
    for i in range(n):
        assert sorted(eng.filter_bytes(int(f)) for f in small.row(i)) == want[i], topics[i]
    reps = TOK_NT_MIN // n + 1
    assert reps * n >= TOK_NT_MIN and reps * int(to[-1]) < 1 << 31
    big_b = np.tile(tb, reps)
    big_o = np.empty(reps * n + 1, np.uint32)
    big_o[:-1] = (np.arange(reps, dtype=np.uint32)[:, None] * np.uint32(to[-1]) + to[None, :-1]).ravel()
    big_o[-1] = reps * int(to[-1])

    def sorted_ids(res):
        row = res.row_ptr.astype(np.int64)
        seg = np.repeat(np.arange(len(row) - 1, dtype=np.int64), np.diff(row))
        return res.filter_id[np.lexsort((res.filter_id, seg))]

    res = eng.match_packed(big_b, big_o, copy=False)
    cnt = np.diff(res.row_ptr.astype(np.int64)).reshape(reps, n)
    assert (cnt == np.diff(small.row_ptr.astype(np.int64))[None, :]).all()
    sid = sorted_ids(small)
    assert (sorted_ids(res).reshape(reps, len(sid)) == sid[None, :]).all()
    eng.close()
