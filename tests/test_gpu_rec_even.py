"""Even-elided topic records on the device (gm_common.h; k_tok's store_rec<EVEN>,
k_walk's REC_REVEN reader).

A three-part pass over an index whose literal edges of level 0, and those of level 2, each carry
at most one token stores two parts {tok1, tok3} {tok4, tok5} and a header bit for each of the
words 0 and 2, where its walk has the reader: the one-lane-per-topic walks (tune "walk_pair" 0 for
the small batches here) and the census.  tune "rec_even" 0 keeps three parts, "rec_parts" 4 full
records.  Every row is compared, by filter name, with the Python restatement of emqx_trie
(oracle/emqx_ref.py) through rec_even 0 / 1 x rec_parts 0 / 4 x walk_pair 0 / 1 / 2, and
stats()["even_passes"] must move exactly when the form is to be taken."""
import ctypes

import numpy as np
import pytest

import closed_cases
import walk_rule_cases as W

pytestmark = pytest.mark.gpu

TOK_NT_MIN = 2 << 20  # gm_tok.inc
BATCHES = (1, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _filters(w0s=("site",), w2s=("device",)):
    """Filters of up to six levels shaped W0/<s>/W2/<d>/<m>/<k>: literal, '+' and '#' at every
    level, for every word of w0s at level 0 and of w2s at level 2."""
    fs = {"#", "+/+/+/7/#"}
    for w0 in w0s:
        fs |= {w0 + "/#", w0 + "/+", w0 + "/1", w0 + "/1/#"} | ({w0} if w0 else set())
        for w2 in w2s:
            p = "%s/1/%s" % (w0, w2)
            fs |= {p, p + "/#", p + "/+", p + "/7", p + "/7/#", p + "/7/m1", p + "/7/+/3", p + "/7/m1/3",
                   p + "/7/m1/", p + "/+/m1/3", "%s/+/%s/7/#" % (w0, w2), "%s/+/%s/+/m1" % (w0, w2),
                   "+/1/%s/7/m1/3" % w2, "+/+/%s/8/#" % w2, "%s/2/%s/8/m2/4" % (w0, w2),
                   "%s/2/+/8/m2/4" % w0, "%s/2/%s/eight888/#" % (w0, w2)}
    return sorted(fs)


def _off(w):
    """w with its last byte one up."""
    return w[:-1] + chr(ord(w[-1]) + 1)


def _topics(w0="site", w2="device"):
    """Topics of 1 to 9 levels whose word 0 or 2 equals the level's word, differs from it by one
    byte, is empty, is missing, or is an 8-byte word; '$' names, wildcard names, "" and "/"."""
    tail = ["1", w2, "7", "m1", "3", "a", "b", "c"]
    ts = ["", "/", "$SYS", "$SYS/x", "$" + w0, "$%s/1/%s/7" % (w0, w2), "+", "#", w0 + "/+/" + w2,
          w0 + "/#", w0 + "/1/" + w2 + "/+/m1", "/".join([w0] + tail + ["d"] * 21)]
    for n in range(1, 10):
        for a in (w0, _off(w0), "", "eight888", w2):
            for b in (w2, _off(w2), "", "eight888", w0):
                ws = ([a] + tail)[:n]
                if n > 2:
                    ws[2] = b
                ts.append("/".join(ws))
    for d in ("7", "8", "9", "eight888"):
        ts += ["%s/2/%s/%s/m2/4" % (w0, w2, d), "%s/3/%s/%s/m1" % (w0, w2, d), "x/1/%s/%s/m1/3" % (w2, d)]
    return list(dict.fromkeys(ts))


def _names(eng, res, n):
    cache = {}

    def name(f):
        if f not in cache:
            cache[f] = eng.filter_bytes(f)
        return cache[f]

    return [sorted(name(int(f)) for f in res.row(i)) for i in range(n)]


def _check(eng, py, topics, what, eligible, pairs=(0, 1, 2), parts=(0, 4), evens=(1, 0)):
    """Rows equal the oracle's through rec_even x rec_parts x walk_pair, and even_passes moves
    exactly for rec_even 1, rec_parts 0, one lane per topic (these batches are small: walk_pair 1
    and 2 run the pair walk) on an index whose levels 0 and 2 allow it.  Defaults afterwards."""
    tb = W._bytes(topics)
    want = [sorted(py.match(t)) for t in tb]
    for ev in evens:
        eng.tune("rec_even", ev)
        for rp in parts:
            eng.tune("rec_parts", rp)
            for pair in pairs:
                eng.tune("walk_pair", pair)
                e0 = eng.stats()["even_passes"]
                got = _names(eng, eng.match(tb), len(tb))
                taken = eng.stats()["even_passes"] - e0
                for i, t in enumerate(tb):
                    assert got[i] == want[i], (what, ev, rp, pair, t)
                assert (taken > 0) == bool(eligible and ev == 1 and rp == 0 and pair == 0), (what, ev, rp, pair, taken)
    eng.tune("rec_even", 1)
    eng.tune("rec_parts", 0)
    eng.tune("walk_pair", 1)
    return want


INDEXES = {
    # name: (filters, topic words, takes the form, word_hash_bits)
    "one/one": (_filters(), ("site", "device"), True, 0),
    "one/many": (_filters(w2s=("device", "sensor")), ("site", "device"), False, 0),
    "many/one": (_filters(w0s=("site", "plant")), ("site", "device"), False, 0),
    "none": (["#", "site", "site/#", "site/+", "site/1", "+/1", "site/1/#", "+/#"], ("site", "device"), True, 0),
    "empty word at level 0": (_filters(w0s=("",)), ("", "device"), False, 0),
    "8-byte c2": (_filters(w2s=("device88",)), ("site", "device88"), True, 0),
    "collision tokens": (_filters(), ("site", "device"), True, 3),
}


@pytest.mark.parametrize("name", list(INDEXES))
def test_indexes_topics_and_block_edges(emqx, name):
    filters, (w0, w2), eligible, bits = INDEXES[name]
    eng, py = W.load(emqx, filters, bits=bits)
    topics = _topics(w0 or "site", w2)
    if not w0:
        topics += _topics("x", w2)[:40] + ["/1/device/7/m1/3", "/1/device", "/2/device/8/m2/4"]
    _check(eng, py, topics, name, eligible)
    for k, n in enumerate(BATCHES):
        batch = [topics[(11 * k + i) % len(topics)] for i in range(n)]
        _check(eng, py, batch, "%s: batch of %d" % (name, n), eligible, pairs=(0, 1), parts=(0,))
    eng.close()


def test_rec_even_tune_values(emqx):
    eng = emqx.Engine()
    for ok in (0, 1, 0, 1):
        eng.tune("rec_even", ok)
    for bad in (-1, 2, 4):
        with pytest.raises(Exception):
            eng.tune("rec_even", bad)
    eng.close()


def test_tn_key_with_dollar_topics(emqx):
    """A '$' name's own key ($SYS, a `tn` key of level 0) is a literal edge of level 0: with it the
    level has two tokens and passes keep three parts; alone it is the one token."""
    eng, py = W.load(emqx, _filters() + ["$SYS"])
    _check(eng, py, _topics(), "site and $SYS", False, pairs=(0, 1))
    eng.close()
    eng, py = W.load(emqx, ["$SYS", "$SYS/#", "$SYS/+", "+/x", "#"])
    _check(eng, py, ["$SYS", "$SYS/x", "$SYT", "$SYS/", "SYS", "", "/", "$SYS/x/y", "a/x"], "$SYS alone", True, pairs=(0, 1))
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


@pytest.mark.parametrize("path", ["dev1", "dev15", "copy-through", "host-pipe-dma"])
def test_entry_paths(emqx, path):
    """match_device at a shifted byte address, and the host pipes with the copy-through k_tok and
    with DMA copies (as tests/test_gpu_rec_parts.py reaches them), one lane per topic."""
    from emqx_amd.engine import pack
    eng, py = W.load(emqx, _filters())
    eng.tune("walk_pair", 0)
    topics = W._bytes(_topics())
    want = [sorted(py.match(t)) for t in topics]
    tb, to = pack(topics, np.uint32)
    n = len(topics)
    e0 = eng.stats()["even_passes"]
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
    assert eng.stats()["even_passes"] > e0, path
    for i, t in enumerate(topics):
        assert got[i] == want[i], (path, t)
    eng.close()


def _commit_delta(eng, py, adds=(), dels=()):
    d0 = eng.stats()["delta_commits"]
    for f in adds:
        eng.trie_insert(f.encode())
        py.insert(f.encode())
    for f in dels:
        eng.trie_delete(f.encode())
        py.delete(f.encode())
    eng.commit()
    assert eng.stats()["delta_commits"] == d0 + 1


def test_deltas_add_a_second_token_between_passes(emqx):
    """A second token at level 0, then at level 2, by delta commits between passes: the passes
    after each commit run three parts and find the new filter.  Deleting it leaves three parts (a
    delta never lowers the state); a full rebuild returns to the two-part form."""
    for new, topic in (("plant/1/device/7/#", "plant/1/device/7/m1/3"),
                       ("site/1/sensor/7/#", "site/1/sensor/7/m1/3"),
                       ("+/1/sensor/7/#", "x/1/sensor/7/m1")):
        eng, py = W.load(emqx, _filters())
        topics = _topics() + [topic]
        _check(eng, py, topics, "before", True, pairs=(0, 1), parts=(0,))
        _commit_delta(eng, py, adds=[new])
        want = _check(eng, py, topics, "after " + new, False, pairs=(0, 1), parts=(0,))
        assert new.encode() in want[-1]
        _commit_delta(eng, py, dels=[new])
        want = _check(eng, py, topics, "deleted " + new, False, pairs=(0, 1), parts=(0,))
        assert new.encode() not in want[-1]
        f0 = eng.stats()["full_commits"]
        eng.tune("fat_buckets", 1)  # (invalidates the host model: the next commit builds in full)
        eng.trie_insert(b"site/1/device/9/late")
        py.insert(b"site/1/device/9/late")
        eng.commit()
        assert eng.stats()["full_commits"] == f0 + 1
        _check(eng, py, topics, "rebuilt", True, pairs=(0, 1), parts=(0,))
        eng.close()


@pytest.mark.parametrize("new", ["plant/1/device/7/#", "site/1/sensor/7/#"])
def test_delta_with_a_pass_in_flight(emqx, new):
    """submit, commit, wait: the pass in flight was enqueued in the two-part form against the
    epoch whose levels 0 and 2 had one token each and gives that epoch's rows; the next pass
    stores three parts and finds the new filter."""
    from emqx_amd.engine import pack
    eng, py = W.load(emqx, _filters())
    eng.tune("walk_pair", 0)
    hit = new[:-1] + "m1/3"
    topics = W._bytes((_topics() + [hit]) * 20)
    before = [sorted(py.match(t)) for t in topics]
    tb, to = pack(topics, np.uint32)
    n = len(topics)
    big, do = _on_device(tb, to, 0)
    e0 = eng.stats()["even_passes"]
    ticket = eng.match_device_submit(big.data_ptr(), do.data_ptr(), n, int(to[-1]))
    assert eng.stats()["even_passes"] == e0 + 1  # (enqueued once so far: a redo comes with the wait)
    _commit_delta(eng, py, adds=[new])
    got = _dev_rows(eng, eng.match_device_wait(ticket), n)
    for i, t in enumerate(topics):
        assert got[i] == before[i], ("in flight", t)
    after = [sorted(py.match(t)) for t in topics]
    assert after != before and new.encode() in after[-1]
    e1 = eng.stats()["even_passes"]
    got = _dev_rows(eng, eng.match_device(big.data_ptr(), do.data_ptr(), n, int(to[-1])), n)
    assert eng.stats()["even_passes"] == e1
    for i, t in enumerate(topics):
        assert got[i] == after[i], ("after the commit", t)
    eng.close()


def test_miniature_cfg3_rows_and_census(emqx):
    """The 2,012-topic miniature cfg3 (levels 0 and 2: `site`, `device`): rows through the matrix,
    2,135 pairs in both forms, and the census's bucket loads and lane iterations of both forms.
    The three-part figures are tests/closed_cases.py's.  In the two-part form a word that differs
    from c_k reads 0, whose signature class may differ from the word's: a literal probe more or
    fewer for such a topic, never a row.  Measured on the MI355X: no difference on this batch --
    17,719 states, 4,742 bucket loads, 2,654 lane iterations, 2,135 pairs in both forms (its four
    such topics end at the root, whose only literal child rides in the arguments and is compared,
    not probed)."""
    filters, topics = closed_cases.miniature()
    eng, py = W.load(emqx, filters)
    assert eng.stats()["max_depth"] == 6
    _check(eng, py, topics, "miniature", True)
    c = {}
    for ev in (0, 1):
        eng.tune("rec_even", ev)
        e0 = eng.stats()["even_passes"]
        c[ev] = W.census(eng, topics)
        assert (eng.stats()["even_passes"] > e0) == (ev == 1)
    eng.tune("rec_even", 1)
    print({k: (v["states"], v["slot_loads"], v["lane_iters"], v["pairs"]) for k, v in c.items()})
    assert c[0]["pairs"] == c[1]["pairs"] == 2135
    assert (c[0]["slot_loads"], c[0]["lane_iters"]) == closed_cases.CENSUS[1]
    # the topics whose word 0 or 2 is not `site` / `device`: "$site...", "other/1/device/..." and
    # "$SYS/x" of the 2,012 -- the only ones a reconstructed 0 can change a probe for
    odd = sum(1 for t in topics if t.split("/")[0] != "site" or (t.count("/") >= 2 and t.split("/")[2] != "device"))
    # (such a topic has at most the states site/S and site/+ at level 2, each with one literal
    # probe that its class can add or drop, a bucket or two long)
    assert abs(c[1]["slot_loads"] - c[0]["slot_loads"]) <= 4 * odd
    assert abs(c[1]["lane_iters"] - c[0]["lane_iters"]) <= 4 * odd
    assert abs(c[1]["states"] - c[0]["states"]) == 0
    eng.close()


def test_large_batch_nontemporal_two_part_records(emqx):
    """From TOK_NT_MIN topics on k_tok stores its records -- two parts and the header words here --
    non-temporally, and the batch is walked one lane per topic by default: the miniature repeated
    to just over that many topics; every repetition's rows are the small batch's."""
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

    e0 = eng.stats()["even_passes"]
    res = eng.match_packed(big_b, big_o, copy=False)
    assert eng.stats()["even_passes"] > e0  # (walk_pair 1: a batch this large is not paired)
    cnt = np.diff(res.row_ptr.astype(np.int64)).reshape(reps, n)
    assert (cnt == np.diff(small.row_ptr.astype(np.int64))[None, :]).all()
    sid = sorted_ids(small)
    assert (sorted_ids(res).reshape(reps, len(sid)) == sid[None, :]).all()
    eng.close()
