"""Closed edge buckets on the device (gm_common.h EDGE_CLOSED; gm_walk.inc, the resolve and the
late match of keyed siblings): a lookup that finds neither its key nor an empty slot in a bucket
ends there when no edge was placed past the bucket.

Every case is matched against the Python restatement of emqx_trie (oracle/emqx_ref.py), rows
compared as sets, through the matrix tune "closed_buckets" 0/1 x "keyed_share" 0/1 x
"root_plus_half" 0/1 x "walk_pair" 0 (one lane per topic: the kernels with the rule), 1 (the
default choice) and 2 (every batch through the pair walk, compiled without it), and once through
the spilling walk.  The census of the miniature cfg3 (tests/closed_cases.py) equals the CPU
restatement's count with the rule on and the parent's figures with it off.  The failure the rule
could introduce is a lost match: an edge placed past a bucket that readers still take for
closed -- the delta case places edges past closed full buckets and matches the topics that need
them."""
import random

import pytest

import closed_cases
import walk_rule_cases as W

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _load(emqx, filters, bits=0, keyed=2):
    return W.load(emqx, filters, bits=bits, keyed=keyed)


def _check(eng, py, topics, what="", pairs=(0, 1, 2)):
    return W.check(eng, py, topics, what, ("closed_buckets", "root_plus_half", "keyed_share"), pairs)


def _census_both(eng, topics):
    c = {}
    for cb in (0, 1):
        eng.tune("closed_buckets", cb)
        c[cb] = W.census(eng, topics)
    eng.tune("closed_buckets", 1)
    return c


def test_miniature_cfg3_rows_and_census(emqx):
    """8 sites x 24 devices, 2,012 topics: rows through the matrix; the census with the rule off
    is the parent's, with it on the CPU restatement's (tests/test_closed_host.py asserts the same
    figures on the host), strictly fewer loads and lane iterations, the same states and pairs."""
    filters, topics = closed_cases.miniature()
    eng, py = _load(emqx, filters)
    _check(eng, py, topics, "full build")
    c = _census_both(eng, topics)
    print({k: (v["slot_loads"], v["lane_iters"], v["wave_iters"]) for k, v in c.items()})
    assert c[0]["pairs"] == c[1]["pairs"] and c[0]["states"] == c[1]["states"]
    assert (c[0]["slot_loads"], c[0]["lane_iters"]) == closed_cases.CENSUS[0]
    assert (c[1]["slot_loads"], c[1]["lane_iters"]) == closed_cases.CENSUS[1]
    assert c[1]["slot_loads"] < c[0]["slot_loads"] and c[1]["lane_iters"] < c[0]["lane_iters"]
    eng.close()


def test_miniature_cfg3_collision_tokens(emqx):
    """3-bit collision tokens (8 level tokens in all): crowded buckets and long chains."""
    rng = random.Random(34)
    filters = closed_cases.cfg3_filters(rng)
    topics = closed_cases.cfg3_topics(rng, 600)
    eng, py = _load(emqx, filters, bits=3)
    _check(eng, py, topics, "collision tokens")
    c = _census_both(eng, topics)
    assert c[0]["pairs"] == c[1]["pairs"] and c[0]["states"] == c[1]["states"]
    assert c[1]["slot_loads"] <= c[0]["slot_loads"] and c[1]["lane_iters"] <= c[0]["lane_iters"]
    eng.close()


def _random_trie(rng, deep=False):
    def word(lvl):
        return "w%d_%d" % (lvl, rng.randrange(3 + 2 * lvl))

    fs = set()
    for _ in range(900):
        depth = 2 + rng.randrange(6)
        ws = [("+" if l > 0 and rng.random() < 0.2 else word(l)) for l in range(depth)]
        fs.add("/".join(ws) + ("/#" if rng.random() < 0.33 else ""))
    ts = []
    for _ in range(1500):
        depth = 2 + rng.randrange(7)
        ts.append("/".join(("absent%d" % rng.randrange(50) if rng.random() < 0.33 else word(l))
                           for l in range(depth)))
    if deep:  # an item of level >= 16 cannot be a compact one: the batch ends in the spilling walk
        fs.add("/".join(["w0_0"] * 20))
        fs.add("/".join(["w0_0"] * 17 + ["+", "#"]))
        ts += ["/".join(["w0_0"] * 20), "/".join(["w0_0"] * 19 + ["absent1"])]
    return sorted(fs), ts


@pytest.mark.parametrize("keyed", [1, 2])
def test_random_trie_a_third_of_the_words_absent(emqx, keyed):
    rng = random.Random(57 + keyed)
    filters, topics = _random_trie(rng)
    eng, py = _load(emqx, filters, keyed=keyed)
    _check(eng, py, topics, "random trie")
    c = _census_both(eng, topics)
    print({k: (v["slot_loads"], v["lane_iters"]) for k, v in c.items()})
    assert c[0]["pairs"] == c[1]["pairs"] and c[0]["states"] == c[1]["states"]
    assert c[1]["slot_loads"] <= c[0]["slot_loads"] and c[1]["lane_iters"] <= c[0]["lane_iters"]
    eng.close()


def test_spilling_walk(emqx):
    """Filters and topics of 20 levels: the batch is redone up to the walk whose items spill to
    global memory ({node, level} pairs: no compact items, no late match) with the rule on and off."""
    rng = random.Random(61)
    filters, topics = _random_trie(rng, deep=True)
    eng, py = _load(emqx, filters)
    r0 = eng.stats()["reruns"]
    _check(eng, py, topics, "spilling walk", pairs=(1,))
    assert eng.stats()["reruns"] > r0
    eng.close()


def _fmix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def _keyed_home(word, nbk):
    """gm_common.h edge_home of a keyed parent's child: a hash of the word's token alone (a word of
    at most 7 bytes: its bytes little-endian, the length in bits 56..62)."""
    b = word.encode()
    assert len(b) <= 7
    tok = int.from_bytes(b, "little") | (len(b) << 56)
    return _fmix64((tok + 0x5851f42d4c957f2d) & M64) & (nbk - 1)


def test_delta_places_edges_past_closed_buckets(emqx):
    """Devices D with both edges (site/S/device, D) and (site/+/device, D) fill D's home bucket.
    New device words whose token has the same home are found by hash; for each, the census of its
    topic with the rule on and off tells whether that full bucket is closed (the rule ends the
    lookup of the absent device there: one load fewer).  One delta commit then adds
    site/S/device/<word>/# for all of them: the edges land past those buckets, which the commit
    must open, and every topic matches its new filter with the rule on and off."""
    filters, topics = closed_cases.miniature()
    eng, py = _load(emqx, filters)
    nodes = {""}
    for f in filters:
        ws = f.split("/")
        ws = ws[:-1] if ws[-1] == "#" else ws
        for i in range(1, len(ws) + 1):
            nodes.add("/".join(ws[:i]))
    ecap = 64
    while ecap < 4 * (len(nodes) - 1):  # gm_common.h EDGE_SLACK
        ecap *= 2
    nbk = ecap // 2
    fset = set(filters)
    full = {}
    for s in range(closed_cases.SITES):
        for j in range(closed_cases.DEVS):
            d = closed_cases.dev(s, j)
            if f"site/{s}/device/{d}/#" in fset and f"site/+/device/{d}/#" in fset:
                full[_keyed_home(str(d), nbk)] = d
    assert len(full) > 20
    cands = []
    for i in range(200000):
        w = "x%d" % i
        if _keyed_home(w, nbk) in full:
            cands.append(w)
            if len(cands) == 12:
                break
    assert len(cands) == 12
    new_topics, closed = [], 0
    for i, w in enumerate(cands):
        t = f"site/{i % closed_cases.SITES}/device/{w}/m1/3"
        c = _census_both(eng, [t])
        assert c[1]["slot_loads"] <= c[0]["slot_loads"]
        closed += c[1]["slot_loads"] < c[0]["slot_loads"]
        new_topics.append(t)
    print("candidates whose full home bucket is closed:", closed, "of", len(cands))
    assert closed >= 3
    d0 = eng.stats()["delta_commits"]
    for i, w in enumerate(cands):
        f = f"site/{i % closed_cases.SITES}/device/{w}/#".encode()
        eng.trie_insert(f)
        py.insert(f)
    eng.commit()
    assert eng.stats()["delta_commits"] == d0 + 1
    want = _check(eng, py, new_topics + topics[:400], "after the delta")
    assert all(len(w) >= 1 for w in want[:len(cands)])
    # the buckets are open now: the rule no longer ends the lookups of other absent devices there
    # early, and still changes no row; then the edges go again and come back into their TOMB slots
    for i, w in enumerate(cands[:6]):
        f = f"site/{i % closed_cases.SITES}/device/{w}/#".encode()
        eng.trie_delete(f)
        py.delete(f)
    eng.commit()
    _check(eng, py, new_topics + topics[:400], "after the deletes", pairs=(0,))
    for i, w in enumerate(cands[:6]):
        f = f"site/{i % closed_cases.SITES}/device/{w}/#".encode()
        eng.trie_insert(f)
        py.insert(f)
    eng.commit()
    _check(eng, py, new_topics + topics[:400], "after the re-inserts", pairs=(0,))
    assert eng.stats()["delta_commits"] == d0 + 3
    eng.close()
