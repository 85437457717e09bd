"""The root's '+' half and the shared line of keyed siblings on the device (gm_walk.inc create's
RP, k_walk's SHARE): the slot of the only literal child H of G/+ (G the root's only literal
child; cfg3: site/+ -> device) rides in the walk's arguments, and the keyed items of one topic
at one level -- one home bucket, a hash of the level's token alone -- are decided from one
loaded line.

Every case is matched against the Python restatement of emqx_trie (oracle/emqx_ref.py), rows
compared as sets, through the full matrix: tune "root_plus_half" 0/1 x "keyed_share" 0/1 x
"walk_pair" 0 (one lane per topic: the kernels with both rules), 1 (the default choice) and 2
(every batch through the pair walk, compiled without them).  tune "keyed" 2 makes small parents
keyed, so that site/S/device and site/+/device share the line of a device D."""
import random

import pytest

import walk_rule_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _load(emqx, filters, bits=0):
    return W.load(emqx, filters, bits=bits, keyed=2, dedup_sorted=True)


def _check(eng, py, topics, what=""):
    return W.check(eng, py, topics, what, ("root_plus_half", "keyed_share"))


def _step(eng, py, topics, what, add=(), delete=()):
    for f in delete:
        eng.trie_delete(f.encode())
        py.delete(f.encode())
    for f in add:
        eng.trie_insert(f.encode())
        py.insert(f.encode())
    eng.commit()
    return _check(eng, py, topics, what)


SITES, DEVS = 8, 24


def _dev(s, j):
    return s * DEVS + j  # global device ids: a token D has the two parents site/s/device, site/+/device


def _cfg3(rng):
    """workloads/gen.cpp gen_cfg3 in miniature: its five filter patterns."""
    fs = set()
    for s in range(SITES):
        for j in range(DEVS):
            d = _dev(s, j)
            r = rng.random()
            if r < 0.7:
                fs.add(f"site/{s}/device/{d}/#")         # the first edge of D
            if r > 0.4:
                fs.add(f"site/+/device/{d}/#")           # the second (0.4 .. 0.7: both)
            if rng.random() < 0.3:
                for k in range(16):
                    if rng.random() < 0.25:
                        fs.add(f"site/{s}/device/{d}/+/{k}")
        for m in range(8):
            if rng.random() < 0.5:
                fs.add(f"site/{s}/device/+/m{m}")
            if rng.random() < 0.3:
                fs.add(f"site/{s}/+/+/m{m}")
    return sorted(fs)


def _cfg3_topics(rng, n):
    ts = []
    for _ in range(n):
        s = rng.randrange(SITES + 1)  # (site 8: no such site)
        d = _dev(s, rng.randrange(DEVS + 2)) if rng.random() < 0.9 else rng.randrange(400)
        ts.append(f"site/{s}/device/{d}/m{rng.randrange(9)}/{rng.randrange(16)}")
    # 1, 2, 3, 6, 8 and 17 levels; a '$' first word; a wildcard name
    ts += ["site", "site/1", "site/1/device", "site/1/device/24", "site/1/device/24/m1/3",
           "site/1/device/24/m1/3/a/b", "site/1/device/24/" + "/".join("l%d" % i for i in range(13)),
           "$site/1/device/24/m1/3", "$site", "$SYS/x", "site/+/device/24/m1/3", "other/1/device/24/m1/3"]
    return ts


@pytest.mark.parametrize("bits", [0, 3])
def test_miniature_cfg3(emqx, bits):
    """8 sites x 24 devices, all five patterns, 2,000 topics.  bits = 3: collision tokens (8
    level tokens in all), so home buckets are full of other keys and the chains continue."""
    rng = random.Random(31 + bits)
    filters = _cfg3(rng)
    topics = _cfg3_topics(rng, 2000)
    eng, py = _load(emqx, filters, bits=bits)
    want = _check(eng, py, topics, "full build")
    assert sum(1 for w in want if len(w) >= 2) > 200  # (topics that match under both parents)
    if bits == 0:
        # the census walk has both rules: each removes bucket loads, neither changes the pairs.
        # With both, a topic's (site/+, device) probe is gone and its two D probes are one load:
        # at least one load less for every topic under a known site (1,500 of 2,000 and more).
        c = {}
        for rp in (0, 1):
            for ks in (0, 1):
                eng.tune("root_plus_half", rp)
                eng.tune("keyed_share", ks)
                c[rp, ks] = W.census(eng, topics)
        eng.tune("root_plus_half", 1)
        eng.tune("keyed_share", 1)
        print({k: (v["slot_loads"], v["lane_iters"]) for k, v in c.items()})
        assert len({v["pairs"] for v in c.values()}) == 1 and len({v["states"] for v in c.values()}) == 1
        assert c[1, 0]["slot_loads"] < c[0, 0]["slot_loads"] and c[0, 1]["slot_loads"] < c[0, 0]["slot_loads"]
        assert c[0, 0]["slot_loads"] - c[1, 1]["slot_loads"] >= 1500
        assert c[1, 1]["lane_iters"] < c[0, 0]["lane_iters"]
    eng.close()


@pytest.mark.parametrize("kids", [0, 1, 2])
def test_literal_children_under_the_plus_child(emqx, kids):
    """G/+ with no, one and two literal children: the copy exists only for one."""
    fs = ["g/a/h/x", "g/a/#", "g/+", "g/+/+/z", "g/b/h2/y"]
    fs += ["g/+/h/#", "g/+/h/q"][: 2 * min(kids, 1)] + ["g/+/h2/+"][: max(kids - 1, 0)]
    ts = ["g", "g/a", "g/a/h", "g/a/h/x", "g/a/h/q", "g/b/h2/y", "g/b/h2", "g/c/h/q/r", "g/c/x/z", "$g/a/h",
          "g/a/h/" + "/".join("w%d" % i for i in range(14)), "f/a/h/q", "g/a/h/q/r/s/t/u"]
    eng, py = _load(emqx, fs)
    _check(eng, py, ts, f"{kids} literal children")
    eng.close()


@pytest.mark.parametrize("shape", ["hash", "terminal", "both", "plus", "all"])
def test_shapes_of_the_only_child(emqx, shape):
    """H with a '#' filter, terminal filters only, both (topics that end at H, n = 3, list both),
    its own '+' child -- and all of them under a root with '#' and '+/#': with the states of
    site/S and its fat half in the same iteration a lane lists more than EMX ids and must flush
    in between."""
    fs = ["site/1/device/7/#", "site/+/device/7/#", "site/+/device/7", "site/1/device/7", "site/1/device/+/#"]
    if shape in ("hash", "both", "all"):
        fs.append("site/+/device/#")
    if shape in ("terminal", "both", "all"):
        fs.append("site/+/device")
    if shape in ("plus", "all"):
        fs += ["site/+/device/+/#", "site/+/device/+", "site/+/device/+/m/#"]
    if shape == "all":
        fs += ["#", "+/#", "site/#", "site/+/#", "site/1/#", "site/1/+/#", "site/1/device/#", "site/1/device"]
    ts = ["site/1/device", "site/2/device", "site/1/device/7", "site/2/device/7", "site/1/device/8",
          "site/1/device/7/m/k", "site/2/device/7/m/k", "site/1/other/7", "site/1", "site",
          "$site/1/device/7", "site/1/device/7/" + "/".join("l%d" % i for i in range(13)),
          "site/1/device/7/m/k/x/y"] * 40  # (a wave's worth of lanes listing at once)
    eng, py = _load(emqx, fs)
    want = _check(eng, py, ts, shape)
    if shape == "all":
        assert max(len(w) for w in want) > 8  # more than EMX ids for one topic
    eng.close()


def test_two_keyed_parents_sharing_a_token(emqx):
    """site/S/device -> D and site/+/device -> D: both edges, only the first, only the second,
    neither (an empty slot in D's home bucket), and, after a delta delete, a tombstone there."""
    fs, both, first, second = [], [], [], []
    for s in range(4):
        for j in range(12):
            d = s * 12 + j
            if j % 4 in (0, 1):
                fs.append(f"site/{s}/device/{d}/#")
            if j % 4 in (0, 2):
                fs.append(f"site/+/device/{d}/#")
            (both if j % 4 == 0 else first if j % 4 == 1 else second if j % 4 == 2 else []).append((s, d))
    ts = [f"site/{s}/device/{d}/m/{k}" for s in range(5) for d in range(50) for k in range(2)]
    eng, py = _load(emqx, fs)
    want = _check(eng, py, ts, "full build")
    n_by = {}
    for w in want:
        n_by[len(w)] = n_by.get(len(w), 0) + 1
    assert n_by.get(2, 0) > 0 and n_by.get(1, 0) > 0 and n_by.get(0, 0) > 0
    # tombstones: one edge of a pair goes, then the other, then one comes back
    s, d = both[0]
    _step(eng, py, ts, "first edge deleted", delete=[f"site/{s}/device/{d}/#"])
    s2, d2 = both[1]
    _step(eng, py, ts, "second edge deleted", delete=[f"site/+/device/{d2}/#"])
    _step(eng, py, ts, "both edges deleted", delete=[f"site/+/device/{d}/#"])
    _step(eng, py, ts, "an edge into a tombstone", add=[f"site/{s}/device/{d}/#"])
    assert eng.stats()["delta_commits"] >= 4
    eng.close()


def test_delta_commits_follow_the_only_child(emqx):
    """Each commit is seen by the next match: H gains a filter, gains a sibling (the copy goes),
    loses the sibling."""
    rng = random.Random(43)
    filters = _cfg3(rng)
    topics = _cfg3_topics(rng, 600) + ["site/3/ext/5/m1", "site/3/ext", "site/3/device", "site/3/ext/5"]
    eng, py = _load(emqx, filters)
    _check(eng, py, topics, "full build")
    _step(eng, py, topics, "H gains a '#' filter", add=["site/+/device/#"])
    _step(eng, py, topics, "H gains a terminal filter", add=["site/+/device"])
    _step(eng, py, topics, "H gains a '+' child", add=["site/+/device/+/m1"])
    _step(eng, py, topics, "H gains a sibling", add=["site/+/ext/+/m1"])
    _step(eng, py, topics, "H loses the sibling", delete=["site/+/ext/+/m1"])
    _step(eng, py, topics, "H loses its '#' filter", delete=["site/+/device/#"])
    assert eng.stats()["delta_commits"] >= 6
    eng.close()
