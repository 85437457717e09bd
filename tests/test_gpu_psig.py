"""Lent signatures on the device (gm_common.h "Lent signatures", gm_walk.inc create): a state D
without literal children lends its slot's signature field to its '+' child, and the walk, which
creates that child's state without a probe, drops the literal probe under it when the next
word's class bit is clear.

A cfg3-shaped trie (workloads/gen.cpp gen_cfg3 at 4 sites x 8 devices: its five patterns, k in
0..15) is matched against the Python restatement of emqx_trie (oracle/emqx_ref.py) with the rule
on and off (tune "plus_sig"), with and without fat buckets, and after every step of a delta
churn of the device states; the census counts the level-5 literal probes the rule removes.

Which kernel a row check runs matters here: the one-lane-per-topic walk holds the filter, the
pair walk is compiled without it (gm_walk.inc create's LENT), and batches as small as these
take the pair walk by default.  Every row check therefore runs with tune "walk_pair" 0 (one
lane per topic: the filter), 1 (the default choice) and 2 (every batch through the pair walk,
which must be unaffected by the lent bits in the slots it reads).

A last case runs a topic whose rank passes the packed staging's rank field."""
import random

import pytest

import walk_rule_cases as W

pytestmark = pytest.mark.gpu

SITES, DEVS, KS = 4, 8, 16


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def sig_bit(word: bytes) -> int:
    """gm_common.h sig_bit of a word of at most 7 bytes (its level token is its bytes, packed)."""
    assert len(word) <= 7
    tok = int.from_bytes(word, "little") | (len(word) << 56)
    return 1 << (((((tok * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> 32) * 6) >> 32)


def _dev(s, j):
    return s * DEVS + j  # global device ids, some of them site numbers too (as on cfg3)


def _filters(rng):
    fs = set()
    for s in range(SITES):
        for j in range(DEVS):
            d = _dev(s, j)
            if j != 5:
                fs.add(f"site/{s}/device/{d}/#")
            if rng.random() < 0.5:
                fs.add(f"site/+/device/{d}/#")
            # device 4 of a site: no D/+/k at all; device 5: only D/+/k
            if j != 4:
                for k in range(KS):
                    if rng.random() < 0.25 or k == j:
                        fs.add(f"site/{s}/device/{d}/+/{k}")
        for m in range(8):
            if rng.random() < 0.6:
                fs.add(f"site/{s}/device/+/m{m}")
            if rng.random() < 0.4:
                fs.add(f"site/{s}/+/+/m{m}")
    return sorted(f.encode() for f in fs)


def _topics():
    ts = [f"site/{s}/device/{_dev(s, j)}/m{m}/{k}"
          for s in range(SITES) for j in range(DEVS) for m in range(2) for k in range(KS)]
    assert len(ts) == 1024
    for s in range(SITES):
        for j in (0, 4, 5, 6, 7):
            p = f"site/{s}/device/{_dev(s, j)}"
            ts += [p + "/m1", p + "/m1/3/x", p + "/m1/3/x/y",  # 5, 7 and 8 levels
                   p + "/only/q/7", p + "/only/q/9", p + "/lit/x", p + "/a/z", p + "/other",
                   p + "/m0/q7", p + "/m0/q8", p + "/m0/q9", p + "/m0/q10", p + "/m0/q11", p + "/m0/q12"]
    ts += ["$site/0/device/0/m1/3", "$SYS/x", "site/+/device/0/m1/3", "site/0/device/0/m1/#", "site"]
    return [t.encode() for t in ts]


def _check(eng, py, topics, what=""):
    """Rows equal the oracle's with the rule on and off, through the one-lane walk (walk_pair 0:
    the kernel with the filter), the default choice (1) and the pair walk (2)."""
    W.check(eng, py, topics, what, ("plus_sig",))


def _load(emqx, filters, bits=0, keyed=1, fat=1):
    return W.load(emqx, filters, bits=bits, keyed=keyed, fat=fat)


def _level5(eng, topics):
    """Literal probes of level 5 (the k of site/S/device/D/m/k) of one census pass."""
    return W.census(eng, topics)["loads_by_level"]["literal"][5]


@pytest.mark.parametrize("fat", [1, 0])
def test_rows_and_level5_probes(emqx, fat):
    """Rows with the rule on and off through every walk (_check), and the census (a one-lane
    walk, so it has the filter whatever the production pass runs): turning the rule on removes at least one
    level-5 literal load for every (topic, D) whose D/+ has literal children none of which is of
    the class of the topic's k (R, from the filters), and keeps at least one for every topic
    whose D/+/k exists.  Inequalities: collision chains add loads on both sides."""
    rng = random.Random(5)
    filters = _filters(rng)
    assert 200 <= len(filters) <= 600
    topics = _topics()
    eng, py = _load(emqx, filters, fat=fat)
    _check(eng, py, topics, "full build")
    kids = {}  # (s, d) -> the k's of site/s/device/d/+/k
    for f in filters:
        w = f.decode().split("/")
        if len(w) == 6 and w[2] == "device" and w[3] != "+" and w[4] == "+":
            kids.setdefault((w[1], w[3]), set()).add(w[5])
    absent = exists = 0
    for t in topics[:1024]:
        w = t.decode().split("/")
        ks = kids.get((w[1], w[3]))
        if not ks:
            continue
        lent = 0
        for k in ks:
            lent |= sig_bit(k.encode())
        absent += 0 if lent & sig_bit(w[5].encode()) else 1
        exists += 1 if w[5] in ks else 0
    assert absent > 100 and exists > 100  # (the trie exercises both sides)
    eng.tune("plus_sig", 1)
    on = _level5(eng, topics)
    eng.tune("plus_sig", 0)
    off = _level5(eng, topics)
    eng.tune("plus_sig", 1)
    print(f"level-5 literal loads: off {off} on {on}; class bit absent {absent}, D/+/k exists {exists}")
    assert off - on >= absent
    assert on >= exists
    eng.close()


@pytest.mark.parametrize("bits,keyed", [(0, 2), (0, 1), (3, 2)])
def test_delta_churn_of_device_states(emqx, bits, keyed):
    """Every delta step that changes a lent signature or whose slot holds one, rows checked with
    the rule on and off through every walk after each commit (_check): a newly added D/+/k must
    match at once in the one-lane walk, which filters by the patched bits."""
    rng = random.Random(9)
    filters = _filters(rng)
    s6, s7 = f"site/1/device/{_dev(1, 6)}", f"site/2/device/{_dev(2, 7)}"
    # a parent with literal children beside its '+' child (keyed at "keyed" 2), a fat node
    filters += [f.encode() for f in (s6 + "/a/z", s6 + "/b/z", s6 + "/+/5", s6 + "/+/11", s7 + "/only/+/7")]
    filters = sorted(set(filters))
    topics = _topics()
    eng, py = _load(emqx, filters, bits=bits, keyed=keyed)
    _check(eng, py, topics, "full build")

    def step(what, add=(), delete=()):
        for f in delete:
            eng.trie_delete(f.encode())
            py.delete(f.encode())
        for f in add:
            eng.trie_insert(f.encode())
            py.insert(f.encode())
        eng.commit()
        _check(eng, py, topics, what)

    d0 = f"site/0/device/{_dev(0, 0)}"
    have = 0
    for f in filters:
        if f.decode().startswith(d0 + "/+/"):
            have |= sig_bit(f.decode().split("/")[5].encode())
    new = [w for w in ("q7", "q8", "q9", "q10", "q11", "q12") if not have & sig_bit(w.encode())]
    assert new, "no probe word of a class that D/+ does not have yet"
    step("literal child under D/+", add=[d0 + "/+/" + new[0]])
    step("literal child under D/+ deleted", delete=[d0 + "/+/" + new[0]])
    d1 = f"site/0/device/{_dev(0, 5)}"
    step("first literal child", add=[d1 + "/lit/x"])
    step("last literal child deleted", delete=[d1 + "/lit/x"])
    d4 = f"site/0/device/{_dev(0, 4)}"
    step("'+' child added", add=[d4 + "/+/3"])
    step("'+' child deleted", delete=[d4 + "/+/3"])
    step("'+' child added again", add=[d4 + "/+/4"])
    step("keyed parent without literal children", delete=[s6 + "/a/z", s6 + "/b/z"])
    step("keyed parent with a literal child again", add=[s6 + "/a/z"])
    step("literal child under a half's '+' child", add=[s7 + "/only/+/9"])
    step("the half moves out", add=[s7 + "/other"])
    if bits == 0:
        assert eng.stats()["delta_commits"] >= 11
    eng.close()


def test_root_lends(emqx):
    """A root without literal children whose '+' child has some: the root's signature lends."""
    eng, py = _load(emqx, [b"+/a", b"+/b/#", b"+/+/c", b"+/a/+/d", b"#"])
    topics = [b"x/a", b"x/q", b"x/b/y", b"x/y/c", b"$x/a", b"x", b"x/a/y/d", b"x/zz", b"lit/q", b"lit/a",
              b"+/a", b"x/a/y/e"]
    _check(eng, py, topics, "root build")
    for what, add, delete in (("literal child under the root's '+' child", b"+/zz", None),
                              ("the root's first literal child", b"lit/q", None),
                              ("the root's last literal child deleted", None, b"lit/q")):
        if add:
            eng.trie_insert(add)
            py.insert(add)
        if delete:
            eng.trie_delete(delete)
            py.delete(delete)
        eng.commit()
        _check(eng, py, topics, what)
    eng.close()


@pytest.mark.parametrize("pair", [1, 0])
def test_rank_past_the_packed_field_is_masked(emqx, pair):
    """One topic with 11 matches and a 3-bit rank field (tune "stage_rank_bits"): the packed pass
    overflows and is redone wide; the redone rows equal the oracle's and no id at or above the
    filter count appears.  This guards the overflow-and-redo path through both walks, not the
    mask in put() itself: the packed words of the overflowed pass, where a rank past the field
    is masked instead of carried into the filter id, are discarded before any row is read."""
    filters = [b"#", b"+/#", b"a/#", b"a/+/#", b"a/b/#", b"a/b/c", b"+/b/c", b"a/+/c", b"+/+/c", b"a/b/+",
               b"+/+/+", b"a/b/d", b"x/y"]
    eng, py = _load(emqx, filters)
    eng.tune("walk_pair", pair)
    eng.tune("stage_rank_bits", 3)
    want = sorted(py.match(b"a/b/c"))
    assert len(want) >= 9
    r0 = eng.stats()["reruns"]
    res = eng.match([b"a/b/c"])
    assert eng.stats()["reruns"] == r0 + 1  # packed, overflowed, redone wide
    assert int(res.filter_id.max()) < len(filters)
    assert sorted(eng.filter_bytes(int(f)) for f in res.row(0)) == want
    eng.tune("stage_rank_bits", 0)
    eng.close()
