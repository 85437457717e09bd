"""The reference of the shared-subscription tests on its own (tests/share_ref.py: pick/6 and the
membership rules of apps/emqx/src/emqx_shared_sub.erl on plain Python): the data transcribed from
emqx_shared_sub_SUITE (tests/golden/shared_sub_vectors.json) and every condition the shared inputs
of tests/share_cases.py promise to the CPU gate and the device test.  No library, no GPU."""
import collections
import json
import os
import random

import pytest

import share_cases as SC
import share_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shared_sub_vectors.json")
with open(GOLDEN) as _f:
    CASES = json.load(_f)["cases"]


def _play(case, draws):
    """The case on one SharedSubRef per view; the publisher keeps its round_robin state per key
    (the process dictionary of :367-371).  -> per message the receiver, or None for a sticky
    group (the caller's choice)."""
    views, names = {}, {}
    for v in sorted({m["view"] for m in case["messages"]}):
        ref = views[v] = R.SharedSubRef()
        ref.set_strategy(None, R.STRATEGIES.index(case["default_strategy"]))
        for g, s in case["group_strategy"].items():
            ref.set_strategy(g, R.STRATEGIES.index(s))
        ref.commit()
        for g, t, sub, local in case["subscribe"]:
            ref.subscribe(g, t.encode(), names.setdefault(sub, len(names)), local if isinstance(local, bool) else local[v])
        ref.commit()
    back = {i: n for n, i in names.items()}
    state, out = {}, []
    for m, draw in zip(case["messages"], draws):
        key = (m["view"], m["group"], m["key"])
        sub, status, st, _ = views[m["view"]].pick(m["group"], m["key"].encode(), m["hc"], m["ht"], draw,
                                                   state.get(key, R.NONE))
        state[key] = st
        out.append(back[sub] if status == R.PICKED else None)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"].split(" ")[0] for c in CASES])
def test_suite_vectors(case):
    rng = random.Random(1)
    for _ in range(20):  # whatever the draws are
        got = _play(case, [rng.getrandbits(32) for _ in case["messages"]])
        e = case["expect"]
        if "receivers" in e:
            assert got == e["receivers"]
        for i, j in e.get("equal", []):
            assert got[i] is not None and got[i] == got[j]
        for i, j in e.get("differ", []):
            assert None not in (got[i], got[j]) and got[i] != got[j]
        for i in e.get("host_strategy", []):
            assert got[i] is None


def test_membership_rules():
    ref = R.SharedSubRef()
    for sub in (1, 2, 3):
        ref.subscribe(1, b"t", sub, True)
    ref.subscribe(1, b"t", 2, True)  # already present: keeps its position
    assert ref.subscribers(1, b"t") == []  # pending until the commit
    ref.commit()
    assert [s for s, _ in ref.subscribers(1, b"t")] == [1, 2, 3]
    ref.unsubscribe(1, b"t", 1)
    ref.subscribe(1, b"t", 1, True)  # a later subscribe appends at the end
    ref.commit()
    assert [s for s, _ in ref.subscribers(1, b"t")] == [2, 3, 1]
    for key in ((1, b""), (1, b"+"), (1, b"#"), (1, b"a/#"), (2, b"t"), (1, b"t2")):  # keys like any other
        ref.subscribe(key[0], key[1], 9, False)
    ref.commit()
    assert ref.subscribers(2, b"t") == [(9, False)] and len(ref.subscribers(1, b"t")) == 3
    assert ref.subscribers(1, b"") == [(9, False)] and ref.subscribers(1, b"a/+") == []
    ref.subscriber_down(9)
    ref.commit()
    assert (1, b"") not in ref.bag and (2, b"t") not in ref.bag  # an emptied key is absent
    assert ref.pick(2, b"t", 0, 0, 0, 5) == (R.NONE, R.NO_SUBSCRIBERS, 5, 0)


def test_pick_table():
    ref = R.SharedSubRef()
    for g in range(7):
        ref.set_strategy(g, g)
        for sub, local in ((10, False), (11, True), (12, False), (13, True)):
            ref.subscribe(g, b"k", sub, local)
        ref.subscribe(g, b"one", 20, False)
    ref.commit()
    assert ref.pick(R.RANDOM, b"k", 1, 2, 7, R.NONE) == (13, R.PICKED, R.NONE, 4)
    assert ref.pick(R.HASH_CLIENTID, b"k", 6, 1, 1, R.NONE)[0] == 12
    assert ref.pick(R.HASH_TOPIC, b"k", 1, 5, 1, R.NONE)[0] == 11
    assert ref.pick(R.LOCAL, b"k", 0, 0, 3, R.NONE)[0] == 13  # the local members in order: 11, 13
    assert ref.pick(R.ROUND_ROBIN, b"k", 0, 0, 6, R.NONE) == (12, R.PICKED, 2, 4)
    assert ref.pick(R.ROUND_ROBIN, b"k", 0, 0, 6, 3) == (10, R.PICKED, 0, 4)
    assert ref.pick(R.ROUND_ROBIN, b"k", 0, 0, 6, 9) == (12, R.PICKED, 2, 4)  # a state left by a larger group
    assert [ref.pick(R.RR_PER_GROUP, b"k", 0, 0, 0, 1)[0] for _ in range(5)] == [10, 11, 12, 13, 10]
    assert ref.pick(R.STICKY, b"k", 0, 0, 0, R.NONE) == (R.NONE, R.HOST_STRATEGY, R.NONE, 4)
    for g in set(range(7)) - {R.STICKY}:  # one member: before any strategy, nothing read or written
        assert ref.pick(g, b"one", 5, 5, 5, 3) == (20, R.PICKED, 3, 1)
    assert ref.counter(R.RR_PER_GROUP, b"one") == 0 and ref.counter(R.RR_PER_GROUP, b"k") == 1


def test_random_case_conditions():
    script = SC.random_case()
    ref = R.SharedSubRef()
    for op in script:
        if op[0] == "S":
            ref.subscribe(*op[1:])
        elif op[0] == "G":
            ref.set_strategy(op[1], op[2])
        elif op[0] == "C":
            ref.commit()
    q = next(op[1] for op in script if op[0] == "Q")
    assert len(q) == 4007 and len(ref.bag) == 300
    multi = [r for r in q if len(ref.subscribers(r[0], r[1])) >= 2]
    assert 2 * len(multi) >= len(q)
    decided = collections.Counter(ref.strategy(r[0]) for r in multi)
    for s in R.DEVICE_DECIDED:
        assert decided[s] >= 200, (R.STRATEGIES[s], decided[s])
    none = sum(1 for r in q if not ref.subscribers(r[0], r[1]))
    assert 0.05 * len(q) <= none <= 0.25 * len(q)
    # hash_bits = 4 leaves 16 tags: of any 17 stored keys two share a tag, and the one that lies
    # later in their chain is reached only past the other's slot, whose tag matches and whose
    # bytes or group differ.  The requests ask for far more than 17 stored keys.
    assert len({(r[0], r[1]) for r in q if ref.subscribers(r[0], r[1])}) > 16 * 8


def test_script_conditions():
    """What the other shared scripts promise."""
    sizes = collections.Counter()
    for op in SC.strategy_script():
        if op[0] == "S":
            sizes[(op[1], op[2])] += 1
    assert {n for n in sizes.values()} == set(SC.SIZES) - {0}
    assert len(sizes) == 7 * (len(SC.SIZES) - 1) * len(SC.MIXES)
    down = [op for op in SC.mutation_script() if op[0] == "S" and op[3] == 2]
    assert len({(op[1], op[2]) for op in down}) >= 40  # subscriber_down of a member of 40 keys
    lens = {len(op[2]) for op in SC.topic_script() if op[0] == "S"}
    assert set(SC.TOPIC_LENGTHS) <= lens
    assert len(next(op[1] for op in SC.random_case() if op[0] == "Q")) // 287 + 1 == 14
