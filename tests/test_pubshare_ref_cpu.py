"""The reference side of the tests of the pick inside the publish, alone: that the cases of
tests/pubshare_cases.py produce, on oracle.emqx_ref.publish and tests/share_ref.py, every kind of
entry the CPU gate (tests/test_pubshare_dev_host.py) and the device test
(tests/test_gpu_pubshare.py) claim to cover.  Without this a case that lost its group entries
would leave those tests comparing empty lists.  No GPU and no library."""
import pytest

import pubshare_cases as PC
import share_cases as SC
import share_ref as SR


def _entries(result):
    return [e for row in result for e in row]


def test_random_case_covers_every_kind():
    script = PC.random_script()
    (res,) = PC.run_ref(script)
    strat = PC.strategy_of(script)
    ents = _entries(res)
    group_ents = [e for e in ents if not isinstance(e[1], str)]
    picked = {strat.get(e[1], strat[None]) for e in group_ents if e[2][1] == SR.PICKED and e[2][3] > 1}
    assert {SR.RANDOM, SR.ROUND_ROBIN, SR.LOCAL, SR.HASH_CLIENTID, SR.HASH_TOPIC} <= picked
    # a single-member key under sticky answers host_strategy like any sticky key
    assert any(e[1] == SR.STICKY and e[2][1] == SR.HOST_STRATEGY and e[2][3] == 1 for e in group_ents)
    assert any(e[1] == SR.STICKY and e[2][1] == SR.HOST_STRATEGY and e[2][3] > 1 for e in group_ents)
    assert any(e[2] == (PC.NONE, SR.NO_SUBSCRIBERS, PC.NONE, 0) for e in group_ents)  # a route with no share key
    hits = {}
    for e in group_ents:
        if e[1] == SR.RR_PER_GROUP and e[2][3] > 1:
            hits.setdefault((e[1], e[0]), []).append(e[2][0])
    assert any(len(set(v)) >= 2 for v in hits.values())  # one counter stepped by several entries
    assert any(e[2] == PC.NOT_SHARED_ANSWER for e in ents) and any(isinstance(e[1], str) for e in ents)
    assert any(not row for row in res) and any(len(row) >= 4 for row in res)
    # round_robin with and without a state that the list carried
    rr = [e for e in group_ents if e[1] == SR.ROUND_ROBIN and e[2][3] > 1]
    assert len({e[2][2] for e in rr}) >= 3
    assert len(group_ents) > 1000


@pytest.mark.parametrize("n", SC.BATCH_SIZES)
@pytest.mark.parametrize("layout", ["spread", "one", "gaps"])
def test_entry_counts(n, layout):
    (res,) = PC.run_ref(PC.count_script(n, layout))
    ents = _entries(res)
    assert len(ents) == n and all(e[2][1] == SR.PICKED and e[2][3] in (2, 5) for e in ents)
    if layout == "one":
        assert len(res) == 1 and len({e[1] for e in ents}) == n
    elif layout == "gaps":
        assert len(res) == 2 * n + 1 and not res[0] and not res[-1] and all(not r for r in res[::2])
    else:
        assert len(res) == n and all(len(r) == 1 for r in res)
    if n > 2:
        assert len({e[2][0] for e in ents}) >= 2


def test_to_lengths():
    (res,) = PC.run_ref(PC.to_length_script())
    lens = {len(e[0]) for e in _entries(res) if e[2][1] == SR.PICKED and e[0] != b"#"}
    assert lens == set(PC.TO_LENGTHS)
    for row in res[:3 * len(PC.TO_LENGTHS)]:  # the To itself and '#', each under both groups
        assert sorted((len(e[0]) > 1 or e[0] != b"#", e[1], e[2][3]) for e in row) == [
            (False, 1, 2), (False, 2, 3), (True, 1, 2), (True, 2, 3)] or len(row[0][0]) == 1
    assert all(e[0] == b"#" for row in res[-6:] for e in row) and all(len(row) == 2 for row in res[-6:])
    assert not any(e[2][0] in (900, 901, 902) for e in _entries(res))


def test_strategies():
    script = PC.strategy_script()
    (res,) = PC.run_ref(script)
    ents = _entries(res)
    assert all(len(r) == 1 for r in res)
    for strat in range(7):
        mine = [e for e in ents if e[1] == strat]
        counts = {e[2][3] for e in mine}
        assert counts == set(SC.SIZES)
        want = SR.HOST_STRATEGY if strat == SR.STICKY else SR.PICKED
        assert all(e[2][1] == (SR.NO_SUBSCRIBERS if e[2][3] == 0 else want) for e in mine)
    rr = [e[2] for e in ents if e[1] == SR.ROUND_ROBIN and e[2][3] == 7]
    # states 0, 5, 6, 12 step to 1, 6, 0 (the wrap), 6; state 3 to 4; undefined draws 0, 6, 7,
    # 2^27 - 1 and 2^32 - 1 rem 7 = 0, 6, 0, 0, 3
    assert {q[2] for q in rr} == {0, 1, 3, 4, 6}


def test_state_lists():
    first, second = PC.run_ref(PC.state_script())
    assert all(e[1] == "n2" for row in first for e in row if e[0] == b"st/+")  # a node entry beside each
    q = [next((e[2] for e in row if e[1] == 4), None) for row in first]  # group 4's entry of each topic
    # empty list: drawn (7 rem 5); the pair: 2 -> 3, alone and after 40 others; another filter's
    # pair, a To that is no filter and another group's pair: drawn; twice: the first (1 -> 2)
    assert [x[2] for x in q[:7]] == [2, 3, 3, 2, 2, 2, 2]
    assert [x[2] for x in q[7:12]] == [2, 1, 0, 1, (2 ** 32 - 1) % 5]  # NONE, 0, Count-1, Count, 2^32-2
    assert q[12][2] == 0 and first[13] == []
    assert all([e[2][2] for e in row if e[1] == 4] == [9 % 5] for row in second)


def test_round_robin_per_group_consecutive():
    a, b = PC.run_ref(PC.rr_group_script())
    got = [e[2][0] for row in a for e in row if e[1] == 2 and e[0] == b"rr/+"]
    assert len(got) > 400 and got == [1 + i % 3 for i in range(len(got))]
    got3 = [e[2][0] for row in a for e in row if e[1] == 2 and e[0] == b"rr/3"]
    assert got3 == [11 + i % 2 for i in range(len(got3))] and len(got3) > 100
    nxt = [e[2][0] for row in b for e in row if e[1] == 2 and e[0] == b"rr/+"]
    assert nxt[0] == 1 + len(got) % 3
    assert any(not row for row in a) and any(e[2] == PC.NOT_SHARED_ANSWER for row in a for e in row)


def test_mutations():
    r = PC.run_ref(PC.mutation_script())
    pick = lambda res, i, to: [e[2] for e in res[i] if e[0] == to and e[1] == 1]
    assert pick(r[0], 0, b"m/a") == [(1, 0, PC.NONE, 2)] and pick(r[0], 2, b"m/a") == [(2, 0, PC.NONE, 2)]
    assert r[1] == r[0]                                         # pending mutations are invisible
    assert pick(r[2], 0, b"m/a") == [(2, 0, PC.NONE, 2)] and pick(r[2], 2, b"m/a") == [(4, 0, PC.NONE, 2)]
    assert pick(r[3], 0, b"m/a") == [] and pick(r[3], 0, b"m/+") == [(3, 0, PC.NONE, 1)]
    assert pick(r[4], 0, b"m/+") == [(PC.NONE, SR.NO_SUBSCRIBERS, PC.NONE, 0)] and len(pick(r[4], 0, b"m/a")) == 1
    for res in r:  # m/x: members but no group route -- the node entry and m/+'s, never (1, m/x)
        assert [e[1] for e in res[1] if e[0] == b"m/x"] == ["n1"]
        assert not any(e[2][0] in (7, 8) for row in res for e in row)


def test_text_round_trip():
    """The CPU gate's input names every entry of the reference's fan-out, in its order."""
    script = PC.random_script()
    text = PC.input_text(script, 4, 100)
    (res,) = PC.run_ref(script)
    head = [ln for ln in text.splitlines() if ln.startswith("P ")]
    assert len(head) == 1 and head[0].startswith("P 700 ") and head[0].endswith(" 1")
    body = text.splitlines()[text.splitlines().index(head[0]) + 2:-1]
    assert [int(ln.split()[3]) for ln in body] == [len(row) for row in res]
