"""ACL rule lists (DESIGN.md 6b "ACL lists") on the CPU, the reference side:

1. tests/acl_ref.py (emqx_authz_rule restated on the oracle) and emqx_amd.authz.compile reproduce
   the five sources and every assertion of t_compile and t_match of the reference's
   emqx_authz_rule_SUITE (tests/golden/authz_rule_vectors.json);
2. every condition that tests/acl_cases.py promises of its inputs holds on acl_ref alone, so a
   case cannot pass on the device without reaching its branch;
3. the global list of the built-in database answers as emqx_authz_mnesia:authorize/4 restated.
"""
import json
import os

import pytest

import acl_cases as AC
import acl_ref as AR
import ruleset_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "authz_rule_vectors.json")) as f:
        return json.load(f)


def test_golden_compile(golden):
    from emqx_amd import authz
    assert sorted(golden["sources"]) == ["SOURCE%d" % i for i in range(1, 6)] == sorted(golden["t_compile"])
    for name, src in golden["sources"].items():
        want = golden["t_compile"][name]
        assert AR.term_json(AR.compile(AR.term_from_json(src))) == want, name
        assert AR.term_json(authz.compile(AR.term_from_json(src))) == want, name


def test_golden_match(golden):
    from emqx_amd import authz
    assert len(golden["t_match"]) == 19
    for v in golden["t_match"]:
        c = golden["clients"][v["client"]]
        client = {"clientid": c["clientid"].encode(), "username": c["username"].encode(),
                  "peerhost": tuple(c["peerhost"])}
        src = AR.term_from_json(golden["sources"][v["source"]])
        want = v["result"] if v["result"] == "nomatch" else tuple(v["result"])
        assert AR.match(client, v["pubsub"], v["topic"].encode(), AR.compile(src)) == want, v
        # the product mirror's host half: compile and match_who agree on every principal
        assert authz.match_who(client, authz.compile(src)[1]) == AR.match_who(client, AR.compile(src)[1]), v


def test_compile_forms_agree():
    """emqx_amd.authz.compile and the restatement on every source rule of the cases."""
    from emqx_amd import authz
    rules = [r for n in AC.LIST_SIZES for r in AC.random_case(n)[0]]
    rules += AC.values_case()[0] + AC.order_case()[0] + AC.depth_case()[0] + AC.slots_rules(3)
    for r in rules:
        assert AR.term_json(authz.compile(r)) == AR.term_json(AR.compile(r)), r
    # and the list the mirror would upload is the one the gate and the GPU test upload
    src = AC.random_case(130)[0]
    al = authz.AclList.__new__(authz.AclList)
    al.rules, al.slots = [authz.compile(r) for r in src], []
    flat = AC.flatten([AR.compile(r) for r in src])
    assert tuple(al._plan()) == flat[:8]
    assert [AR.term_json(w) for w in al.slots] == [AR.term_json(w) for w in flat[8]]


@pytest.mark.parametrize("n_rules", AC.LIST_SIZES)
def test_random_case_conditions(n_rules):
    (rules, clients, reqs), compiled, first, res = AC.random_reference(n_rules)
    assert len(rules) == n_rules and len(reqs) == 4007
    assert [n for _, _, n in reqs[-len(RR.EDGE_NAMES):]] == RR.EDGE_NAMES
    assert {r[0] for r in rules} == {"allow", "deny"} and {r[2] for r in rules} == {"publish", "subscribe", "all"}
    assert set(AC.flatten(compiled)[5]) == {AC.WHO_ALL, AC.WHO_USERNAME, AC.WHO_CLIENTID, AC.WHO_HOST}
    assert {len(r[3]) for r in rules} == {0, 1, 2, 3, 4}
    fs = [f for r in compiled for f in r[3]]
    assert any(isinstance(f, tuple) and f[0] == "pattern" for f in fs)
    assert any(isinstance(f, tuple) and f[0] == "eq" for f in fs)
    for outcome in ("nomatch", ("matched", "allow"), ("matched", "deny")):
        assert res.count(outcome) >= 0.1 * len(reqs), outcome
    # with 4 bits of hash an unconfirmed token match answers some request differently
    unc = [AC.unconfirmed_first(clients[c], p, t, compiled) for c, p, t in reqs]
    assert sum(1 for a, b in zip(unc, first) if a != b) >= 1


def test_client_table_conditions():
    ids = [c["clientid"] for c in AC.CLIENTS]
    users = [c["username"] for c in AC.CLIENTS]
    for col in (ids, users):
        assert {len(v) for v in col if v is not None} >= {1, 7, 8, 9, 40}
        for v in (b"", b"+", b"#", b"a/b", b"${clientid}", b"$s", AC.ID40A, AC.ID40B):
            assert v in col
    assert any(c["clientid"] is None and c["username"] is not None for c in AC.CLIENTS)
    assert any(c["clientid"] is not None and c["username"] is None for c in AC.CLIENTS)
    assert any(c["clientid"] is None and c["username"] is None for c in AC.CLIENTS)
    (rules, clients, reqs), compiled, first, res = AC.reference("values")
    names = {n for _, _, n in reqs}
    for v in AC.VALUES:
        assert b"c/" + v in names and v in names
    by = {(c, p, n): r for (c, p, n), r in zip(reqs, first)}
    cid = {v: i for i, v in enumerate(ids) if v is not None}
    # a value that equals no name word matches nothing, a plain one matches its own word
    for v in (b"", b"+", b"#", b"a/b"):
        assert by[(cid[v], "subscribe", b"c/" + v)] is None and by[(cid[v], "subscribe", v)] != 0
    for v in (b"a", b"sevenby", b"eightbyt", b"ninebytes", AC.ID40A, AC.ID40B, b"${clientid}", b"$s"):
        assert by[(cid[v], "subscribe", b"c/" + v)] == 0 and by[(cid[v], "subscribe", v)] == 0
    assert by[(cid[AC.ID40A], "subscribe", b"c/" + AC.ID40B)] is None
    # undefined: the placeholder stays a literal word
    undef = next(i for i, c in enumerate(AC.CLIENTS) if c["clientid"] is None and c["username"] is None)
    assert by[(undef, "subscribe", b"c/${clientid}")] == 0 and by[(undef, "publish", b"u/${username}/x")] == 1
    assert by[(undef, "subscribe", b"c/a")] is None
    # an eq filter keeps the placeholder literal for everybody
    assert by[(cid[b"a"], "publish", b"${clientid}")] == 1 and by[(cid[b"a"], "publish", b"c/${username}")] == 2


def test_order_conditions():
    (rules, clients, reqs), compiled, first, res = AC.reference("order")
    by = {(c, p, n): r for (c, p, n), r in zip(reqs, first)}
    assert by[(0, "publish", b"o/deny/x")] == 0 and AR.match(clients[0], "publish", b"o/deny/x", compiled[1]) != "nomatch"
    assert by[(0, "publish", b"p/x")] == 3 and by[(0, "subscribe", b"p/x")] == 2
    assert by[(0, "publish", b"w/x")] == 5 and by[(1, "publish", b"w/x")] == 4
    assert by[(0, "publish", b"s/x/second")] == 6 and by[(0, "publish", b"s/x")] is None
    assert by[(0, "publish", b"nothing")] is None


def test_slot_conditions():
    (rules, clients, reqs), compiled, first, res = AC.reference("slots")
    flat = AC.flatten(compiled)
    assert flat[5] == [AC.WHO_HOST] * 64 and flat[6] == list(range(64)) and len(flat[8]) == 64
    assert first == [0, 31, 32, 63, None]
    assert AC.table_args(clients, flat[8])[3] == [1 << 0, 1 << 31, 1 << 32, 1 << 63, 0]
    with pytest.raises(ValueError):
        AC.flatten([AR.compile(r) for r in AC.slots_rules(65)])
    from emqx_amd import authz
    with pytest.raises(ValueError):
        authz.AclList(AC.slots_rules(65))  # refused before anything touches the device


def test_tiling_conditions():
    (rules, clients, reqs), compiled, first, res = AC.reference("tiling")
    pos, total = AC.layout(compiled)
    at = {(r, k): (tile, word, words) for r, k, tile, word, words in pos}
    # rule 51's header is the last record of tile 0, its first filter is word 0 of tile 1
    assert at[(51, None)] == (0, 1020, 2) and at[(51, 0)] == (1, 0, 3)
    # rule 102's two matching filters lie either side of the edge between tiles 1 and 2
    assert at[(102, 1)] == (1, 1020, 4) and at[(102, 2)] == (2, 0, 3) and AC.tiles_of(total) == 3
    by = {(c, n): r for (c, p, n), r in zip(reqs, first)}
    assert by[(4, b"a/b")] == 51 and by[(4, b"a")] == 51
    assert by[(4, b"b/x")] == 102 and by[(4, b"b")] == 102 and by[(5, b"b/x")] == 103
    c4 = clients[4]
    assert AR.match_topics(c4, b"b/x", compiled[102][3][1:2]) and AR.match_topics(c4, b"b/x", compiled[102][3][2:])
    assert not AR.match_topics(c4, b"b", compiled[102][3][1:2]) and AR.match_topics(c4, b"b", compiled[102][3][2:])
    assert by[(4, b"/".join([b"f7"] * 16))] == 7 and by[(4, b"x")] == 103


def test_depth_conditions():
    (rules, clients, reqs), compiled, first, res = AC.reference("depth")
    depths = {len(n.split(b"/")) for _, _, n in reqs}
    assert depths >= {16, 17, 40}
    fdepths = {len(f[1] if isinstance(f, tuple) else f) for r in compiled for f in r[3]}
    assert fdepths >= {16, 17, 40}
    pat = compiled[0][3][0]
    assert pat[0] == "pattern" and len(pat[1]) == 17 and pat[1][16] == AR.PH_CLIENTID
    assert set(first) == {0, 1, 2, 3, None}
    ids = [c["clientid"] for c in clients]
    by = {(c, p, n): r for (c, p, n), r in zip(reqs, first)}
    lv17 = lambda last: b"/".join([b"a"] * 16 + [last])  # noqa: E731
    assert by[(ids.index(AC.ID40A), "subscribe", lv17(AC.ID40A))] == 0
    assert by[(ids.index(AC.ID40B), "subscribe", lv17(AC.ID40A))] != 0
    assert by[(ids.index(b"+"), "subscribe", lv17(b"+"))] == 2  # the eq filter, not the fed "+"


def test_builtin_db_equals_mnesia_authorize():
    from emqx_amd import authz
    table, clients, reqs = AC.builtin_db_case()
    assert len(table) >= 200
    rules = AC.builtin_db_rules(table)
    assert [AR.term_json(authz.compile(r)) for r in authz.AclList.builtin_db_rules(AC.builtin_db_records(table))] == \
        [AR.term_json(AR.compile(r)) for r in rules]
    compiled = [AR.compile(r) for r in rules]
    want = [AR.mnesia_authorize(clients[c], p, n, table) for c, p, n in reqs]
    got = [AR.matches(clients[c], p, n, compiled) for c, p, n in reqs]
    assert got == want
    # the table's last `all` rule denies "#": every request is decided, both ways
    assert set(want) == {("matched", "allow"), ("matched", "deny")}
    assert len(AC.flatten(compiled)[8]) == 0  # one rule per user and no host slot: a fixed record per client
