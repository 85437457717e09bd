"""The reference side of the built-in database's tests, with no device and no project code:
tests/acl_ref.py's mnesia_authorize against the vectors transcribed from the reference's own suite
(tests/golden/authz_mnesia_vectors.json), and every condition that the shared inputs of
tests/acldb_cases.py promise, asserted on the reference alone."""
import collections
import json
import os

import pytest

import acl_cases as AC
import acl_ref as AR
import acldb_cases as DC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "authz_mnesia_vectors.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_table(group, kind, client):
    """setup_client_samples/3 (emqx_authz_mnesia_SUITE.erl:141-161)."""
    rules = [(s["permission"], s["action"], t.encode()) for s in group["rules"] for t in s["topics"]]
    return {"all" if kind == "all" else (kind, client[kind]): rules}


def golden_client(doc):
    c = doc["client"]
    return {"clientid": c["clientid"].encode(), "username": c["username"].encode(), "peerhost": tuple(c["peerhost"])}


def test_golden_vectors_shape(golden):
    assert golden["key_kinds"] == ["username", "clientid", "all"]
    assert [g["name"] for g in golden["groups"]] == ["no_topic_rules", "allow_topic_rules", "deny_topic_rules"]
    assert [len(g["samples"]) for g in golden["groups"]] == [3, 37, 37]
    assert [g["no_match"] for g in golden["groups"]] == ["deny", "deny", "allow"]


@pytest.mark.parametrize("kind", ["username", "clientid", "all"])
def test_mnesia_authorize_against_golden(golden, kind):
    client = golden_client(golden)
    for g in golden["groups"]:
        table = golden_table(g, kind, client)
        for want, action, topic in g["samples"]:
            m = AR.mnesia_authorize(client, action, topic.encode(), table)
            got = g["no_match"] if m == "nomatch" else m[1]
            assert got == want, (g["name"], kind, action, topic)
            assert DC.answer(DC.decide(client, action, topic.encode(), table)) == m


def test_golden_normalize_rules(golden):
    """t_normalize_rules: a string topic is accepted; the three refused rules are what they are."""
    n = golden["normalize_rules"]
    who = AR.term_from_json(n["who"])
    assert who == ("username", b"username")
    (perm, action, topic), = [AR.term_from_json(r) for r in n["accepted"]["rules"]]
    assert isinstance(topic, str)  # an Erlang string
    client = golden_client(golden)
    want, act, t = n["accepted"]["sample"]
    assert AR.mnesia_authorize(client, act, t.encode(), {who: [(perm, action, AR._bin(topic))]}) == ("matched", want)
    assert [r["error"] for r in n["refused"]] == ["invalid_rule", "invalid_rule_action", "invalid_rule_permission"]
    bad = [AR.term_from_json(r["rules"][0]) for r in n["refused"]]
    assert isinstance(bad[0], list) and bad[1][1] == "pub" and bad[2][0] == "accept"


@pytest.mark.parametrize("name", ["keys", "order", "random", "depth", "runs", "tiling", "shapes", "update"])
def test_decide_is_mnesia_authorize(name):
    """The (permission, source, position) that the device is compared with gives authorize/4's
    answer for every request of every case."""
    s = DC.case(name)
    table = {}
    q = iter(s.queries())
    # replay the script's table: the queries hold the answers of the table committed before them
    t = DC.Script(s.clients)
    for op in s.ops:
        if op[0] == "store":
            t.store(op[1], op[2])
        elif op[0] == "many":
            t.store_many(op[1])
        elif op[0] == "delete":
            t.delete(op[1])
        elif op[0] == "purge":
            t.purge()
        elif op[0] == "commit":
            t.commit()
            table = t.table
        elif op[0] == "query":
            _, reqs, want, _ = next(q)
            if name == "runs":
                reqs, want = reqs[:12], want[:12]  # the 65,536-rule walks are checked once, by decide
            for (c, p, n), w in zip(reqs, want):
                assert DC.answer(w) == AR.mnesia_authorize(s.clients[c], p, n, table)


def test_key_lengths():
    assert [len(k) for k in DC.KEYS[:7]] == [0, 1, 7, 8, 9, 40, 40] and DC.KEYS[5][:-1] == DC.KEYS[6][:-1]
    assert {b"+", b"#", b"a/b", b"${clientid}"} <= set(DC.KEYS)
    t = DC.keys_table()
    for k in DC.KEYS:
        assert t[("clientid", k)] != t[("username", k)]
    # every key decides some request as a client id and as a username, and so does `all`
    s = DC.case("keys")
    _, reqs, want, _ = s.queries()[0]
    seen = {(w[1], AC.CLIENTS[c]["clientid" if w[1] == 0 else "username"]) for (c, _, _), w in zip(reqs, want)
            if w and w[1] < 2}
    assert {(0, k) for k in DC.KEYS} | {(1, k) for k in DC.KEYS} <= seen
    assert any(w and w[1] == 2 for w in want)
    # undefined id, undefined username, both
    undef = {(c["clientid"] is None, c["username"] is None) for c in AC.CLIENTS}
    assert {(True, False), (False, True), (True, True)} <= undef
    # placeholder and eq filters decide in all three kinds
    for src in (0, 1, 2):
        key = lambda c: ("all" if src == 2 else (("clientid", "username")[src], AC.CLIENTS[c][("clientid", "username")[src]]))
        fs = {t[key(c)][w[2]][2] for (c, _, _), w in zip(reqs, want) if w and w[1] == src}
        assert any(b"${" in f and not f.startswith(b"eq ") for f in fs), (src, fs)
        assert any(f.startswith(b"eq ") for f in fs), (src, fs)


def test_source_order():
    s = DC.case("order")
    _, reqs, want, count = s.queries()[0]
    got = dict(zip(reqs, want))
    assert got[(0, "publish", b"x/1")] == (1, DC.CLIENTID, 0)
    assert got[(0, "subscribe", b"x/1")] == (0, DC.USERNAME, 0)   # the client-id rule is for publish
    assert got[(0, "subscribe", b"y/z")] == (1, DC.ALL, 0)
    assert got[(0, "publish", b"q")] is None
    # the same bytes as the other kind of key find nothing
    assert got[(1, "publish", b"x/1")] is None
    # an empty record answers like an absent one, and counts
    assert [got[(2, p, n)] for p in ("publish", "subscribe") for n in (b"x/1", b"y/z", b"q")] == \
           [got[(3, p, n)] for p in ("publish", "subscribe") for n in (b"x/1", b"y/z", b"q")]
    assert count == 4


def test_random_case_outcomes():
    s = DC.case("random")
    _, reqs, want, _ = s.queries()[0]
    assert len(reqs) == 4007
    by = collections.Counter(None if w is None else w[1] for w in want)
    assert min(by[DC.CLIENTID], by[DC.USERNAME], by[DC.ALL], by[None]) >= 50, by
    # at least 50 requests fall through a client-id record that has rules
    fell = sum(1 for (c, _, _), w in zip(reqs, want)
               if (w is None or w[1] != DC.CLIENTID) and s.table.get(("clientid", s.clients[c]["clientid"])))
    assert fell >= 50
    assert {w[0] for w in want if w} == {0, 1}  # both permissions decide


def test_depth_and_sizes():
    _, reqs, _, _ = DC.case("depth").queries()[0]
    assert {16, 17, 40} <= {len(n.split(b"/")) for _, _, n in reqs}
    assert any(len(f.split(b"/")) == 17 for _, _, f in DC.case("depth").table["all"])
    t = DC.case("runs").table
    assert sorted(len(r) for r in t.values()) == [1, 300, 300, DC.MAX_RULES] and "all" not in t
    _, reqs, want, _ = DC.case("runs").queries()[0]
    assert (1, DC.CLIENTID, DC.MAX_RULES - 1) in want and (1, DC.CLIENTID, 299) in want and (1, DC.CLIENTID, 0) in want


def test_all_tiles_layout():
    """The `all` stream of the tiling case: rule 51's record ends at the edge of tile 0, rule 52
    starts tile 1 and decides b/x, the stream has three tiles."""
    compiled = [AR.compile((p, "all", a, [f])) for p, a, f in DC.tiling_rules()]
    pos, total = AC.layout(compiled)
    at = {(r, k): (tile, word, words) for r, k, tile, word, words in pos}
    assert at[(51, 0)] == (0, AC.RS_TILE_WORDS - 2, 2)
    assert at[(52, None)] == (1, 0, 2)
    assert AC.tiles_of(total) == 3
    _, reqs, want, _ = DC.case("tiling").queries()[0]
    got = dict(zip(reqs, want))
    assert got[(4, "publish", b"b/x")] == (1, DC.ALL, 52) and got[(4, "publish", b"/".join([b"a"] * 17))] == (0, DC.ALL, 51)
    assert got[(4, "publish", b"x")] == (1, DC.ALL, 104) and got[(4, "publish", b"/".join([b"f103"] * 16))] == (0, DC.ALL, 103)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_chain_keys(hash_bits):
    ks = DC.chain_keys(hash_bits)
    homes = {DC.home(k, hash_bits, DC.MIN_SLOTS) for k in ks}
    assert len(set(ks)) == 4 and len(homes) == 1 and homes.pop() + 4 > DC.MIN_SLOTS
    if hash_bits:
        assert len({DC.key_token(k, hash_bits) for k in ks}) == 1 and all(len(k) > 7 for k in ks)


def test_update_script_steps():
    s = DC.case("update")
    qs = s.queries()
    assert len(qs) == 12
    assert qs[1][2] == qs[0][2] and qs[1][3] == 3 and qs[0][3] == 0     # stored, not visible, counted
    assert qs[2][2] != qs[1][2] and qs[3][2] == qs[2][2]
    assert qs[4][2] != qs[3][2] and qs[5][2] != qs[4][2] and qs[7][2] != qs[6][2] and qs[8][2] != qs[7][2]
    assert qs[9][2] == qs[8][2] and qs[9][3] == qs[8][3]                # the forced rebuild changes no answer
    assert qs[10][2] == qs[9][2] and qs[10][3] == 1 and qs[11][3] == 1  # the purge waits for its commit
    assert {w[1] for w in qs[11][2] if w} == {DC.USERNAME}
    assert [n for n in DC.BATCH_SIZES] == [0, 1, 255, 256, 257, 513]
