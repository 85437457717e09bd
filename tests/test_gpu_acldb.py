"""GPU parity of the built-in authorization database (emqx_amd.AclDb over emqxgm_acldb_*,
k_acldb, and the mirror emqx_amd.BuiltinDb; DESIGN.md 6b "Built-in database") against the
reference semantics of tests/acl_ref.py (mnesia_authorize), on the scripts of tests/acldb_cases.py
-- the same ones the CPU gate (tests/test_acldb_dev_host.py) runs the kernel's phases and the host
code on under ASan + UBSan: permission, source and position of the deciding rule per request."""
import json
import os
import random

import numpy as np
import pytest

import acl_cases as AC
import acl_ref as AR
import acldb_cases as DC
import acldb_checks as K

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "authz_mnesia_vectors.json")


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _numbers(rules):
    return [(AC.PERM[p], AC.ACTION[a], f) for p, a, f in rules]


def _key(key):
    return (DC.ALL, b"") if key == "all" else (DC.KIND[key[0]], key[1])


def _refused(emqx, db, clients):
    """The refused calls: each raises (-EINVAL) and leaves the database and what is pending alone."""
    E = emqx.EngineError
    ok = [(1, 1, b"a/b")]
    for kind, rules in ((3, ok), (0, [(2, 1, b"t")]), (0, [(1, 0, b"t")]), (1, [(1, 4, b"t")]),
                        (0, [(1, 3, b"t")] * (DC.MAX_RULES + 1))):
        with pytest.raises(E):
            db.store(kind, b"kk", rules)
    with pytest.raises(E):
        db.store_many([(0, b"k", ok), (3, b"k", ok)])
    with pytest.raises(E):
        db.delete(3, b"kk")
    with pytest.raises(E):
        db.match([b"t"], [1], [1], [b"c"], [None])
    with pytest.raises(E):
        db.match([b"t"], [0], [3], [b"c"], [None])
    for key, value in (("no_such_key", 1), ("rebuild_load_pct", 51), ("rebuild_garbage_pct", 0), ("pass_names", 0)):
        with pytest.raises(E):
            db.tune(key, value)


@pytest.fixture
def play(emqx):
    def run(s):
        db = emqx.AclDb(word_hash_bits=s.hash_bits)
        db.tune("counters", 1)
        if s.pass_names:
            db.tune("pass_names", s.pass_names)
        ids = [c["clientid"] for c in s.clients]
        users = [c["username"] for c in s.clients]
        out = []
        for op in s.ops:
            if op[0] == "store":
                db.store(*_key(op[1]), _numbers(op[2]))
            elif op[0] == "many":
                db.store_many([_key(k) + (_numbers(r),) for k, r in op[1]])
            elif op[0] == "delete":
                db.delete(*_key(op[1]))
            elif op[0] == "purge":
                db.purge()
            elif op[0] == "commit":
                db.commit()
            elif op[0] == "tune":
                db.tune(op[1], op[2])
            elif op[0] == "refused":
                _refused(emqx, db, s.clients)
            else:
                reqs = op[1]
                perm, src, pos = db.match([n for _, _, n in reqs], [c for c, _, _ in reqs],
                                          [AC.ACTION[p] for _, p, _ in reqs], ids, users)
                assert perm.dtype == np.uint32 and perm.shape == src.shape == pos.shape == (len(reqs),)
                rows = [None if int(p) == 0xFFFFFFFF else (int(p), int(q), int(r)) for p, q, r in zip(perm, src, pos)]
                assert all(int(q) == int(r) == 0xFFFFFFFF for p, q, r in zip(perm, src, pos) if int(p) == 0xFFFFFFFF)
                out.append((rows, db.stats(), db.count()))
        db.close()
        return out
    return run


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_key_lengths_and_filter_forms(play, hash_bits):
    K.check_keys(play, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_source_order_and_empty_records(play, hash_bits):
    K.check_order(play, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_random_case(play, hash_bits):
    K.check_random(play, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_depth(play, hash_bits):
    K.check_depth(play, hash_bits)


def test_run_sizes(play):
    """Runs of 1, 300 and 65,536 rules; 65,537 are refused (the update script's refused calls)."""
    K.check_runs(play, 0)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_all_tiles(play, hash_bits):
    K.check_tiling(play, hash_bits)


def test_empty_all_record(play):
    K.check_empty_all(play)


def test_all_record_edited_repeatedly(play):
    K.check_all_edits(play)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_table_shapes(play, hash_bits):
    K.check_shapes(play, hash_bits)


@pytest.mark.parametrize("n", DC.BATCH_SIZES)
def test_block_edges(play, n):
    K.check_block(play, n)


def test_passes(play):
    K.check_passes(play)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_update_script(play, hash_bits):
    K.check_update(play, hash_bits, exact_alloc=False)


def test_golden_vectors_through_the_mirror(emqx):
    """emqx_authz_mnesia_SUITE's topic-rule samples under each key kind, and t_normalize_rules,
    through emqx_amd.BuiltinDb."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    c = doc["client"]
    client = {"clientid": c["clientid"].encode(), "username": c["username"].encode(), "peerhost": tuple(c["peerhost"])}
    db = emqx.BuiltinDb()
    for kind in doc["key_kinds"]:
        who = "all" if kind == "all" else (kind, client[kind])
        for g in doc["groups"]:
            db.purge_rules()
            db.store_rules(who, [(s["permission"], s["action"], t.encode()) for s in g["rules"] for t in s["topics"]])
            db.commit()
            assert db.record_count() == 1
            got = db.authorize([client] * len(g["samples"]), [a for _, a, _ in g["samples"]],
                               [t.encode() for _, _, t in g["samples"]])
            got = [g["no_match"] if m == "nomatch" else m[1] for m in got]
            assert got == [w for w, _, _ in g["samples"]], (kind, g["name"])
    n = doc["normalize_rules"]
    who = AR.term_from_json(n["who"])
    db.purge_rules()
    db.store_rules(who, [AR.term_from_json(r) for r in n["accepted"]["rules"]])
    db.commit()
    want, act, t = n["accepted"]["sample"]
    assert db.authorize([client], [act], [t.encode()]) == [("matched", want)]
    assert db.get_rules(who) == ("ok", [("allow", "publish", b"t")])
    for bad in n["refused"]:
        with pytest.raises(emqx.InvalidRule) as e:
            db.store_rules(who, [AR.term_from_json(r) for r in bad["rules"]])
        assert e.value.reason == bad["error"]
    with pytest.raises(emqx.InvalidRule) as e:
        db.store_rules(who, [("allow", "publish", 7)])
    assert e.value.reason == "invalid_rule_topic"
    assert db.get_rules(who) == ("ok", [("allow", "publish", b"t")])  # a refused store leaves the record
    db.delete_rules(who)
    assert db.get_rules(who) == "not_found" and db.record_count() == 0
    db.close()


def test_same_answers_as_the_acl_list(emqx):
    """The random case through emqx_amd.BuiltinDb and through AclList.from_builtin_db over the same
    records: k_acl is a second witness."""
    s = DC.case("random")
    _, reqs, want, _ = s.queries()[0]
    db = emqx.BuiltinDb()
    db.store_many(s.table.items())
    db.commit()
    clients = [s.clients[c] for c, _, _ in reqs]
    got = db.authorize(clients, [p for _, p, _ in reqs], [n for _, _, n in reqs])
    assert got == [DC.answer(w) for w in want]
    assert db.record_count() == len(s.table)
    lst = emqx.AclList.from_builtin_db(list(s.table.items()))
    assert lst.matches(clients, [p for _, p, _ in reqs], [n for _, _, n in reqs]) == got
    lst.close()
    db.close()


def test_seventy_thousand_keys(emqx):
    """70,000 client-id records of one rule each and four `all` rules: more rules than an ACL list
    holds (emqxgm_acl_set refuses them with -EINVAL before any launch), loaded by one store_many
    and answered from the keyed store."""
    rng = random.Random(70000)
    n_keys = 70000
    table = {("clientid", b"dev-%05d" % i): [(("allow", "deny")[i % 3 == 0], ("publish", "subscribe", "all")[i % 3],
                                              (b"d/${clientid}/#", b"d/+/state", b"eq d/x")[i % 3])]
             for i in range(n_keys)}
    table["all"] = [("deny", "subscribe", b"shared/secret"), ("allow", "all", b"shared/#"), ("deny", "publish", b"d/#"),
                    ("allow", "subscribe", b"u/${username}/+")]
    with pytest.raises(emqx.EngineError, match="-22"):
        emqx.AclList.from_builtin_db(list(table.items()))
    clients = [{"clientid": rng.choice([b"dev-%05d" % rng.randrange(n_keys), b"stranger-%d" % i, None]),
                "username": rng.choice([b"bob", None]), "peerhost": None} for i in range(500)]
    reqs = []
    for _ in range(4007):
        c = rng.randrange(len(clients))
        cid = clients[c]["clientid"] or b"x"
        reqs.append((c, rng.choice(["publish", "subscribe"]),
                     rng.choice([b"d/" + cid + b"/t", b"d/" + cid + b"/state", b"d/x", b"shared/secret", b"shared/x",
                                 b"u/bob/cmd", b"other"])))
    want = [DC.decide(clients[c], p, n, table) for c, p, n in reqs]
    assert {w[1] for w in want if w} == {DC.CLIENTID, DC.ALL} and None in want
    db = emqx.BuiltinDb()
    db.store_many(table.items())
    db.commit()
    assert db.record_count() == n_keys + 1
    got = db.authorize([clients[c] for c, _, _ in reqs], [p for _, p, _ in reqs], [n for _, _, n in reqs])
    assert got == [DC.answer(w) for w in want]
    perm, src, pos = db.db.match([n for _, _, n in reqs], [c for c, _, _ in reqs], [AC.ACTION[p] for _, p, _ in reqs],
                                 [c["clientid"] for c in clients], [c["username"] for c in clients])
    assert [None if int(a) == 0xFFFFFFFF else (int(a), int(b), int(c)) for a, b, c in zip(perm, src, pos)] == want
    st = db.db.stats()
    assert st["clientid_records"] == n_keys and st["all_rules"] == 4
    assert st["rebuilds"] == 0 and st["garbage_words"] == 0
    assert st["clientid_deleted"] == 0 and 2 * n_keys <= st["clientid_slots"]
    db.close()
