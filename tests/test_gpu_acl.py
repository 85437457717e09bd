"""GPU parity of ACL rule lists (emqx_amd.Acl over emqxgm_acl_*, k_acl, and the mirror
emqx_amd.AclList; DESIGN.md 6b "ACL lists") against the reference semantics of tests/acl_ref.py,
on the inputs of tests/acl_cases.py -- the same ones the CPU gate (tests/test_acl_dev_host.py)
runs the kernel's phases on under ASan + UBSan."""
import numpy as np
import pytest

import acl_cases as AC
import acl_ref as AR
import ruleset_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _same(reqs, rows, want):
    assert len(rows) == len(reqs)
    bad = [(reqs[i], rows[i], want[i]) for i in range(len(reqs)) if rows[i] != want[i]]
    assert not bad, bad[:5]


def _acl(emqx, compiled, hash_bits=0):
    """(handle with the list set and counters on, the list's host-slot principals)."""
    flat = AC.flatten(compiled)
    acl = emqx.Acl(word_hash_bits=hash_bits)
    acl.tune("counters", 1)
    acl.set(*flat[:8])
    return acl, flat[8]


def _match(acl, exprs, clients, reqs):
    ids, users, _, bits = AC.table_args(clients, exprs)
    out = acl.match([n for _, _, n in reqs], [c for c, _, _ in reqs], [AC.ACTION[p] for _, p, _ in reqs],
                    ids, users, bits)
    assert out.dtype == np.uint32 and out.shape == (len(reqs),)
    return [None if int(r) == 0xFFFFFFFF else int(r) for r in out]


def _run(emqx, compiled, clients, reqs, hash_bits=0):
    acl, exprs = _acl(emqx, compiled, hash_bits)
    rows = _match(acl, exprs, clients, reqs)
    st = acl.stats()
    acl.close()
    return rows, st


@pytest.mark.parametrize("hash_bits", [0, 4])
@pytest.mark.parametrize("n_rules", AC.LIST_SIZES)
def test_random_cases(emqx, n_rules, hash_bits):
    """63 / 64 / 65 / 130 rules of 0..4 filters, every action, permission and who kind, 4,007
    requests ending in the edge names: the first matching rule of every request."""
    (rules, clients, reqs), compiled, first, res = AC.random_reference(n_rules)
    rows, st = _run(emqx, compiled, clients, reqs, hash_bits)
    _same(reqs, rows, first)
    assert st["rules"] == n_rules and st["filters"] == st["records"] == sum(len(r[3]) for r in compiled)
    assert st["deep"] == 2  # the 40- and the 17-level name; the 16-level one is tokenised
    assert st["candidates"] > st["removed"], st
    if hash_bits:
        # 4 bits of hash: different words share tokens; the device's byte check tells them apart
        assert st["removed"] >= 1, st


def test_mirror_on_a_random_list(emqx):
    """emqx_amd.AclList (compile, host slots, client table, permissions) on the 65-rule list."""
    (rules, clients, reqs), compiled, first, res = AC.random_reference(65)
    al = emqx.AclList(rules)
    cs = [clients[c] for c, _, _ in reqs]
    got = al.matches(cs, [p for _, p, _ in reqs], [n for _, _, n in reqs])
    _same(reqs, got, res)
    _same(reqs, al.first_rules(cs, [p for _, p, _ in reqs], [n for _, _, n in reqs]), first)
    assert {"nomatch", ("matched", "allow"), ("matched", "deny")} == set(got)
    al.close()


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_client_values(emqx, hash_bits):
    """Every client value as a word of a name, for every client: "", "+", "#" and "a/b" equal
    no name word, an undefined value leaves the placeholder a literal word."""
    (rules, clients, reqs), compiled, first, res = AC.reference("values")
    rows, st = _run(emqx, compiled, clients, reqs, hash_bits)
    _same(reqs, rows, first)
    assert st["candidates"] >= 1, st  # 40-byte ids and literal placeholders: confirmed on the bytes


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_first_match_order(emqx, hash_bits):
    (rules, clients, reqs), compiled, first, res = AC.reference("order")
    rows, _ = _run(emqx, compiled, clients, reqs, hash_bits)
    _same(reqs, rows, first)


def test_who_slots(emqx):
    """Host slots 0, 31, 32 and 63 decide; slot 64 is refused by set, 65 principals by AclList."""
    (rules, clients, reqs), compiled, first, res = AC.reference("slots")
    assert first == [0, 31, 32, 63, None]
    acl, exprs = _acl(emqx, compiled)
    _same(reqs, _match(acl, exprs, clients, reqs), first)
    flat = list(AC.flatten(compiled)[:8])
    flat[6] = [64] + flat[6][1:]
    with pytest.raises(emqx.EngineError):
        acl.set(*flat)
    _same(reqs, _match(acl, exprs, clients, reqs), first)  # the old list still answers
    acl.close()
    with pytest.raises(ValueError):
        emqx.AclList(AC.slots_rules(65))
    al = emqx.AclList(rules)
    _same(reqs, al.matches([clients[c] for c, _, _ in reqs], ["publish"] * len(reqs), [n for _, _, n in reqs]), res)
    al.close()


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_tiling(emqx, hash_bits):
    """Three tiles: a rule header as the last record of a tile with its first filter at word 0
    of the next, and a rule whose two matching filters lie either side of a tile edge."""
    (rules, clients, reqs), compiled, first, res = AC.reference("tiling")
    pos, total = AC.layout(compiled)
    at = {(r, k): (tile, word) for r, k, tile, word, words in pos}
    assert at[(51, None)] == (0, 1020) and at[(51, 0)] == (1, 0)
    assert at[(102, 1)] == (1, 1020) and at[(102, 2)] == (2, 0) and AC.tiles_of(total) == 3
    rows, st = _run(emqx, compiled, clients, reqs, hash_bits)
    _same(reqs, rows, first)
    assert st["tiles"] == 3 and st["candidates"] >= 1, st


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_depth(emqx, hash_bits):
    """Names and filters of 16, 17 and 40 levels; a 17-level pattern whose placeholder is the
    17th level: everything past 16 levels is matched on the bytes, substitution included."""
    (rules, clients, reqs), compiled, first, res = AC.reference("depth")
    rows, st = _run(emqx, compiled, clients, reqs, hash_bits)
    _same(reqs, rows, first)
    deep = sum(1 for _, _, n in reqs if len(n.split(b"/")) > AC.RS_MAX_LEVELS)
    assert st["deep"] == deep > 0 and st["candidates"] >= deep, st


@pytest.mark.parametrize("n", AC.BATCH_SIZES)
def test_block_edges(emqx, n):
    """0, 1, 255, 256, 257 and 513 requests: the last block's idle lanes reach every barrier."""
    (rules, clients, reqs), compiled, first, res = AC.block_case(n)
    assert len(reqs) == n
    rows, _ = _run(emqx, compiled, clients, reqs)
    _same(reqs, rows, first)


def test_passes(emqx):
    """4,007 requests in 14 passes of 300: the answers and counters of the one-pass call."""
    (rules, clients, reqs), compiled, first, res = AC.random_reference(65)
    assert -(-len(reqs) // AC.PASS_NAMES) == 14
    acl, exprs = _acl(emqx, compiled)
    rows1 = _match(acl, exprs, clients, reqs)
    st1 = acl.stats()
    acl.tune("pass_names", AC.PASS_NAMES)
    rows = _match(acl, exprs, clients, reqs)
    st = acl.stats()
    assert rows == rows1
    _same(reqs, rows, first)
    assert st["deep"] == 2 * st1["deep"] == 4 and st["visited"] == 2 * st1["visited"]
    acl.close()


def test_replacing_a_list(emqx):
    """set switches the answers; a refused set or request leaves them; empty lists, lists of
    rules with no filter, one client and no client at all."""
    (rules, clients, reqs), compiled_a, first_a, _ = AC.random_reference(63)
    reqs, first_a = reqs[-300:], first_a[-300:]
    compiled_b = AC.random_reference(64)[1]
    first_b = [AC.first_rule(clients[c], p, n, compiled_b) for c, p, n in reqs]
    assert first_a != first_b
    acl, exprs_a = _acl(emqx, compiled_a)
    _same(reqs, _match(acl, exprs_a, clients, reqs), first_a)
    flat_b = AC.flatten(compiled_b)
    acl.set(*flat_b[:8])
    _same(reqs, _match(acl, flat_b[8], clients, reqs), first_b)
    filters, flags, owner, perm, action, who, slot, strings = flat_b[:8]
    for bad in ((filters, flags, owner[::-1], perm, action, who, slot, strings),             # descending
                (filters, flags, [len(perm)] * len(owner), perm, action, who, slot, strings),  # out of range
                (filters, [2] * len(flags), owner, perm, action, who, slot, strings),          # unknown flag
                (filters, flags, owner, [2] + perm[1:], action, who, slot, strings),
                (filters, flags, owner, perm, [0] + action[1:], who, slot, strings),
                (filters, flags, owner, perm, action, [4] + who[1:], slot, strings),
                (filters, flags, owner, perm, action, who, [64] + slot[1:], strings)):
        with pytest.raises(emqx.EngineError):
            acl.set(*bad)
    ids, users, _, bits = AC.table_args(clients, flat_b[8])
    names = [n for _, _, n in reqs]
    with pytest.raises(emqx.EngineError):  # a client index out of range
        acl.match(names, [len(clients)] * len(reqs), [1] * len(reqs), ids, users, bits)
    with pytest.raises(emqx.EngineError):  # an action that is neither publish nor subscribe
        acl.match(names, [0] * len(reqs), [3] * len(reqs), ids, users, bits)
    _same(reqs, _match(acl, flat_b[8], clients, reqs), first_b)
    for empty in AC.EMPTY_LISTS:
        flat = AC.flatten([AR.compile(r) for r in empty])
        acl.set(*flat[:8])
        assert _match(acl, flat[8], clients, reqs) == [None] * len(reqs)
        assert acl.stats()["rules"] == len(empty) and acl.stats()["records"] == 0
    acl.set(*AC.flatten(compiled_a)[:8])
    _same(reqs, _match(acl, exprs_a, clients, reqs), first_a)
    assert _match(acl, exprs_a, [], []) == []
    acl.close()
    (rules, clients, reqs), compiled, first, res = AC.reference("one_client")
    rows, _ = _run(emqx, compiled, clients, reqs)
    _same(reqs, rows, first)


def test_builtin_database(emqx):
    """from_builtin_db over a few hundred records: emqx_authz_mnesia:authorize/4 per request."""
    table, clients, reqs = AC.builtin_db_case()
    al = emqx.AclList.from_builtin_db(AC.builtin_db_records(table))
    assert len(al.slots) == 0 and len(table) >= 200
    want = [AR.mnesia_authorize(clients[c], p, n, table) for c, p, n in reqs]
    got = al.matches([clients[c] for c, _, _ in reqs], [p for _, p, _ in reqs], [n for _, _, n in reqs])
    _same(reqs, got, want)
    al.close()


def test_one_rule_equals_match_rules(emqx):
    """A single rule {allow, all, all, Filters} with no placeholder answers rule 0 exactly where
    emqxgm_match_rules with EMQXGM_RULE_WORDS / EMQXGM_RULE_EQ finds a filter."""
    fs, _, names, _ = RC.single_reference(True)
    fs = [f for f in fs if f[1][:1] not in (b"+", b"#")]  # with a root wildcard every name has a hit
    src = [("eq", f[1]) if f[0] == "eq" else f[1] for f in fs]
    assert not any(AR.PH_CLIENTID in f or AR.PH_USERNAME in f for _, f in fs)
    # a filter that starts with "eq " would be read as an eq filter by compile_topic/1
    assert not any(isinstance(f, bytes) and f.startswith(b"eq ") for f in src)
    compiled = [AR.compile(("allow", "all", "all", src))]
    clients = [{"clientid": b"c", "username": b"u", "peerhost": None}]
    reqs = [(0, "publish" if i % 2 else "subscribe", n) for i, n in enumerate(names)]
    rows, _ = _run(emqx, compiled, clients, reqs)
    tr = emqx.TopicRules([f if f[0] == "eq" else f[1] for f in fs], words=True)
    hit = tr.first_match(names)
    assert rows == [None if h is None else 0 for h in hit]
    assert 50 <= sum(1 for r in rows if r == 0) <= len(rows) - 50
