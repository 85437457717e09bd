"""GPU parity of rule sets that return every matching rule per name (emqx_amd.RuleSet over
emqxgm_ruleset_*, k_ruleset) against the reference semantics of
tests/ruleset_ref.py, on the inputs of tests/ruleset_cases.py -- the same ones the CPU gate
(tests/test_ruleset_dev_host.py) runs the kernel's phases on under ASan + UBSan."""
import numpy as np
import pytest

import ruleset_cases as RC
import ruleset_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _same(names, rows, want):
    assert len(rows) == len(names)
    bad = [(names[i], rows[i], want[i]) for i in range(len(names)) if rows[i] != want[i]]
    assert not bad, bad[:5]


def _ruleset(emqx, rules, word_hash_bits=0):
    rs = emqx.RuleSet(rules, word_hash_bits=word_hash_bits)
    rs.tune("counters", 1)
    return rs


def test_suite_vectors(emqx):
    """a. emqx_rule_engine_SUITE t_get_rules_for_topic / _2: the hit lists and Len0 + 2 / + 4."""
    cases = RC.suite_cases()
    assert [c[0] for c in cases] == ["t_get_rules_for_topic", "t_get_rules_for_topic_2"]
    for (name, rules, topic, hits, count), more in zip(cases, (2, 4)):
        rs = emqx.RuleSet([])
        len0 = len(emqx.get_rules_for_topic(rs, topic))
        rs.set(rules)
        got = emqx.get_rules_for_topic(rs, topic)
        assert got == hits, name
        assert len(got) == len0 + more == count
        assert emqx.get_matched_egress_bridges(rs, topic) == hits


@pytest.mark.parametrize("hash_bits", [0, 4])
@pytest.mark.parametrize("n_rules", RR.MASK_EDGES)
def test_random_cases(emqx, n_rules, hash_bits):
    """b. rules of 0..4 filters in all three forms, 4,007 names ending in the edge names."""
    rules, names, want = RR.reference(n_rules)
    assert len(names) == 4007 and names[-len(RR.EDGE_NAMES):] == RR.EDGE_NAMES
    if n_rules == 63:
        assert sum(1 for r in want if not r) >= 0.05 * len(names)  # names that hit nothing
    rs = _ruleset(emqx, rules, hash_bits)
    _same(names, rs.match(names), want)
    st = rs.stats()
    assert st["records"] == st["filters"] == sum(len(r) for r in rules) and st["rules"] == n_rules
    assert st["deep"] == 2  # the 40- and the 17-level name; the 16-level one is tokenised
    if hash_bits:
        # 4 bits of hash: different words share tokens; the device's byte check tells them apart
        assert st["removed"] >= 1, st
        assert st["candidates"] > st["removed"], st


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_tile_edges_many_tiles(emqx, hash_bits):
    """c. 8,550 record words in 9 tiles, every name with 6..14 hits."""
    rules, names, want = RC.tiling_reference()
    pos, total = RC.layout(rules)
    assert sum(p[3] for p in pos) == 8550 and RC.tiles_of(total) == 9
    assert 6 <= min(len(r) for r in want) and max(len(r) for r in want) <= 14
    rs = _ruleset(emqx, rules, hash_bits)
    _same(names, rs.match(names), want)
    st = rs.stats()
    assert st["tiles"] == 9 and st["visited"] == len(names) * len(rules)


@pytest.mark.parametrize("second_rule_own", [False, True])
def test_tile_edge_between_two_hits(emqx, second_rule_own):
    """c. a/# the last record of tile 0, a/+ the first of tile 1: one rule's two filters (the
    rule once), or two rules (both)."""
    rules, names, want = RC.edge_reference(second_rule_own)
    pos, total = RC.layout(rules)
    assert pos[-2][1:] == (0, 1020, 2) and pos[-1][1:] == (1, 0, 3) and RC.tiles_of(total) == 2
    assert want[0] == ([60, 61] if second_rule_own else [60]) and names[0] == b"a/b"
    rs = _ruleset(emqx, rules)
    _same(names, rs.match(names), want)
    assert rs.stats()["tiles"] == 2


@pytest.mark.parametrize("n", RC.BLOCK_SIZES)
def test_block_edges(emqx, n):
    """d. 0, 1, 255, 256, 257, 513 and 4,007 names: the last block's idle lanes reach every
    barrier."""
    rules, names, want = RC.block_case(n)
    assert len(names) == n
    rs = _ruleset(emqx, rules)
    ptr, rule = rs.match_csr(names)
    assert ptr.dtype == np.uint64 and ptr.shape == (n + 1,) and rule.dtype == np.uint32
    assert ptr[0] == 0 and int(ptr[-1]) == len(rule) == sum(len(r) for r in want)
    _same(names, [rule[int(ptr[i]):int(ptr[i + 1])].tolist() for i in range(n)], want)


def test_passes(emqx):
    """e. 4,007 names in 14 passes of 300: rows and ptr equal the one-pass answer."""
    rules, names, want = RC.block_case(4007)
    assert -(-len(names) // RC.PASS_NAMES) == 14
    rs = _ruleset(emqx, rules)
    ptr1, rule1 = rs.match_csr(names)
    deep1 = rs.stats()["deep"]
    rs.tune("pass_names", RC.PASS_NAMES)
    ptr, rule = rs.match_csr(names)
    assert np.array_equal(ptr, ptr1) and np.array_equal(rule, rule1)
    assert rs.stats()["deep"] == deep1 + 2  # each name counted in one pass
    _same(names, rs.match(names), want)


def test_replacing_a_list(emqx):
    """f. set switches the answers; a refused set leaves them; empty lists give empty rows."""
    rules_a, names, want_a = RR.reference(63)
    rules_b, _, _ = RC.block_case(4007)
    names = names[-300:]
    want_a = want_a[-300:]
    want_b = RR.all_match(names, rules_b)
    assert want_a != want_b
    rs = emqx.RuleSet(rules_a)
    _same(names, rs.match(names), want_a)
    rs.set(rules_b)
    _same(names, rs.match(names), want_b)
    filters, flags, owner = RC.flat(rules_b)
    with pytest.raises(emqx.EngineError):
        rs.set_raw(filters, flags, owner[::-1], len(rules_b))  # descending filter_rule
    with pytest.raises(emqx.EngineError):
        rs.set_raw(filters, flags, [len(rules_b)] * len(owner), len(rules_b))  # rule out of range
    with pytest.raises(emqx.EngineError):
        rs.set_raw(filters, [3] * len(flags), owner, len(rules_b))  # unknown flag
    _same(names, rs.match(names), want_b)
    for empty in RC.EMPTY_LISTS:
        rs.set(empty)
        assert rs.match(names) == [[] for _ in names]
        assert rs.stats()["rules"] == len(empty)
    rs.set(rules_a)
    _same(names, rs.match(names), want_a)


@pytest.mark.parametrize("words", [False, True])
def test_first_entry_equals_first_match_path(emqx, words):
    """g. single-filter rules: the first entry of each row is what k_rules reports."""
    fs, rules, names, want = RC.single_reference(words)
    rs = emqx.RuleSet(rules)
    rows = rs.match(names)
    _same(names, rows, want)
    tr = emqx.TopicRules([f if isinstance(f, tuple) and f[0] == "eq" else (f[1] if isinstance(f, tuple) else f)
                          for f in fs], words=words)
    assert RR.first_of(rows) == tr.first_match(names)
    assert sum(1 for r in rows if len(r) >= 2) >= 100  # the first entry is a choice among several
    if not words:
        assert any(not r for r in rows)  # '$' names under root wildcards: NONE on both paths
