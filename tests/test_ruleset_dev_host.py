"""The CPU gate of the rule-set device path: k_ruleset's phase functions
(emqx_amd/csrc/gm_ruleset.inc) run lane by lane, phase by phase, and the host code behind the
emqxgm_ruleset_* C-ABI (emqx_amd/csrc/gm_ruleset.cpp, every "device" array an allocation of
exactly the bytes in use) run under ASan + UBSan in tests/host_harness/ruleset_dev_main.cpp, on
exactly the inputs of tests/test_gpu_ruleset.py (tests/ruleset_cases.py), against the reference
semantics of tests/ruleset_ref.py.  No GPU; this passes before the kernel runs on one."""
import os
import subprocess

import pytest

import host_build
import ruleset_cases as RC
import ruleset_ref as RR

CSRC = host_build.CSRC
H = host_build.H
DEPS = [os.path.join(CSRC, f) for f in ("gm_ruleset.cpp", "gm_ruleset.inc", "gm_ruleset_match.h",
                                        "gm_match.h")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "ruleset_shim.h")]


@pytest.fixture(scope="module")
def exe():
    return host_build.build("ruleset_dev_main.cpp", deps=DEPS)


def _hex(b: bytes) -> str:
    return b.hex() or "-"


def _run(exe, rules, names, hash_bits, tmp_path, pass_names=0):
    lines = [str(hash_bits), str(pass_names), str(len(rules))]
    for rule in rules:
        lines.append(str(len(rule)))
        for f in rule:
            flag, f = ({"eq": 1, "words": 2}[f[0]], f[1]) if isinstance(f, tuple) else (0, f)
            lines.append(f"{flag} {_hex(f)}")
    lines.append(str(len(names)))
    lines += [_hex(n) for n in names]
    path = tmp_path / "ruleset_dev_in.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=host_build.ENV, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and out[-2].startswith("STATS "), r.stdout[-500:]
    assert len(out) == len(names) + 2
    rows = [[int(x) for x in line.split()] for line in out[:len(names)]]
    keys = ("records", "tiles", "filters", "rules", "candidates", "removed", "deep", "visited")
    return rows, dict(zip(keys, map(int, out[-2].split()[1:])))


def _same(names, rows, want):
    bad = [(names[i], rows[i], want[i]) for i in range(len(names)) if rows[i] != want[i]]
    assert not bad, bad[:5]


def test_suite_vectors(exe, tmp_path):
    cases = RC.suite_cases()
    assert [len(c[1]) for c in cases] == [2, 6]
    for name, rules, topic, hits, count in cases:
        rows, st = _run(exe, rules, [topic], 0, tmp_path)
        assert rows == [hits] and len(rows[0]) == count, name
        assert st["rules"] == len(rules) and st["filters"] == sum(len(r) for r in rules)


@pytest.mark.parametrize("hash_bits", [0, 4])
@pytest.mark.parametrize("n_rules", RR.MASK_EDGES)
def test_random_cases(exe, n_rules, hash_bits, tmp_path):
    rules, names, want = RR.reference(n_rules)
    assert len(names) == 4007 and names[-len(RR.EDGE_NAMES):] == RR.EDGE_NAMES
    rows, st = _run(exe, rules, names, hash_bits, tmp_path)
    _same(names, rows, want)
    assert st["records"] == sum(len(r) for r in rules)
    assert st["deep"] == 2  # the 40- and the 17-level name; the 16-level one is tokenised
    assert st["visited"] <= len(names) * st["records"]
    if hash_bits:
        assert st["removed"] >= 1, st
        assert st["candidates"] > st["removed"]


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_tile_edges_many_tiles(exe, hash_bits, tmp_path):
    rules, names, want = RC.tiling_reference()
    pos, total = RC.layout(rules)
    # 8,550 record words; with the RS_END padding at tile ends the stream has 9 tiles
    assert sum(p[3] for p in pos) == 8550 and RC.tiles_of(total) == 9
    assert 6 <= min(len(r) for r in want) and max(len(r) for r in want) <= 14
    rows, st = _run(exe, rules, names, hash_bits, tmp_path)
    _same(names, rows, want)
    assert st["tiles"] == 9 and st["visited"] == len(names) * len(rules)


@pytest.mark.parametrize("second_rule_own", [False, True])
def test_tile_edge_between_two_hits(exe, second_rule_own, tmp_path):
    rules, names, want = RC.edge_reference(second_rule_own)
    # on the reference alone: a/# is the last record of tile 0, a/+ the first of tile 1, and the
    # stream has two tiles
    pos, total = RC.layout(rules)
    (r0, t0, w0, n0), (r1, t1, w1, n1) = pos[-2:]
    assert (t0, w0, n0) == (0, 1020, 2) and (t1, w1, n1) == (1, 0, 3)
    assert w0 + n0 + n1 > RC.RS_TILE_WORDS and RC.tiles_of(total) == 2
    assert (r0 == r1) == (not second_rule_own)
    assert RR.filters_matching(b"a/b", rules[60]) == (1 if second_rule_own else 2)
    assert want[0] == ([60, 61] if second_rule_own else [60])
    rows, st = _run(exe, rules, names, 0, tmp_path)
    _same(names, rows, want)
    assert st["tiles"] == 2, st


@pytest.mark.parametrize("n", RC.BLOCK_SIZES)
def test_block_edges(exe, n, tmp_path):
    rules, names, want = RC.block_case(n)
    assert len(names) == n
    rows, _ = _run(exe, rules, names, 0, tmp_path)
    _same(names, rows, want)


def test_passes(exe, tmp_path):
    rules, names, want = RC.block_case(4007)
    assert -(-len(names) // RC.PASS_NAMES) == 14
    rows, st = _run(exe, rules, names, 0, tmp_path, pass_names=RC.PASS_NAMES)
    _same(names, rows, want)
    assert st["deep"] == 2  # each name is counted in one pass


@pytest.mark.parametrize("rules", RC.EMPTY_LISTS)
def test_empty_lists(exe, rules, tmp_path):
    names = RR.EDGE_NAMES
    rows, st = _run(exe, rules, names, 0, tmp_path)
    assert rows == [[] for _ in names]
    assert st["records"] == 0 and st["tiles"] == 0 and st["rules"] == len(rules)


@pytest.mark.parametrize("words", [False, True])
def test_single_filter_rules_first_entry(exe, words, tmp_path):
    fs, rules, names, want = RC.single_reference(words)
    assert len(rules) == 64 and len(names) == 600
    rows, _ = _run(exe, rules, names, 0, tmp_path)
    _same(names, rows, want)
    assert RR.first_of(rows) == RR.first_of(want)
