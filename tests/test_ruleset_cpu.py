"""Rule sets that return every matching rule per name, on the CPU:

1. the reference semantics (tests/ruleset_ref.py, on the oracle's emqx_topic:match/2) reproduce
   the rule-engine suite's vectors (tests/golden/rule_engine_vectors.json, from
   apps/emqx_rule_engine/test/emqx_rule_engine_SUITE.erl:285-346);
2. the filter compile step and the token predicate of emqx_amd/csrc/gm_ruleset_match.h agree
   with that reference, run by tests/host_harness/ruleset_main.cpp under ASan + UBSan -- with
   hash_bits 4 the token stage must raise false candidates that the byte check removes.
"""
import json
import os
import subprocess

import pytest

import ruleset_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "tests", "host_harness")
EXE = os.path.join(H, "build", "ruleset_main_asan")
SRC = os.path.join(H, "ruleset_main.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "emqx_amd", "csrc", f) for f in ("gm_ruleset_match.h", "gm_common.h")]


def test_reference_reproduces_rule_engine_suite():
    with open(os.path.join(ROOT, "tests", "golden", "rule_engine_vectors.json")) as f:
        cases = json.load(f)["cases"]
    assert [c["name"] for c in cases] == ["t_get_rules_for_topic", "t_get_rules_for_topic_2"]
    for c in cases:
        rules = [[f.encode() for f in r["from"]] for r in c["rules"]]
        topic = c["topic"].encode()
        rows = RR.all_match([topic], rules)
        assert rows == [c["hits"]], c["name"]
        assert len(rows[0]) == c["count"]
        assert RR.first_match([topic], rules) == [c["hits"][0]]
        m = RR.mask([topic], rules)
        assert m.shape == (1, 1) and int(m[0, 0]) == sum(1 << r for r in c["hits"])
    assert len(cases[1]["rules"]) == 6 and cases[1]["hits"] == [0, 1, 3, 4]


@pytest.fixture(scope="module")
def exe():
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in DEPS):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", SRC, "-o", EXE]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return EXE


def _hex(b: bytes) -> str:
    return b.hex() or "-"


def _run(exe, rules, names, hash_bits, tmp_path):
    lines = [str(hash_bits), str(len(rules))]
    for rule in rules:
        lines.append(str(len(rule)))
        for f in rule:
            flag, f = ({"eq": 1, "words": 2}[f[0]], f[1]) if isinstance(f, tuple) else (0, f)
            lines.append(f"{flag} {_hex(f)}")
    lines.append(str(len(names)))
    lines += [_hex(n) for n in names]
    path = tmp_path / "ruleset_in.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout.split("\n")
    assert out[-1] == "" and out[-2].startswith("STATS "), r.stdout[-500:]
    rows = [[int(x) for x in line.split()] for line in out[:len(names)]]
    assert len(out) == len(names) + 2
    keys = ("records", "tiles", "token_hits", "removed", "deep")
    return rows, dict(zip(keys, map(int, out[-2].split()[1:])))


@pytest.mark.parametrize("hash_bits", [0, 4])
@pytest.mark.parametrize("n_rules", RR.MASK_EDGES)
def test_token_predicate_matches_reference(exe, n_rules, hash_bits, tmp_path):
    rules, names, want = RR.reference(n_rules)
    # the inputs exercise what they are meant to, judged on the reference alone: most names hit
    # several rules, many hits come from more than one filter of a rule (reported once), and
    # one case has names without a hit
    assert len(names) == 4007 and names[-len(RR.EDGE_NAMES):] == RR.EDGE_NAMES
    assert {len(r) for r in rules} == {0, 1, 2, 3, 4}
    two, dedupe, none = RR.reference_stats(n_rules)
    assert two >= 0.5 and dedupe >= 50
    if n_rules == 63:
        assert 0.05 <= none <= 0.95
    rows, st = _run(exe, rules, names, hash_bits, tmp_path)
    bad = [(names[i], rows[i], want[i]) for i in range(len(names)) if rows[i] != want[i]]
    assert not bad, bad[:5]
    assert st["records"] == sum(len(r) for r in rules)
    assert st["deep"] == 2  # the 40- and the 17-level name; the 16-level one is tokenised
    if hash_bits:
        # 4 bits of hash: different words share tokens, and only the byte check tells them apart
        assert st["removed"] >= 1, st
        assert st["token_hits"] > st["removed"]


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_token_predicate_over_several_tiles(exe, hash_bits, tmp_path):
    rules, names = RR.tiling_case()
    rows, st = _run(exe, rules, names, hash_bits, tmp_path)
    assert st["tiles"] >= 3, st
    assert rows == RR.all_match(names, rules)
    assert min(len(r) for r in rows) >= 1  # every name meets the filters built from it
