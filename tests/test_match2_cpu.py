"""mqtt_match (emqx_amd/csrc/gm_match.h), the matcher of k_rules, k_verify and
k_verify_scatter, against the oracle's emqx_topic:match/2 on the CPU: every (name, filter) pair
of tests/match2_cases.py, 2 x 1,232,100 decisions, run by tests/host_harness/match2_main.cpp
under ASan + UBSan.  The set holds names with a '#' word, which match/2 compares as a word
before it looks for a final '#' of the filter (emqx_topic.erl:78 before :82)."""
import os
import subprocess

import numpy as np
import pytest

import match2_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "tests", "host_harness")
EXE = os.path.join(H, "build", "match2_main_asan")
SRC = os.path.join(H, "match2_main.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "emqx_amd", "csrc", f) for f in ("gm_match.h", "gm_common.h")]


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


def test_set_is_not_vacuous():
    """Judged on the oracle alone: a few percent of the pairs match, and the class that a
    matcher returning true at any final '#' gets wrong is there in numbers."""
    s = M.strings()
    assert len(s) == 1110
    binary, words = M.oracle(False), M.oracle(True)
    for mat in (binary, words):
        assert mat.shape == (1110, 1110)
        assert 0.005 <= mat.mean() <= 0.05, int(mat.sum())
    assert not (binary & ~words).any()  # the '$' clauses only ever take matches away
    assert (words & ~binary).any()
    hard = sum(M.hash_under_hash(n, f) for f in s if f[-1:] == b"#" for n in s if b"#/" in n)
    assert hard >= 250, hard
    assert not any(words[j, i] for j, f in enumerate(s) if f[-1:] == b"#"
                   for i, n in enumerate(s) if b"#/" in n and M.hash_under_hash(n, f))


def test_mqtt_match_equals_oracle_on_every_pair(exe, tmp_path):
    s = M.strings()
    lines = [str(len(s))] + [x.hex() or "-" for x in s]
    path = tmp_path / "match2_in.txt"
    path.write_text("\n".join(lines + lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout.split("\n")
    assert len(out) == 2 * len(s) + 1 and out[-1] == ""
    assert all(len(row) == len(s) for row in out[:-1])
    got = np.array([np.frombuffer(row.encode(), np.uint8) == ord("1") for row in out[:-1]])
    for words in (False, True):
        want = M.oracle(words)
        bad = np.argwhere(got[int(words)::2] != want)
        # every difference named with its class, so that a regression says what it is
        msg = [(s[i], s[j], bool(want[j, i]), M.hash_under_hash(s[i], s[j], prefix=False))
               for j, i in bad[:8]]
        assert len(bad) == 0, (words, len(bad), "(name, filter, oracle, '#' under final '#')", msg)
