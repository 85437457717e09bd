"""mqtt_match on the device (k_rules through emqxgm_match_rules) against the oracle's
emqx_topic:match/2, pair by pair: the set of tests/match2_cases.py -- every string of 1..3 words
over wildcard, '$', empty and long words, as names and as filters -- so that names with a '#' or
'+' word and filters with '#' in any position are decided, not only the shapes a broker would
accept.  tests/test_match2_cpu.py runs the same function over the same set on the CPU."""
import random

import numpy as np
import pytest

import match2_cases as M
from oracle import emqx_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    e = emqx_amd.Engine()
    yield e
    e.close()


def _flags(mode):
    from emqx_amd.engine import RULE_EQ, RULE_WORDS
    return {"binary": 0, "words": RULE_WORDS, "eq": RULE_EQ}[mode]


def _diff(got, want, names, filters):
    bad = np.argwhere(got != want)
    return [(filters[j], names[i], bool(want[j, i])) for j, i in bad[:8]], len(bad)


@pytest.mark.parametrize("mode", ["binary", "words", "eq"])
def test_every_pair_decided_alone(eng, mode):
    """One launch per filter with that filter as the only rule: each (name, filter) pair is
    decided by itself on the LDS-staged rule path (k_rules<true>)."""
    from emqx_amd.engine import NONE
    s = M.strings()
    if mode == "eq":
        want = np.array([[n == f for n in s] for f in s])  # (distinct strings: the diagonal)
    else:
        want = M.oracle(mode == "words")
    got = np.zeros_like(want)
    for j, f in enumerate(s):
        out = eng.match_rules(s, [f], [_flags(mode)])
        assert ((out == 0) | (out == NONE)).all()
        got[j] = out == 0
    msg, n_bad = _diff(got, want, s, s)
    assert n_bad == 0, (n_bad, "(filter, name, oracle)", msg)


@pytest.mark.parametrize("mode", ["binary", "words"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_first_match_over_the_whole_set(eng, mode, seed):
    """All 1,110 strings as one ordered rule list (more than k_rules<true> stages: the
    global-memory path), shuffled: the first matching rule per name."""
    s = M.strings()
    order = list(range(len(s)))
    random.Random(seed).shuffle(order)
    want = M.first_match(M.oracle(mode == "words"), order)
    assert len(order) > 1024 and (want != 0xFFFFFFFF).mean() > 0.5
    got = eng.match_rules(s, [s[j] for j in order], [_flags(mode)] * len(order))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(s[i], int(got[i]), int(want[i])) for i in bad[:8]]


@pytest.mark.parametrize("mode", ["binary", "words"])
def test_golden_match_vectors_crossed(eng, golden, mode):
    """The names and filters of the reference suite's match/2 vectors (tests/golden), every name
    against every filter; the vectors' own pairs keep their recorded answers."""
    from emqx_amd.engine import NONE
    names = sorted({n.encode() for n, _, _ in golden["match"]})
    filters = sorted({f.encode() for _, f, _ in golden["match"]})
    if mode == "words":
        want = np.array([[R.match(R.words(n), R.words(f)) for n in names] for f in filters])
    else:
        want = np.array([[R.match(n, f) for n in names] for f in filters])
        for n, f, exp in golden["match"]:
            assert want[filters.index(f.encode()), names.index(n.encode())] == exp
    got = np.array([eng.match_rules(names, [f], [_flags(mode)]) != NONE for f in filters])
    msg, n_bad = _diff(got, want, names, filters)
    assert n_bad == 0, (n_bad, "(filter, name, oracle)", msg)
