"""Reference semantics of rule sets that return every matching rule per name
(emqx_amd/csrc/gm_ruleset_match.h) on the oracle's emqx_topic:match/2
(oracle/emqx_ref.py), and the random inputs their tests share.  A helper, not a test.

A rule is a sequence of filters; a filter is ``bytes`` (match/2 on binaries), ``("words", F)``
(match/2 on word lists: no '$' clauses) or ``("eq", F)`` (word-list equality) -- the three forms
of ``_first`` in tests/test_gpu_rules.py.  A rule matches a name when any of its filters does
(emqx_plugin_libs_rule:can_topic_match_oneof/2, emqx_plugin_libs_rule.erl:340-346).
"""
import functools
import random
from typing import List, Optional, Sequence

import numpy as np

from oracle import emqx_ref as R


def filter_matches(name: bytes, f) -> bool:
    if isinstance(f, tuple):
        kind, f = f
        if kind == "eq":
            return R.words(name) == R.words(f)
        assert kind == "words", kind
        return R.match(R.words(name), R.words(f))
    return R.match(name, f)


def filters_matching(name: bytes, rule) -> int:
    return sum(1 for f in rule if filter_matches(name, f))


def all_match(names: Sequence[bytes], rules) -> List[List[int]]:
    return [[r for r, rule in enumerate(rules) if filters_matching(n, rule)] for n in names]


def first_of(rows: List[List[int]]) -> List[Optional[int]]:
    return [row[0] if row else None for row in rows]


def first_match(names: Sequence[bytes], rules) -> List[Optional[int]]:
    return first_of(all_match(names, rules))


def mask_of(rows: List[List[int]], n_rules: int) -> np.ndarray:
    m = np.zeros((len(rows), (n_rules + 63) // 64), np.uint64)
    for i, row in enumerate(rows):
        for r in row:
            m[i, r // 64] |= np.uint64(1) << np.uint64(r % 64)
    return m


def mask(names: Sequence[bytes], rules) -> np.ndarray:
    return mask_of(all_match(names, rules), len(rules))


# ---- random inputs ----------------------------------------------------------------------
# words of 0, 1, 7, 8 and 9 bytes (a level token packs up to 7 bytes and hashes longer words),
# two long words that differ only in their last byte, a '$' word and a word with a wildcard
# character inside
VOCAB = [b"", b"a", b"b", b"sevenby", b"eightbyt", b"ninebytes", b"long-word-number-1",
         b"long-word-number-2", b"$s", b"+x"]
MASK_EDGES = (63, 64, 65, 130)
BATCH_SIZES = (1, 255, 256, 257, 4007)
EDGE_NAMES = [b"", b"/", b"//", b"$SYS/x", b"$", b"$s", b"a/+", b"a/#", b"#", b"+",
              # a "#" word of a name equals a filter's '#' before that can match the rest
              # (emqx_topic.erl:78-83): a/#/c does not match a/#
              b"a/#/c", b"#/a", b"a/#/", b"+/#/a/b",
              b"/".join([b"a"] * 40), b"/".join([b"a"] * 17), b"/".join([b"a"] * 16),
              b"a/" + b"w" * 300, b"a/" + b"w" * 299 + b"x"]


def _word(rng):
    return rng.choice(VOCAB[:3]) if rng.random() < 0.6 else rng.choice(VOCAB)


def rand_name(rng) -> bytes:
    ws = [_word(rng) for _ in range(rng.randint(1, 5))]
    if rng.random() < 0.1:
        ws[0] = b"zz"  # a first word no filter has: only a root wildcard can match the name
    return b"/".join(ws)


def rand_filter(rng, root_literal: bool = False):
    d = rng.randint(1, 5)
    ws = []
    for i in range(d):
        r = rng.random()
        if i == 0 and root_literal:
            ws.append(_word(rng))
        elif i == d - 1 and r < 0.2:
            ws.append(b"#")
        elif r < 0.4:
            ws.append(b"+")
        elif r < 0.43:
            ws.append(b"#")  # also as a non-final word: a literal
        else:
            ws.append(_word(rng))
    f = b"/".join(ws)
    k = rng.random()
    if k < 0.15:
        return ("eq", f)
    return ("words", f) if k < 0.45 else f


def rand_rules(rng, n_rules: int, root_literal: bool = False):
    """0 to 4 filters per rule, flags drawn from 0, words and eq."""
    return [[rand_filter(rng, root_literal) for _ in range(rng.randint(0, 4))]
            for _ in range(n_rules)]


def random_case(n_rules: int, n_names: int = 4007):
    """(rules, names) of the random case for a rule count; names end with EDGE_NAMES.  The
    63-rule case has no filter with a root wildcard, so its "zz/..." names have no hit."""
    rng = random.Random(1000 + n_rules)
    rules = rand_rules(rng, n_rules, root_literal=(n_rules == 63))
    names = [rand_name(rng) for _ in range(n_names - len(EDGE_NAMES))] + EDGE_NAMES
    return rules, names


@functools.lru_cache(maxsize=None)
def reference(n_rules: int):
    """(rules, names, rows) of random_case(n_rules), computed once per process; read only."""
    rules, names = random_case(n_rules)
    return rules, names, all_match(names, rules)


@functools.lru_cache(maxsize=None)
def reference_stats(n_rules: int):
    rules, names, rows = reference(n_rules)
    return case_stats(names, rules, rows)


def tiling_case():
    """About 600 single-filter rules of long words (17-word records: several record tiles)
    against 500 names; a name matches the filters built from it and the final-'#' ones."""
    rng = random.Random(77)
    long_words = [b"long-word-number-%d" % i for i in range(12)]
    names = [b"/".join(rng.choice(long_words) for _ in range(16)) for _ in range(500)]
    rules = []
    for i in range(600):
        ws = names[rng.randrange(len(names))].split(b"/")
        for k in range(16):
            if rng.random() < 0.3:
                ws[k] = b"+"
        if i % 3 == 0:
            ws = ws[:rng.randint(1, 15)] + [b"#"]
        rules.append([b"/".join(ws)])
    return rules, names


def case_stats(names, rules, rows):
    """(share of names with >= 2 hits, (name, rule) pairs with more than one of the rule's
    filters matching, share of names with no hit)."""
    two = sum(1 for row in rows if len(row) >= 2) / len(names)
    none = sum(1 for row in rows if not row) / len(names)
    dedupe = sum(1 for n, row in zip(names, rows) for r in row if filters_matching(n, rules[r]) > 1)
    return two, dedupe, none
