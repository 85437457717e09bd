"""The inputs that the rule-set device path is checked on, shared by its CPU gate
(tests/test_ruleset_dev_host.py: the kernel's phases and the host code under ASan + UBSan) and
its GPU tests (tests/test_gpu_ruleset.py), so that both see exactly the same cases.  Built on
tests/ruleset_ref.py; expected rows are computed once per process and are read only.  A helper,
not a test."""
import functools
import json
import os

import ruleset_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RS_MAX_LEVELS = 16    # emqx_amd/csrc/gm_ruleset_match.h
RS_TILE_WORDS = 1024
BLOCK_SIZES = (0,) + RR.BATCH_SIZES[:4] + (513,) + RR.BATCH_SIZES[4:]  # 0 1 255 256 257 513 4007
PASS_NAMES = 300


def suite_cases():
    """[(name, rules, topic, hits, count)] of tests/golden/rule_engine_vectors.json."""
    with open(os.path.join(ROOT, "tests", "golden", "rule_engine_vectors.json")) as f:
        cases = json.load(f)["cases"]
    return [(c["name"], [[f.encode() for f in r["from"]] for r in c["rules"]], c["topic"].encode(),
             c["hits"], c["count"]) for c in cases]


def flat(rules):
    """(filters, flags, filter_rule) of a rule list, in emqxgm_ruleset_set's terms."""
    filters, flags, owner = [], [], []
    for r, rule in enumerate(rules):
        for f in rule:
            flag, f = ({"eq": 1, "words": 2}[f[0]], f[1]) if isinstance(f, tuple) else (0, f)
            filters.append(f)
            flags.append(flag)
            owner.append(r)
    return filters, flags, owner


def record_words(f) -> int:
    """Words of a filter's compiled record (rs_compile): header + one per level, a final '#'
    takes none, more than RS_MAX_LEVELS levels: the header alone."""
    eq = isinstance(f, tuple) and f[0] == "eq"
    ws = (f[1] if isinstance(f, tuple) else f).split(b"/")
    n = len(ws) - (1 if not eq and ws[-1] == b"#" else 0)
    return 1 if n > RS_MAX_LEVELS else 1 + n


def layout(rules):
    """([(rule, tile, word in tile, words)] per filter, total words of the stream) as rs_append
    lays the records out: none straddles a tile."""
    at, pos = 0, []
    for r, rule in enumerate(rules):
        for f in rule:
            w = record_words(f)
            if at % RS_TILE_WORDS and at % RS_TILE_WORDS + w > RS_TILE_WORDS:
                at += RS_TILE_WORDS - at % RS_TILE_WORDS
            pos.append((r, at // RS_TILE_WORDS, at % RS_TILE_WORDS, w))
            at += w
    return pos, at


def tiles_of(total_words: int) -> int:
    return (total_words + RS_TILE_WORDS - 1) // RS_TILE_WORDS


def edge_list(second_rule_own: bool):
    """Sixty 17-word records (1,020 words), then a/# (2 words: 1,022) and a/+ (3 words: it does
    not fit, the stream is padded and a/+ opens tile 1).  Both match a/b.  second_rule_own: a/+ is
    a rule of its own (both rules are reported) instead of the second filter of a/#'s rule (the
    rule is reported once, its two hits lying in two tiles)."""
    fill = [[b"/".join(b"f%d" % i for _ in range(16))] for i in range(60)]
    tail = [[b"a/#"], [b"a/+"]] if second_rule_own else [[b"a/#", b"a/+"]]
    names = [b"a/b", b"a", b"a/b/c", b"/".join([b"f7"] * 16), b"x"]
    return fill + tail, names


@functools.lru_cache(maxsize=None)
def edge_reference(second_rule_own: bool):
    rules, names = edge_list(second_rule_own)
    return rules, names, RR.all_match(names, rules)


@functools.lru_cache(maxsize=None)
def tiling_reference():
    rules, names = RR.tiling_case()
    return rules, names, RR.all_match(names, rules)


def block_case(n: int):
    """The last n names (the edge names among them) of the 65-rule random case."""
    rules, names, want = RR.reference(65)
    return rules, names[len(names) - n:], want[len(want) - n:]


def single_filter_rules(words: bool):
    """64 single-filter rules for the comparison with the first-match path (TopicRules): plain
    filters (words off) or word-list filters (words on), ("eq", F) kept in both."""
    rules, _ = RR.random_case(130)
    fs = [f for rule in rules for f in rule][:64]
    out = []
    for f in fs:
        if isinstance(f, tuple) and f[0] == "eq":
            out.append(f)
        else:
            f = f[1] if isinstance(f, tuple) else f
            out.append(("words", f) if words else f)
    return out


@functools.lru_cache(maxsize=None)
def single_reference(words: bool):
    fs = single_filter_rules(words)
    names = RR.reference(63)[1][-600:]
    rules = [[f] for f in fs]
    return fs, rules, names, RR.all_match(names, rules)


EMPTY_LISTS = ([], [[], [], []])
