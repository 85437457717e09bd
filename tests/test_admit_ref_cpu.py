"""The reference semantics of the admission pass alone (tests/admit_ref.py), on the CPU: against
the reference suite's vectors, against the oracle on valid UTF-8, and the coverage of the seeded
sweep the device tests run (tests/admit_cases.py), counted from admit_ref's answers alone so that
the sweep cannot pass by being all ``ok``."""
import collections
import json
import os

import pytest

import admit_cases as AC
import admit_ref as R
from oracle import emqx_ref as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "reference_vectors.json")))


def test_validate_vectors(golden):
    long_topic = b"".join(str(i).encode() + b"/" for i in range(0, 66667))
    for kind, topic, exp in golden["validate"]:
        t = long_topic if isinstance(topic, dict) else topic.encode()
        assert R.validate(kind, t) == exp, (kind, topic)
        # and as the record reports it
        w0 = R.record(R.NAME if kind == "name" else R.FILTER, t)[0]
        assert R.V_NAMES[w0 & 0xFF] == ("ok" if exp is True else exp)


def test_parse_vectors(golden):
    for inp, opts, exp in golden["parse"]:
        o = {k: (v.encode() if isinstance(v, str) else v) for k, v in opts.items()}
        got = R.parse(inp.encode(), o)
        if isinstance(exp, dict):
            assert got is None, inp
        else:
            assert got == (exp[0].encode(), {k: (v.encode() if isinstance(v, str) else v) for k, v in exp[1].items()})
        # and as the record reports it (options reach the pass as the HAS_SHARE bit alone)
        rec = R.record(R.FILTER, inp.encode(), R.IN_HAS_SHARE if "share" in opts else 0)
        assert ((rec[0] >> 8) & 0xFF) == (R.P_INVALID if isinstance(exp, dict) else R.P_OK)
        if not isinstance(exp, dict):
            assert inp.encode()[rec[2]:] == exp[0].encode()
            assert bool(rec[0] & R.F_SHARED) == ("share" in exp[1])
            if "share" in exp[1] and "share" not in opts:
                assert inp.encode()[7:7 + rec[3]] == exp[1]["share"].encode()


def test_levels_vectors(golden):
    for topic, exp in golden["levels"]:
        assert R.levels(topic.encode()) == exp
        assert R.record(R.NAME, topic.encode())[1] == exp


def test_caps_suite_vectors():
    v = json.load(open(os.path.join(GOLDEN, "admission_vectors.json")))
    c = R.caps(**v["check_pub"]["caps"])
    for flags, exp in v["check_pub"]["cases"]:
        # the suite's flags carry no topic: do_check_pub's levels clause does not apply (:83-92)
        got = R.check_pub(b"t", flags["qos"], flags["retain"], c)
        assert got == (0 if exp == "ok" else exp)
        rec = R.record(R.NAME, b"t", flags["qos"] | (R.IN_RETAIN if flags["retain"] else 0), c)
        assert (rec[0] >> 16) & 0xFF == got
    c = R.caps(**v["check_sub"]["caps"])
    for topic, subopts, exp in v["check_sub"]["cases"]:
        got, lookup = R.check_sub(topic.encode(), subopts, c)
        assert got == (0 if exp == "ok" else exp) and not lookup
        rec = R.record(R.FILTER, topic.encode(), R.IN_HAS_SHARE if "share" in subopts else 0, c)
        assert (rec[0] >> 16) & 0xFF == got


def test_golden_file_is_what_its_script_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_admission_vectors",
                                                  os.path.join(GOLDEN, "make_admission_vectors.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert json.load(open(os.path.join(GOLDEN, "admission_vectors.json"))) == json.loads(json.dumps(m.VECTORS))


def _valid_utf8(b):
    try:
        b.decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def test_equals_the_oracle_on_valid_utf8():
    items = set(AC.sweep_items()) | set(AC.PARSE_ITEMS) | set(AC.ALIGN_ITEMS)
    for b in AC.malformed() + AC.straddles()[:2]:
        items |= set(b["items"])
    n = 0
    for it in sorted(items):
        if not _valid_utf8(it):
            continue
        n += 1
        for kind in ("name", "filter"):
            try:
                want = O.validate(it, kind)
            except O.TopicError as e:
                want = e.args[0]
            assert R.validate(kind, it) == want, (kind, it)
        for opts in ({}, {"share": b"g"}):
            try:
                want = O.parse(it, opts)
            except O.TopicError:
                want = None
            assert R.parse(it, opts) == want, (it, opts)
    assert n > 1000


def test_malformed_classes_end_in_function_clause():
    for what, m in AC.MALFORMED.items():
        assert not _valid_utf8(m), what
        if what == "bad second of four":
            continue  # its '+' is reached only after the clause fails: function_clause too
        assert R.validate("filter", m) == "function_clause", what
        assert R.validate("filter", b"#" + m) == "topic_invalid_char", what
        assert R.validate("filter", m + b"#") == "function_clause", what
        assert R.validate("filter", b"#/" + m) == "topic_invalid_#", what
        assert R.validate("filter", m + b"/#") == "function_clause", what
    assert R.validate("filter", b"\xf0\x9f\x2b\x80") == "function_clause"
    assert R.validate("filter", "€".encode()[:2] + b"/" + "€".encode()[2:]) == "function_clause"
    for c in (0xD7FF, 0xE000, 0xFFFE, 0xFFFF, 0x10FFFF):
        assert R.validate("name", chr(c).encode()) is True
    for kind, item, want in (("name", b"a/#/b", "topic_invalid_#"), ("name", b"a/b#", "topic_invalid_char"),
                             ("name", b"#", "topic_name_error"), ("name", b"a/+", "topic_name_error")):
        assert R.validate(kind, item) == want


def test_sweep_coverage():
    """4096 items of 0-40 bytes, as names and as filters.  Every validate verdict an item of at
    most 40 bytes can have (topic_too_long needs 65536 bytes: the length cases have it), both parse
    verdicts and every caps reason occur at least 20 times."""
    name_b, filter_b = AC.sweep()
    assert len(name_b["items"]) == 4096 and all(len(it) <= 40 for it in name_b["items"])
    verdicts, parses, reasons = collections.Counter(), collections.Counter(), collections.Counter()
    for b in (name_b, filter_b):
        for rec in AC.expected(b):
            verdicts[R.V_NAMES[rec[0] & 0xFF]] += 1
            if b["mode"] == R.FILTER:
                parses[(rec[0] >> 8) & 0xFF] += 1
            reasons[(b["mode"], (rec[0] >> 16) & 0xFF)] += 1
    for v in R.V_NAMES:
        if v != "topic_too_long":
            assert verdicts[v] >= 20, (v, verdicts)
    assert parses[R.P_OK] >= 20 and parses[R.P_INVALID] >= 20, parses
    for key in ((R.NAME, 0), (R.NAME, 0x90), (R.NAME, 0x9B), (R.NAME, 0x9A), (R.FILTER, 0), (R.FILTER, 0x8F),
                (R.FILTER, 0xA2), (R.FILTER, 0x9E)):
        assert reasons[key] >= 20, (key, reasons)
    flags = collections.Counter()
    for rec in AC.expected(filter_b):
        for f in (R.F_WILDCARD, R.F_SHARED, R.F_EXCLUSIVE, R.F_EXCL_LOOKUP):
            flags[f] += bool(rec[0] & f)
    assert all(flags[f] >= 20 for f in (R.F_WILDCARD, R.F_SHARED, R.F_EXCLUSIVE, R.F_EXCL_LOOKUP)), flags
