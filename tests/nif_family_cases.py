"""Device scenarios for the NIF's other families (tests/test_gpu_nif.py, E and F): the retainer,
match_rules and rule sets, ACL lists, the ACL database and shared subscriptions, each through the
driver of tests/host_harness/nif_driver.c.  Inputs come from the family's own *_cases.py where it
has some; every expectation from its Python reference (retain_ref, ruleset_ref, acl_ref through
acl_cases / acldb_cases, share_ref through share_cases).  Built like tests/nif_cases.py: a scenario
fills a Script and returns check(run)."""
import struct

import acl_cases as AC
import acldb_cases as AD
import retain_ref as RR
import ruleset_cases as RS
import ruleset_ref as RUR
import share_cases as SC
import share_ref as SR
from oracle import emqx_ref as R
from nif_cases import OK, TRUE, FALSE, UNDEFINED, NONE, boolean
from nif_terms import Atom, Var

A = Atom


# ---- E. the retainer ----------------------------------------------------------------------------
NOW = 1000
SPECS = [[1, 2], [3]]
E_BASE = [(b"a/b", 0), (b"a/c", 500), (b"a/d", 5000), (b"b", 0), (b"b/c/d", 7000), (b"$SYS/x", 0),
          (b"/a", 0), (b"a//b", 999)]
E_DELTA = [(b"x/y/z", 1), (b"x/y", 0), (b"a/e", 1001), (b"w/" + b"v" * 300, 0)]
E_FILTERS = [b"#", b"+", b"a/+", b"a/#", b"+/+/+", b"$SYS/#", b"x/y/#", b"b", b"nope/#", b"a/b", b"+/+"]
RC_DONE = 3


def case_retainer(s):
    ref = RR.Retainer(SPECS)
    s.call("retain_open", [0, SPECS], bind="T")
    steps = []   # (output index, expected, how to compare)

    def store(items, ts0, four):
        for k, (t, exp) in enumerate(items):
            ts = ts0 + 10 * k
            if four:
                steps.append((s.call("retain_store", [Var("T"), t, exp, ts]), OK, "eq"))
            else:
                steps.append((s.call("retain_store", [Var("T"), t, exp]), OK, "eq"))
            ref.store_retained(t, exp, ts if four else 0)

    def match_all():
        o = s.call("retain_match", [Var("T"), E_FILTERS, NOW])
        steps.append((o, [sorted(ref.match_messages(f, NOW)) for f in E_FILTERS], "rows"))

    store(E_BASE, 100, True)
    steps.append((s.call("retain_commit", [Var("T")]), OK, "eq"))
    match_all()
    # a small delta on top of the base: the second batch lands in the delta store
    steps.append((s.call("retain_tune", [Var("T"), A("delta_max"), 64]), OK, "eq"))
    store(E_DELTA, 50, True)
    steps.append((s.call("retain_store", [Var("T"), b"three", 0]), OK, "eq"))  # retain_store/3: timestamp 0
    ref.store_retained(b"three", 0, 0)
    steps.append((s.call("retain_commit", [Var("T")]), OK, "eq"))
    match_all()
    # cursor reads: limit 1, 2 and 0 (all), drained to the end
    want = [sorted(ref.match_messages(f, NOW)) for f in E_FILTERS]
    drains = []
    for limit in (1, 2, 0):
        n_steps = 1 if limit == 0 else max(len(w) for w in want) // limit + 1
        outs = []
        cursors = [b""] * len(E_FILTERS)
        for k in range(n_steps):
            outs.append(s.call("retain_match_limit", [Var("T"), E_FILTERS, NOW, [limit] * len(E_FILTERS), cursors],
                               bind="Q"))
            cursors = Var("Q_2")
        drains.append((limit, outs))
    # pages, ordered by timestamp (all distinct here but `three`, which has the only 0)
    pages = []
    for f in (None, b"a/#", b"+/+"):
        for limit in (1, 4, 100):
            for page in (1, 2, 3):
                o = s.call("retain_page_read", [Var("T"), UNDEFINED if f is None else f, page, limit, NOW])
                pages.append((o, ref.page_read(f, page, limit, NOW), (f, page, limit)))
    steps.append((s.call("retain_delete", [Var("T"), b"b"]), OK, "eq"))
    ref.delete_message(b"b")
    steps.append((s.call("retain_commit", [Var("T")]), OK, "eq"))
    match_all()
    o = s.call("retain_clear_expired", [Var("T"), NOW])
    steps.append((o, sorted(ref.clear_expired(NOW)), "sorted"))
    match_all()
    gone = sorted(ref.search_table(R.words(b"a/+"), 0))
    o = s.call("retain_delete_matching", [Var("T"), b"a/+"])
    ref.delete_message(b"a/+")
    steps.append((o, gone, "sorted"))
    match_all()
    steps.append((s.call("retain_clean", [Var("T")]), OK, "eq"))
    ref.clean()
    steps.append((s.call("retain_commit", [Var("T")]), OK, "eq"))
    match_all()
    s.drop("Q")
    s.drop("Q_1")
    s.drop("Q_2")
    s.drop("T")

    def check(r):
        assert gone and len(gone) < len(E_BASE)
        for o, exp, how in steps:
            got = r.out[o]
            if how == "rows":
                got = [sorted(row) for row in got]
            elif how == "sorted":
                got = sorted(got)
            assert got == exp, (s.lines[o][:80] if o < len(s.lines) else o, got, exp)
        for limit, outs in drains:
            rows = [[] for _ in E_FILTERS]
            for o in outs:
                got_rows, curs = r.out[o]
                assert len(got_rows) == len(curs) == len(E_FILTERS)
                for i, row in enumerate(got_rows):
                    assert limit == 0 or len(row) <= limit, (limit, i, row)
                    rows[i] += row
            assert [sorted(x) for x in rows] == want, (limit, rows)   # each topic once, none missing
            assert all(len(set(x)) == len(x) for x in rows)
            assert all(struct.unpack("<QII", c)[1] == RC_DONE for c in curs), (limit, curs)
        for o, exp, what in pages:
            assert r.out[o] == exp, (what, r.out[o], exp)
    return check


# ---- F. match_rules and rule sets ---------------------------------------------------------------
def _nif_filter(f):
    return (f[1], A(f[0])) if isinstance(f, tuple) else (f, A("binary"))


HAND_RULES = [[b"a/+", ("eq", b"a/#")], [], [("words", b"$SYS/#"), b"#"], [("words", b"+/b")], [b"a/b", b"a/b"],
              [("eq", b"")], [b"+"]]
HAND_NAMES = [b"a/b", b"a/#", b"$SYS/x", b"", b"x", b"a/b/c", b"/b", b"$q"]


def case_ruleset(s):
    s.call("open", [[0], 64, 4096, 200, 8, {}], bind="R")
    s.call("ruleset_open", [0, 0], bind="S")
    lists = [(HAND_RULES, HAND_NAMES)] + [RS.edge_list(own) for own in (True, False)]
    outs = []
    for rules, names in lists:
        rules = [list(rule) for rule in rules]
        st = s.call("ruleset_set", [Var("S"), [[_nif_filter(f) for f in rule] for rule in rules]])
        outs.append((st, s.call("ruleset_match", [Var("S"), list(names)]), RUR.all_match(names, rules)))
    # match_rules: the first matching rule of a flat list, in all three kinds
    flat = [f for rule in HAND_RULES for f in rule]
    first = s.call("match_rules", [Var("R"), HAND_NAMES, [_nif_filter(f) for f in flat]])
    want_first = RUR.first_match(HAND_NAMES, [[f] for f in flat])
    none = s.call("match_rules", [Var("R"), HAND_NAMES, []])
    close = s.call("ruleset_close", [Var("S")])
    after = s.call("ruleset_match", [Var("S"), [b"a"]], valid=False)
    s.drop("S")
    s.drop("R")

    def check(r):
        for st, m, want in outs:
            assert r.out[st] == OK and r.out[m] == want, (r.out[st], r.out[m], want)
        assert r.out[first] == [NONE if w is None else w for w in want_first], (r.out[first], want_first)
        assert {A("none")} < set(r.out[first]) and r.out[none] == [NONE] * len(HAND_NAMES)
        assert r.out[close] == OK and r.out[after] == A("badarg")
    return check


# ---- F. ACL lists -------------------------------------------------------------------------------
def _opt(v):
    return UNDEFINED if v is None else v


def case_acl(s):
    s.call("acl_open", [0, 0], bind="L")
    outs = []
    for case in (AC.values_case(), AC.slots_case(), AC.order_case()):
        rules, clients, reqs = case
        compiled, first, _ = AC.answers(case)
        filters, flags, owner, perm, action, who, slot, strings, exprs = AC.flatten(compiled)
        terms = []
        for r in range(len(compiled)):
            w = {AC.WHO_ALL: A("all"), AC.WHO_USERNAME: (A("username"), strings[r]),
                 AC.WHO_CLIENTID: (A("clientid"), strings[r]), AC.WHO_HOST: (A("slot"), slot[r])}[who[r]]
            fs = [(filters[i], A("eq") if flags[i] & AC.EQ else A("words")) for i in range(len(filters)) if owner[i] == r]
            terms.append((A("allow") if perm[r] else A("deny"), w,
                          A({1: "publish", 2: "subscribe", 3: "all"}[action[r]]), fs))
        ids, users, _, bits = AC.table_args(clients, exprs)
        st = s.call("acl_set", [Var("L"), terms])
        m = s.call("acl_match", [Var("L"), ([(_opt(i), _opt(u), b) for i, u, b in zip(ids, users, bits)],
                                            [(n, c, A(p)) for c, p, n in reqs])])
        outs.append((st, m, [NONE if f is None else f for f in first]))
    close = s.call("acl_close", [Var("L")])
    s.drop("L")

    def check(r):
        for st, m, want in outs:
            assert r.out[st] == OK, r.out[st]
            got = r.out[m]
            assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:10]
            assert len(set(want)) > 2
        assert r.out[close] == OK
    return check


# ---- F. the ACL database ------------------------------------------------------------------------
def case_acldb(s):
    sc = AD.keys_case()
    reqs = sc.queries()[0][1]
    some = reqs[::7]
    sc.delete(("clientid", b"a"))
    sc.delete(("username", b"sevenby"))
    sc.commit()
    sc.query(some)
    sc.store("all", [("deny", "all", b"#")])
    sc.commit()
    sc.query(some)
    sc.purge()
    sc.commit()
    sc.query(some)
    s.call("acldb_open", [0, 0], bind="D")
    clients = [(_opt(c["clientid"]), _opt(c["username"])) for c in sc.clients]
    outs, oks = [], []

    def store(key, rules):
        kind, k = (A("all"), b"") if key == "all" else (A(key[0]), key[1])
        oks.append(s.call("acldb_store", [Var("D"), kind, k, [(A(p), A(a), t) for p, a, t in rules]]))

    for op in sc.ops:
        if op[0] == "many":
            for key, rules in op[1]:
                store(key, rules)
        elif op[0] == "store":
            store(op[1], op[2])
        elif op[0] == "delete":
            oks.append(s.call("acldb_delete", [Var("D"), A(op[1][0]), op[1][1]]))
        elif op[0] == "purge":
            oks.append(s.call("acldb_purge", [Var("D")]))
        elif op[0] == "commit":
            oks.append(s.call("acldb_commit", [Var("D")]))
        elif op[0] == "query":
            src = {AD.CLIENTID: A("clientid"), AD.USERNAME: A("username"), AD.ALL: A("all")}
            want = [A("nomatch") if d is None else (A("allow") if d[0] else A("deny"), src[d[1]], d[2]) for d in op[2]]
            outs.append((s.call("acldb_match", [Var("D"), (clients, [(n, c, A(p)) for c, p, n in op[1]])]), want))
    close = s.call("acldb_close", [Var("D")])
    s.drop("D")

    def check(r):
        assert all(r.out[o] == OK for o in oks), [r.out[o] for o in oks if r.out[o] != OK][:5]
        assert len(outs) == 4
        for o, want in outs:
            got = r.out[o]
            assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:10]
        assert len(set(outs[0][1])) > 4 and set(outs[3][1]) == {A("nomatch")}
        assert r.out[close] == OK
    return check


# ---- F. shared subscriptions --------------------------------------------------------------------
def case_share(s):
    script = SC.mutation_script()
    want = SC.run_ref(script)
    s.call("share_open", [0, 0], bind="H")
    oks, outs = [], []
    for op in script:
        if op[0] == "S":
            oks.append(s.call("share_subscribe", [Var("H"), op[1], op[2], op[3], boolean(op[4])]))
        elif op[0] == "U":
            oks.append(s.call("share_unsubscribe", [Var("H"), op[1], op[2], op[3]]))
        elif op[0] == "D":
            oks.append(s.call("share_down", [Var("H"), op[1]]))
        elif op[0] == "G":
            oks.append(s.call("share_strategy", [Var("H"), A("default") if op[1] is None else op[1],
                                                 A(SR.STRATEGIES[op[2]])]))
        elif op[0] == "C":
            oks.append(s.call("share_commit", [Var("H")]))
        elif op[0] == "Q":
            outs.append(("Q", s.call("share_pick", [Var("H"), [(t, g, hc, ht, draw, UNDEFINED if st == SR.NONE else st)
                                                               for g, t, hc, ht, draw, st in op[1]]])))
        elif op[0] == "M":
            outs.append(("M", s.call("share_members", [Var("H"), op[1], op[2]])))
        elif op[0] in ("K", "X"):
            outs.append((op[0], None))
    close = s.call("share_close", [Var("H")])
    s.drop("H")
    status = {SR.PICKED: A("picked"), SR.NO_SUBSCRIBERS: A("no_subscribers"), SR.HOST_STRATEGY: A("host_strategy")}

    def check(r):
        assert all(r.out[o] == OK for o in oks), [r.out[o] for o in oks if r.out[o] != OK][:5]
        assert len(outs) == len(want)
        seen = set()
        for (kind, o), w in zip(outs, want):
            if kind == "Q":
                exp = [(status[st], UNDEFINED if m == SR.NONE else m, UNDEFINED if so == SR.NONE else so, n)
                       for m, st, so, n in w]
                assert r.out[o] == exp, [(g, e) for g, e in zip(r.out[o], exp) if g != e][:10]
                seen |= {e[0] for e in exp}
            elif kind == "M":
                assert r.out[o] == [(sub, boolean(loc)) for sub, loc in w], (r.out[o], w)
        assert {A("picked"), A("no_subscribers")} <= seen
        assert r.out[close] == OK
    return check


FAMILIES = {"ruleset": case_ruleset, "acl": case_acl, "acldb": case_acldb, "share": case_share}
