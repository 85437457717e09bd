"""The inputs of the tests of the pick inside the publish (emqxgm_publish_shared_batch, k_pubshare;
DESIGN.md 6b "The pick inside the publish"), one set for the reference alone
(tests/test_pubshare_ref_cpu.py), the CPU gate (tests/test_pubshare_dev_host.py) and the device
(tests/test_gpu_pubshare.py).  A helper, not a test.

A script is a list of operations.  Groups and subscribers are integers (the handles), nodes are
strings, topics and filters are bytes:
  ("G", group | None, strategy)   set_strategy       ("S", group, topic, sub, local)  subscribe
  ("U", group, topic, sub)        unsubscribe        ("C",)                           share commit
  ("RA", filter, dest)            add_route          ("RD", filter, dest)             delete_route
  ("RC",)                         route commit       dest: a node, or a group (its route is on n1)
  ("P", topics, msgs)             publish -> per topic [(To, dest, (member, status, state, Count))]
msgs[i] = (hc, ht, draw, states) of topic i; states is None (the call passes no state list when
every message of it has None) or a list of ((group, To), value) in the publisher's order.

The expected answer of topic t is built in two steps: the entries are oracle.emqx_ref.publish's;
each group entry's quadruple is share_ref.SharedSubRef.pick's with the state the case passed for
(group, To) (the first pair of the list), each node entry's is NOT_SHARED_ANSWER."""
import random

import share_cases as SC
import share_ref as SR
from oracle import emqx_ref as R

NONE = SR.NONE
NOT_SHARED = 5
NOT_SHARED_ANSWER = (NONE, NOT_SHARED, NONE, 0)
LOCAL_NODE = "n1"
TO_LENGTHS = (1, 7, 8, 9, 64, 300)


def gname(g):
    """The group's name in the oracle's route bag (a binary: aggre/1 sorts groups after nodes)."""
    return b"g%05d" % g


def _dest(d):
    return d if isinstance(d, str) else (gname(d), LOCAL_NODE)


def state_of(states, group, to):
    for (g, t), v in states or ():
        if g == group and t == to:
            return v
    return NONE


# ---- the reference player ------------------------------------------------------------------------
class RefPlayer:
    """Plays a script on the oracle's router and share_ref; per "P" also what the fan-out of that
    moment looks like (for the CPU gate, which writes the route arrays itself)."""

    def __init__(self):
        self.rt, self.ref = R.Router(), SR.SharedSubRef()
        self.groups = {}   # name -> handle
        self.filters = {}  # filter bytes -> id, in order of first add_route (never reused)

    def op(self, op):
        k = op[0]
        if k == "G":
            self.ref.set_strategy(op[1], op[2])
        elif k == "S":
            self.ref.subscribe(*op[1:])
        elif k == "U":
            self.ref.unsubscribe(*op[1:])
        elif k == "C":
            self.ref.commit()
        elif k == "RA":
            self.filters.setdefault(op[1], len(self.filters))
            if not isinstance(op[2], str):
                self.groups[gname(op[2])] = op[2]
            self.rt.add_route(op[1], _dest(op[2]))
        elif k == "RD":
            self.rt.delete_route(op[1], _dest(op[2]))
        elif k == "RC":
            pass
        elif k == "P":
            return self.publish(op[1], op[2])
        else:
            raise ValueError(op)

    def publish(self, topics, msgs):
        out = []
        for t, (hc, ht, draw, states) in zip(topics, msgs):
            entries, _ = R.publish(self.rt, t, LOCAL_NODE, {})
            row = []
            for to, dest in entries:
                if isinstance(dest, str):
                    row.append((to, dest, NOT_SHARED_ANSWER))
                else:
                    g = self.groups[dest]
                    row.append((to, g, self.ref.pick(g, to, hc, ht, draw, state_of(states, g, to))))
            out.append(row)
        return out


def run_ref(script):
    p = RefPlayer()
    return [r for r in (p.op(op) for op in script) if r is not None]


def canon(result):
    """An answer with each topic's entries sorted: the reference's entries are a set (route/2)."""
    return [sorted(row, key=lambda e: (e[0], str(e[1]))) for row in result]


def same_as_ref(play, script, **kw):
    """Plays the script and asserts every answer equal to the reference's; -> (got, ref)."""
    got, ref = play(script, **kw), run_ref(script)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        g, r = canon(g), canon(r)
        assert len(g) == len(r), (k, len(g), len(r))
        bad = [i for i in range(len(r)) if g[i] != r[i]]
        assert not bad, (k, len(bad), bad[:3], [(g[i], r[i]) for i in bad[:3]])
    return got, ref


# ---- the text the CPU gate reads (tests/host_harness/pubshare_dev_main.cpp) ----------------------
def _hex(b):
    return bytes(b).hex() or "-"


def input_text(script, hash_bits=0, chunk=0):
    """The share operations as they are; per "P" the filter string pool and, per topic, the entries
    of the reference's fan-out as (filter id, dest word) and the state list as (group, filter id,
    value) -- a To that is no filter is dropped, as the callers of the C-ABI drop it."""
    p = RefPlayer()
    lines = ["%d %d" % (hash_bits, chunk)]
    for op in script:
        k = op[0]
        if k == "G":
            lines.append("G %d %d" % (NONE if op[1] is None else op[1], op[2]))
        elif k == "S":
            lines.append("S %d %s %d %d" % (op[1], _hex(op[2]), op[3], int(op[4])))
        elif k == "U":
            lines.append("U %d %s %d" % (op[1], _hex(op[2]), op[3]))
        elif k == "C":
            lines.append("C")
        if k != "P":
            p.op(op)
            continue
        topics, msgs = op[1], op[2]
        filters = sorted(p.filters, key=p.filters.get)
        absent = all(m[3] is None for m in msgs)
        lines.append("P %d %d %d" % (len(topics), len(filters), 0 if absent else 1))
        lines.append(" ".join(_hex(f) for f in filters) if filters else "")
        for t, (hc, ht, draw, states) in zip(topics, msgs):
            entries, _ = R.publish(p.rt, t, LOCAL_NODE, {})
            ent = []
            for to, dest in entries:
                d = 0 if dest == LOCAL_NODE else 1 if isinstance(dest, str) else 0x80000000 | p.groups[dest]
                ent += [p.filters[to], d]
            st = []
            for (g, to), v in states or ():
                if to in p.filters:
                    st += [g, p.filters[to], v]
            lines.append(" ".join(str(v) for v in [hc, ht, draw, len(ent) // 2, len(st) // 3] + ent + st))
        p.op(op)  # (the counters move on as in the program)
    lines.append("E")
    return "\n".join(lines) + "\n"


def parse_output(text, script):
    """The program's quadruples, in the reference's entry order, back into the script's answers."""
    lines = [ln for ln in text.splitlines() if ln and not ln.startswith("#")]
    ref, at, out = run_ref(script), 0, []
    for res in ref:
        got = []
        for row in res:
            got.append([(to, dest, tuple(int(v) for v in lines[at + j].split())) for j, (to, dest, _) in enumerate(row)])
            at += len(row)
        out.append(got)
    assert at == len(lines), (at, len(lines))
    return out


# ---- inputs --------------------------------------------------------------------------------------
def count_script(n, layout):
    """n entries in one pass, across the work-group edges: "spread" one entry per topic, "one" all
    in one topic (n groups on one filter), "gaps" one per topic with an empty row first, last and
    between every two."""
    script = [("G", None, SR.RANDOM)]
    if layout == "one":
        for g in range(n):
            script += [("RA", b"c/one", g), ("S", g, b"c/one", 2 * g + 1, True), ("S", g, b"c/one", 2 * g + 2, False)]
        script += [("RA", b"c/other", "n2"), ("C",), ("RC",)]
        topics = [b"c/one"] if n else [b"c/none"]
    else:
        script += [("RA", b"c/+", 3)] + [("S", 3, b"c/+", s, s % 2 == 0) for s in range(1, 6)] + [("C",), ("RC",)]
        topics = [b"c/x"] * n
        if layout == "gaps":
            topics = [b"none"] + [t for hit in topics for t in (hit, b"none")]
    msgs = [(i, 0, i * 2654435761 % 2 ** 32, None) for i in range(len(topics))]
    return script + [("P", topics, msgs)]


def to_length_script():
    """Keys (To) of every length; the same bytes under two groups; two filters under one group."""
    tos = [bytes(97 + (i * 7 + n) % 26 for i in range(n)) for n in TO_LENGTHS]
    script, sub = [("G", None, SR.HASH_CLIENTID)], 1
    for to in tos + [b"#"]:
        for g in (1, 2):
            script.append(("RA", to, g))
            for _ in range(2 + (g == 2)):
                script.append(("S", g, to, sub, True))
                sub += 1
    # keys that differ from a To in their last byte or their length have members but no route
    script += [("S", 1, tos[4][:-1] + b"!", 900, True), ("S", 1, tos[3][:-1], 901, True), ("S", 3, tos[0], 902, True)]
    script += [("C",), ("RC",)]
    topics = [t for t in tos + [tos[5][:-1], b"zz"] for _ in range(3)]
    return script + [("P", topics, [(i, 0, 0, None) for i in range(len(topics))])]


def strategy_script():
    """Every strategy (group = its code) over keys of every size and locality mix, hc, ht, draw and
    the round_robin state at their edges.  A key of size 0 is a group route with no share key."""
    script, topics, msgs = [], [], []
    for strat in range(7):
        script.append(("G", strat, strat))
        for si, size in enumerate(SC.SIZES):
            for mi, mix in enumerate(SC.MIXES):
                to = b"s/%d/%d/%s" % (strat, size, mix.encode())
                script.append(("RA", to, strat))
                for sub, local in SC.members_of(size, mix, 1000 * si + 100 * mi + 1):
                    script.append(("S", strat, to, sub, local))
                for v in SC.edge_values(size):
                    cases = [(v, 12345, 777, None), (12345, v, 777, [((strat, to), 3)])]
                    cases += [(12345, 777, v, [((strat, to), st)]) for st in SC.edge_states(size)]
                    topics += [to] * len(cases)
                    msgs += cases
    return script + [("C",), ("RC",), ("P", topics, msgs)]


def state_script():
    """The state list: empty, the pair alone, after 40 others, a pair of the same group and another
    filter, the same pair twice (the first wins), a To that is no filter; values at their edges.
    Then a call that passes no list at all."""
    g, to, count = 4, b"st/a", 5
    script = [("G", g, SR.ROUND_ROBIN), ("RA", to, g), ("RA", b"st/b", g), ("RA", b"st/+", "n2")]
    script += [("S", g, t, s, True) for t in (to, b"st/b") for s in range(1, count + 1)] + [("C",), ("RC",)]
    others = [((g + 1 + i % 3, b"st/b" if i % 2 else to), i) for i in range(40)]
    lists = [[], [((g, to), 2)], others + [((g, to), 2)], [((g, b"st/b"), 2)], [((g, to), 1), ((g, to), 3)],
             [((g, b"st/nofilter"), 2)], [((g + 1, to), 2)]]
    lists += [[((g, to), v)] for v in (NONE, 0, count - 1, count, 2 ** 32 - 2)]
    topics = [to] * len(lists) + [b"st/b", b"none"]
    msgs = [(1, 2, 7, st) for st in lists] + [(1, 2, 7, [((g, b"st/b"), 4), ((g, to), 0)]), (1, 2, 7, [((g, to), 0)])]
    return script + [("P", topics, msgs), ("P", topics[:3], [(1, 2, 9, None)] * 3)]


def rr_group_script(n=513):
    """round_robin_per_group: one key hit from n topics of one call (every third topic also hits a
    second key, every fifth none) takes consecutive values in entry order; a second call goes on
    from there."""
    script = [("G", 2, SR.RR_PER_GROUP), ("G", 6, SR.HASH_TOPIC), ("RA", b"rr/+", 2), ("RA", b"rr/3", 2), ("RA", b"rr/+", 6),
              ("RA", b"rr/+", "n1")]
    script += [("S", 2, b"rr/+", s, True) for s in (1, 2, 3)] + [("S", 2, b"rr/3", s, False) for s in (11, 12)]
    script += [("S", 6, b"rr/+", s, True) for s in (21, 22)] + [("C",), ("RC",)]
    topics = [b"none" if i % 5 == 4 else b"rr/3" if i % 3 == 0 else b"rr/1" for i in range(n)]
    msgs = [(i, i, i, None) for i in range(n)]
    return script + [("P", topics, msgs), ("P", topics[:7], msgs[:7])]


def mutation_script():
    """A share commit between two calls changes the pick; a deleted group route, after its commit,
    removes the entry; a share key with no route is never answered."""
    script = [("G", 1, SR.HASH_CLIENTID), ("RA", b"m/a", 1), ("RA", b"m/+", 1), ("RA", b"m/x", "n1"),
              ("S", 1, b"m/a", 1, True), ("S", 1, b"m/a", 2, True), ("S", 1, b"m/+", 3, True),
              ("S", 1, b"m/x", 7, True), ("S", 1, b"m/x", 8, True),  # members, but no group route on m/x
              ("C",), ("RC",)]
    topics = [b"m/a", b"m/x", b"m/a"]
    msgs = [(0, 0, 0, None), (1, 0, 0, None), (1, 0, 0, None)]
    script += [("P", topics, msgs)]
    script += [("U", 1, b"m/a", 1), ("S", 1, b"m/a", 4, False), ("P", topics, msgs),  # pending: invisible
               ("C",), ("P", topics, msgs)]
    script += [("RD", b"m/a", 1), ("RC",), ("P", topics, msgs)]
    script += [("RA", b"m/a", 1), ("RC",), ("U", 1, b"m/+", 3), ("C",), ("P", topics, msgs)]
    return script


def random_script(seed=20261):
    """44 filters (plain and wildcard) with node and group routes over 9 groups (one per strategy,
    two on the default), share keys of 0 to 20 members, 700 topics."""
    rng = random.Random(seed)
    script = [("G", g, g) for g in range(7)] + [("G", None, SR.LOCAL)]
    words = [b"a", b"b", b"c", b"dd"]
    filters = [b"#", b"+/+", b"a/#", b"a/+/c", b"+/b/#", b"zzz"]
    while len(filters) < 44:
        f = b"/".join(rng.choice(words + [b"+"]) for _ in range(rng.randrange(1, 4)))
        f += rng.choice((b"", b"", b"/#"))
        if f not in filters:
            filters.append(f)
    sub, keys = 1, []
    for f in filters:
        if rng.random() < 0.5:
            script.append(("RA", f, rng.choice(("n1", "n2"))))
        for g in rng.sample(range(9), rng.choice((0, 1, 1, 2, 3))):
            script.append(("RA", f, g))
            keys.append((g, f))
            n = rng.choice((0, 1, 1, 2, 3, 5, 20))  # 0: a group route with no share key
            for _ in range(n):
                script.append(("S", g, f, sub, rng.random() < 0.4))
                sub += 1
    script += [("C",), ("RC",)]
    topics, msgs = [], []
    for i in range(700):
        t = b"$none/x" if i % 50 == 0 else b"/".join(rng.choice(words) for _ in range(rng.randrange(1, 4)))
        states = None
        if rng.random() < 0.7:
            states = [(rng.choice(keys), rng.choice((NONE, rng.randrange(25)))) for _ in range(rng.randrange(0, 6))]
            if rng.random() < 0.1:
                states.append(((rng.randrange(9), b"no/such/filter"), 1))
        topics.append(t)
        msgs.append((rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), states))
    return script + [("P", topics, msgs)]


def strategy_of(script):
    """group -> strategy code as the script's "G" operations leave it (None: the default)."""
    return {op[1]: op[2] for op in script if op[0] == "G"}


ALL_SCRIPTS = {
    "to_lengths": to_length_script, "strategies": strategy_script, "states": state_script, "rr_group": rr_group_script,
    "mutations": mutation_script, "random": random_script,
}
