"""The inputs of the shared-subscription tests, one set for the reference alone
(tests/test_share_ref_cpu.py), the CPU gate (tests/test_share_dev_host.py) and the device
(tests/test_gpu_share.py), and the checks the last two share.

A script is a list of operations:
  ("S", group, topic, sub, local)   subscribe        ("U", group, topic, sub)   unsubscribe
  ("D", sub)                        subscriber_down  ("G", group | None, strategy)  set_strategy
  ("C",)                            commit           ("T", key, value)          tune
  ("R",)                            the refused calls, each of which must fail and change nothing
  ("Q", [(group, topic, hc, ht, draw, state)])   pick  -> [(member, status, state, Count)]
  ("M", group, topic)               members -> [(sub, local)]
  ("K", group, topic)               counter -> int | None
  ("X",)                            stats   -> dict (the reference answers None)
A player takes (script, hash_bits, pass_names) and returns the results of Q, M, K and X in order.
"""
import random

import share_ref as R

NONE = R.NONE
STAT_KEYS = ("keys", "slots", "deleted", "max_chain", "members", "live_words", "garbage_words",
             "load_rebuilds", "garbage_rebuilds", "growths", "counters", "pending")
SIZES = (0, 1, 2, 3, 7, 64, 65)
MIXES = ("all_local", "none_local", "mixed")
TOPIC_LENGTHS = (0, 1, 7, 8, 9, 64, 300)
BATCH_SIZES = (0, 1, 255, 256, 257, 513)


# ---- players ----------------------------------------------------------------------------------
def run_ref(script):
    ref, out = R.SharedSubRef(), []
    for op in script:
        if op[0] == "S":
            ref.subscribe(*op[1:])
        elif op[0] == "U":
            ref.unsubscribe(*op[1:])
        elif op[0] == "D":
            ref.subscriber_down(op[1])
        elif op[0] == "G":
            ref.set_strategy(op[1], op[2])
        elif op[0] == "C":
            ref.commit()
        elif op[0] == "Q":
            out.append(ref.dispatch_batch(op[1]))
        elif op[0] == "M":
            out.append(ref.subscribers(op[1], op[2]))
        elif op[0] == "K":
            out.append(ref.counter(op[1], op[2]))
        elif op[0] == "X":
            out.append(None)
    return out


def run_lib(shared_sub_cls, refused, script, hash_bits=0, pass_names=0):
    """The script on emqx_amd.SharedSub (the C-ABI through ctypes)."""
    s, out = shared_sub_cls(0, hash_bits), []
    try:
        if pass_names:
            s.tune("pass_names", pass_names)
        for op in script:
            if op[0] == "S":
                s.subscribe(*op[1:])
            elif op[0] == "U":
                s.unsubscribe(*op[1:])
            elif op[0] == "D":
                s.subscriber_down(op[1])
            elif op[0] == "G":
                s.set_strategy(op[1], op[2])
            elif op[0] == "C":
                s.commit()
            elif op[0] == "T":
                s.tune(op[1], op[2])
            elif op[0] == "R":
                refused(s)
            elif op[0] == "Q":
                q = op[1]
                o = s.pick([r[0] for r in q], [r[1] for r in q], [r[2] for r in q], [r[3] for r in q],
                           [r[4] for r in q], [r[5] for r in q])
                out.append([tuple(int(v) for v in row) for row in o])
            elif op[0] == "M":
                out.append(s.members(op[1], op[2]))
            elif op[0] == "K":
                out.append(s.counter(op[1], op[2]))
            elif op[0] == "X":
                out.append(s.stats())
    finally:
        s.close()
    return out


def _hex(b):
    return bytes(b).hex() or "-"


def input_text(script, hash_bits=0, pass_names=0):
    """The script as the text tests/host_harness/share_dev_main.cpp reads."""
    lines = [f"{hash_bits} {pass_names}"]
    for op in script:
        if op[0] == "S":
            lines.append(f"S {op[1]} {_hex(op[2])} {op[3]} {int(op[4])}")
        elif op[0] == "U":
            lines.append(f"U {op[1]} {_hex(op[2])} {op[3]}")
        elif op[0] == "D":
            lines.append(f"D {op[1]}")
        elif op[0] == "G":
            lines.append(f"G {NONE if op[1] is None else op[1]} {op[2]}")
        elif op[0] == "T":
            lines.append(f"T {op[1]} {op[2]}")
        elif op[0] in ("C", "R", "X"):
            lines.append(op[0])
        elif op[0] == "Q":
            lines.append(f"Q {len(op[1])}")
            lines += [f"{g} {_hex(t)} {hc} {ht} {dr} {st}" for g, t, hc, ht, dr, st in op[1]]
        elif op[0] in ("M", "K"):
            lines.append(f"{op[0]} {op[1]} {_hex(op[2])}")
    lines.append("E")
    return "\n".join(lines) + "\n"


def parse_output(text, script):
    """The program's output back into the results of the script's Q, M, K and X."""
    lines = [ln for ln in text.splitlines() if ln and not ln.startswith("#")]
    at, out = 0, []
    for op in script:
        if op[0] == "Q":
            rows = [tuple(int(v) for v in lines[at + i].split()) for i in range(len(op[1]))]
            at += len(op[1])
            out.append(rows)
        elif op[0] == "M":
            f = lines[at].split()
            assert f[0] == "M" and int(f[1]) == len(f) - 2, lines[at]
            out.append([(int(v) & 0x7FFFFFFF, bool(int(v) >> 31)) for v in f[2:]])
            at += 1
        elif op[0] == "K":
            f = lines[at].split()
            assert f[0] == "K", lines[at]
            out.append(None if int(f[1]) == NONE else int(f[1]))
            at += 1
        elif op[0] == "X":
            f = lines[at].split()
            assert f[0] == "STATS" and len(f) == 1 + len(STAT_KEYS), lines[at]
            out.append(dict(zip(STAT_KEYS, (int(v) for v in f[1:]))))
            at += 1
    assert at == len(lines), (at, len(lines))
    return out


def same_as_ref(play, script, hash_bits=0, pass_names=0):
    """Plays the script and asserts every answer equal to the reference's; -> (got, ref)."""
    got, ref = play(script, hash_bits, pass_names), run_ref(script)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        if r is None:
            continue
        if isinstance(r, list) and len(r) > 8:
            bad = [i for i in range(max(len(g), len(r))) if i >= len(g) or i >= len(r) or tuple(g[i]) != tuple(r[i])]
            assert not bad, (k, len(bad), bad[:5], [(g[i], r[i]) for i in bad[:5] if i < len(g) and i < len(r)])
        else:
            assert g == r, (k, g, r)
    return got, ref


# ---- inputs -----------------------------------------------------------------------------------
def members_of(size, mix, base):
    """`size` members from handle `base` on: (sub, local)."""
    local = {"all_local": lambda i: True, "none_local": lambda i: False, "mixed": lambda i: i % 3 == 1}[mix]
    return [(base + i, local(i)) for i in range(size)]


def edge_values(count):
    return sorted({0, max(count - 1, 0), count, 2 ** 27 - 1, 2 ** 32 - 1})


def edge_states(count):
    return [NONE, 0, max(count - 2, 0), max(count - 1, 0), count + 5]


def strategy_script():
    """Every strategy against keys of every size and locality mix, the hash inputs and the
    round_robin state at their edges."""
    script, q = [], []
    for strat in range(7):
        script.append(("G", strat, strat))  # group = strategy code
        for si, size in enumerate(SIZES):
            for mi, mix in enumerate(MIXES):
                topic = b"s/%d/%s" % (size, mix.encode())
                for sub, local in members_of(size, mix, 1000 * si + 100 * mi + 1):
                    script.append(("S", strat, topic, sub, local))
                for v in edge_values(size):
                    q.append((strat, topic, v, 12345, 777, NONE))
                    q.append((strat, topic, 12345, v, 777, 3))
                    for st in edge_states(size):
                        q.append((strat, topic, 12345, 777, v, st))
    script += [("C",), ("Q", q), ("X",)]
    for size in SIZES:
        script.append(("K", R.RR_PER_GROUP, b"s/%d/mixed" % size))
    return script


def topic_script():
    """Topics of every length; the same bytes under two groups; one group under two topics; the
    wildcard characters as plain bytes."""
    topics = [bytes((97 + (i * 7 + n) % 26) for i in range(n)) for n in TOPIC_LENGTHS] + [b"+", b"#", b"a/#", b"a/+"]
    script, q, sub = [("G", None, R.HASH_CLIENTID)], [], 1
    for g in (1, 2):
        for t in topics:
            for _ in range(2):
                script.append(("S", g, t, sub, True))
                sub += 1
    script.append(("C",))
    for g in (1, 2, 3):
        for t in topics + [b"a", b"a/", topics[6][:-1], topics[6] + b"x", topics[3][:-1] + b"\x00"]:
            q += [(g, t, 0, 0, 0, NONE), (g, t, 1, 0, 0, NONE)]
    script.append(("Q", q))
    script += [("M", 1, topics[0]), ("M", 2, topics[6]), ("M", 3, topics[1])]
    return script


def mutation_script():
    """Absent keys, an emptied key, a member moved to the end by unsubscribe and subscribe, a
    duplicate subscribe, subscriber_down of a member of 40 keys, a key stored again after its
    delete, pending mutations invisible before the commit."""
    keys = [(7, b"m/%d" % i) for i in range(40)]
    q = [(g, t, hc, 0, 0, NONE) for g, t in keys + [(7, b"m/absent"), (8, b"m/0")] for hc in (0, 1, 2)]
    script = [("G", 7, R.HASH_CLIENTID)]
    for g, t in keys:
        script += [("S", g, t, 1, True), ("S", g, t, 2, False), ("S", g, t, 3, True)]
    script += [("Q", q), ("C",), ("Q", q), ("M", 7, b"m/5")]
    script += [("U", 7, b"m/0", 1), ("S", 7, b"m/0", 1, True),  # moved to the end
               ("S", 7, b"m/1", 2, False),                      # a duplicate keeps its place
               ("U", 7, b"m/2", 1), ("U", 7, b"m/2", 2), ("U", 7, b"m/2", 3),  # emptied
               ("U", 7, b"m/absent", 9), ("Q", q), ("C",), ("Q", q),
               ("M", 7, b"m/0"), ("M", 7, b"m/1"), ("M", 7, b"m/2"), ("X",)]
    script += [("D", 2), ("C",), ("Q", q), ("M", 7, b"m/3"), ("X",)]
    script += [("S", 7, b"m/2", 5, False), ("S", 7, b"m/2", 2, True), ("C",), ("Q", q), ("M", 7, b"m/2")]
    script += [("D", 1), ("D", 3), ("D", 5), ("C",), ("Q", q), ("X",)]
    script += [("D", 2), ("S", 7, b"m/9", 2, False), ("C",), ("Q", q), ("X",)]
    return script


def golden_rr_script(split):
    """t_round_robin_per_group_even_distribution_one_group and _two_groups: ten messages alternate
    over two members per group, message 0 to the first; in one call or one call per message."""
    script = [("G", None, R.RR_PER_GROUP)]
    script += [("S", 1, b"foo/bar", 10, True), ("S", 1, b"foo/bar", 11, True),
               ("S", 2, b"foo/bar", 12, True), ("S", 2, b"foo/bar", 13, True), ("C",)]
    q = [(g, b"foo/bar", i, i, i, NONE) for i in range(10) for g in (1, 2)]
    script += [("Q", [r]) for r in q] if split else [("Q", q)]
    script += [("K", 1, b"foo/bar"), ("K", 2, b"foo/bar")]
    return script


def counter_script():
    """round_robin_per_group: reset by a subscribe (a duplicate one too), wrap, a counter above
    Count after members left, the one-member shortcut, a strategy switched to and from it between
    commits, the counter of an emptied key."""
    t = b"c/t"
    one = [(4, t, 0, 0, 0, NONE)]
    script = [("G", 4, R.RR_PER_GROUP)]
    script += [("S", 4, t, i, True) for i in (1, 2, 3, 4, 5)]
    script += [("C",), ("K", 4, t), ("Q", one * 4), ("K", 4, t)]           # 1 2 3 4
    script += [("U", 4, t, 4), ("U", 4, t, 5), ("U", 4, t, 3), ("C",), ("K", 4, t),  # counter 4 > Count 2
               ("Q", one * 3), ("K", 4, t)]                                # 1 2 1: wrap
    script += [("S", 4, t, 2, True), ("C",), ("K", 4, t), ("Q", one), ("K", 4, t)]   # a duplicate resets
    script += [("U", 4, t, 2), ("C",), ("Q", one * 2), ("K", 4, t)]        # one member: counter untouched
    script += [("G", 4, R.RANDOM), ("S", 4, t, 6, False), ("C",), ("K", 4, t), ("Q", one * 2), ("K", 4, t)]
    script += [("G", 4, R.RR_PER_GROUP), ("C",), ("Q", one * 3), ("K", 4, t)]
    script += [("G", 4, R.HASH_TOPIC), ("U", 4, t, 1), ("U", 4, t, 6), ("C",), ("K", 4, t), ("Q", one),
               ("S", 4, t, 7, True), ("S", 4, t, 8, True), ("G", 4, R.RR_PER_GROUP), ("C",), ("K", 4, t),
               ("Q", one * 2), ("K", 4, t)]                               # the old counter was never deleted
    script += [("U", 4, t, 7), ("U", 4, t, 8), ("C",), ("K", 4, t), ("Q", one)]
    # the default strategy governs groups that have none set
    script += [("S", 5, t, 1, True), ("S", 5, t, 2, True), ("G", None, R.RR_PER_GROUP), ("C",), ("Q", [(5, t, 0, 0, 0, NONE)] * 3),
               ("G", None, R.ROUND_ROBIN), ("C",), ("Q", [(5, t, 0, 0, 0, 0), (5, t, 0, 0, 1, NONE)]), ("K", 5, t)]
    return script


def random_case(seed=20260):
    """300 keys over 9 groups (one per strategy and two with the default), 4,007 requests."""
    rng = random.Random(seed)
    script = [("G", g, g) for g in range(7)] + [("G", None, R.LOCAL)]
    keys, sub = [], 1
    for k in range(300):
        g = k % 9
        t = b"r/%d/%s" % (k, bytes(rng.randrange(97, 123) for _ in range(rng.choice((0, 1, 3, 9, 30)))))
        n = rng.choice((1, 1, 2, 2, 3, 5, 8, 20))
        keys.append((g, t))
        for _ in range(n):
            script.append(("S", g, t, sub, rng.random() < 0.4))
            sub += 1
    script.append(("C",))
    q = []
    for _ in range(4007):
        if rng.random() < 0.15:
            g, t = rng.randrange(9), b"r/none/%d" % rng.randrange(50)
        else:
            g, t = rng.choice(keys)
        st = rng.choice((NONE, rng.randrange(25)))
        q.append((g, t, rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), st))
    script += [("Q", q), ("X",)]
    return script


def big_script(n_keys=70000):
    """70,000 keys stored in commits of 1, 300 and the rest, which forces table growths; then half
    of them rewritten, which forces a garbage rebuild; then the random requests."""
    rng = random.Random(7)
    keys = [(k % 5, b"big/%d" % k) for k in range(n_keys)]
    script = [("G", None, R.HASH_CLIENTID)]
    for lo, hi in ((0, 1), (1, 301), (301, n_keys)):
        for k in range(lo, hi):
            g, t = keys[k]
            script += [("S", g, t, 2 * k + 1, True), ("S", g, t, 2 * k + 2, False)]
        script += [("C",), ("X",)]
    for k in range(0, n_keys, 2):
        g, t = keys[k]
        script.append(("S", g, t, 3 * n_keys + k, True))
    script += [("T", "rebuild_garbage_pct", 30), ("C",), ("X",)]
    q = []
    for _ in range(4007):
        g, t = rng.choice(keys) if rng.random() < 0.85 else (rng.randrange(5), b"big/x%d" % rng.randrange(99))
        q.append((g, t, rng.getrandbits(32), 0, 0, NONE))
    script += [("Q", q)]
    return script


def block_script(n):
    script = [("G", None, R.RANDOM)] + [("S", 1, b"b/%d" % k, 10 * k + i, True) for k in range(5) for i in range(k + 1)]
    script += [("C",), ("Q", [(1, b"b/%d" % (i % 6), 0, 0, i * 2654435761 % 2 ** 32, NONE) for i in range(n)])]
    return script


# ---- checks shared by the CPU gate and the device test ---------------------------------------
def check_strategies(play):
    got, ref = same_as_ref(play, strategy_script())
    answers = ref[0]
    # the one-member shortcut leaves the counter where the subscribe set it
    assert ref[2 + SIZES.index(1)] == 0 and got[2 + SIZES.index(1)] == 0  # set by the subscribe, never stepped
    assert any(a[1] == R.HOST_STRATEGY for a in answers) and any(a[1] == R.NO_SUBSCRIBERS for a in answers)


def unstaged(script):
    """The script with the topics hashed from global memory ("stage_lds" 0) instead of from the
    block's LDS copy, the default."""
    return [("T", "stage_lds", 0)] + script


def long_topic_script():
    """300 requests of 300-byte topics: the first block's bytes pass the staging buffer, the
    second block's fit."""
    t = bytes(97 + i % 26 for i in range(300))
    script = [("G", None, R.HASH_CLIENTID), ("S", 1, t, 1, True), ("S", 1, t, 2, True), ("S", 1, t[:-1] + b"!", 3, True),
              ("C",)]
    return script + [("Q", [(1, t if i % 3 else t[:-1] + b"!", i, 0, 0, NONE) for i in range(300)])]


def check_topics(play, hash_bits, stage=True):
    same_as_ref(play, topic_script() if stage else unstaged(topic_script()), hash_bits)
    same_as_ref(play, long_topic_script() if stage else unstaged(long_topic_script()), hash_bits)


def check_mutations(play, hash_bits):
    got, _ = same_as_ref(play, mutation_script(), hash_bits)
    stats = [g for g in got if isinstance(g, dict)]
    assert stats[0]["keys"] == 39 and stats[0]["deleted"] == 1 and stats[0]["members"] == 39 * 3
    assert stats[1]["members"] == 39 * 2
    assert stats[2]["keys"] == 1 and stats[2]["members"] == 1  # m/2 keeps the member subscribed after its down
    assert stats[3]["keys"] == 1 and stats[3]["members"] == 1 and stats[3]["pending"] == 0


def check_golden_rr(play, split):
    got, _ = same_as_ref(play, golden_rr_script(split))
    rows = [r for g in got[:-2] for r in g]
    assert [r[0] for r in rows[0::2]] == [10, 11] * 5 and [r[0] for r in rows[1::2]] == [12, 13] * 5
    assert got[-2:] == [2, 2]


def check_counters(play):
    same_as_ref(play, counter_script())


def check_random(play, hash_bits, pass_names=0, stage=True):
    got, _ = same_as_ref(play, random_case() if stage else unstaged(random_case()), hash_bits, pass_names)
    return got


def check_block(play, n):
    same_as_ref(play, block_script(n))


def check_big(play):
    got, _ = same_as_ref(play, big_script())
    stats = [g for g in got if isinstance(g, dict)]
    assert stats[0]["slots"] < stats[1]["slots"] < stats[2]["slots"] and stats[2]["keys"] == 70000
    assert stats[2]["load_rebuilds"] >= 1 and stats[2]["garbage_rebuilds"] == 0
    assert stats[3]["garbage_rebuilds"] >= 1 and stats[3]["members"] == 70000 * 2 + 35000


def check_refused(play):
    """The refused calls change nothing: the same answers before and after."""
    base = random_case()
    q = base[-2]
    got, _ = same_as_ref(play, base[:-1] + [("S", 1, b"pending", 1, True), ("R",), q, ("C",), ("M", 1, b"pending")])
    keep = [i for i, r in enumerate(q[1]) if r[0] != R.RR_PER_GROUP]  # (those counters move on)
    assert [got[0][i] for i in keep] == [got[1][i] for i in keep] and got[2] == [(1, True)]
