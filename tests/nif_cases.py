"""Scenarios for the NIF (c_src/emqx_trie_gpu_nif.c) run by tests/host_harness/nif_driver.c on the
fake erl_nif runtime: the scripts, and what each result and message must be according to the
Python references (oracle/emqx_ref.py).  Shared by the CPU gate (tests/test_nif_host.py: the real
async layer over the oracle-backed mock engine) and the device tests (tests/test_gpu_nif.py: the
engine itself).  A scenario builds its script into a Script and returns check(run), which asserts
on the driver's output; nothing here asks the engine anything through another path.

The mock engine's publish fan-out is a fixed function of the matched filter ids (see
tests/host_harness/mock_engine.h); mock_publish() below restates it, the device's comes from
emqx_ref.publish()."""
import collections
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import emqx_ref as R  # noqa: E402
from nif_terms import (Atom, Pid, Ref, Res, Var, Improper, TRUE, FALSE, OK, ERROR, BADARG,  # noqa: E402,F401
                       UNDEFINED, NONE, boolean, decode, encode)

MOD = Atom("emqx_trie_gpu")
TIMEOUT = Atom("timeout")
GM_PAR_MIN = 1024  # c_src/emqx_trie_gpu_nif.c: bulk calls of this many filters run one thread per engine


class Script:
    def __init__(self):
        self.lines = []
        self.n_out = 0
        self.last_valid = {}  # "name/arity" -> the argument list of its last call (malformed sweep)

    def _out(self):
        self.n_out += 1
        return self.n_out - 1

    def call(self, name, args, pid=1, bind="-", valid=True):
        args = list(args)
        if valid:
            self.last_valid["%s/%d" % (name, len(args))] = args
        self.lines.append("call %d %s/%d %s %s" % (pid, name, len(args), bind, encode(args)))
        return self._out()

    def recv(self, pid, ms, bind="-"):
        self.lines.append("recv %d %d %s" % (pid, ms, bind))
        return self._out()

    def ref(self, name):
        self.lines.append("ref " + name)
        return self._out()

    def drop(self, name):
        self.lines.append("drop " + name)

    def rc(self, v):
        self.lines.append("rc %d" % v)

    def rc_create(self, v):
        self.lines.append("rc_create %d" % v)

    def balance(self):
        self.lines.append("balance")

    def sleep(self, ms):
        self.lines.append("sleep %d" % ms)

    def load(self, res, threads, calls, cancel_pct, seed, topics):
        self.lines.append("load %s %d %d %d %d %s" % (res, threads, calls, cancel_pct, seed, encode(list(topics))))

    def text(self):
        return "\n".join(self.lines) + "\n"


class Run:
    """A driver run: out[i] is the term of the i-th "= " / "< " line."""

    def __init__(self, returncode, stdout, stderr):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr
        self.out, self.table, self.balances, self.messages, self.violations = [], {}, [], [], []
        self.load, self.mailbox = None, None
        cur = None
        for line in stdout.splitlines():
            tag, _, rest = line.partition(" ")
            if tag in ("=", "<"):
                self.out.append(TIMEOUT if rest == "timeout" else decode(rest))
            elif tag == "T":
                name, calls = rest.split()
                self.table[name] = int(calls)
            elif tag == "B":
                w = rest.split()
                if w[0] == "mailbox":
                    self.mailbox = int(w[1])
                    continue
                if w[0] == "res" and (cur is None or "envs" in cur):
                    cur = {}
                    self.balances.append(cur)
                cur[w[1] if w[0] == "res" else "envs"] = int(w[-1])
            elif tag == "M":
                ti, _, term = rest.partition(" ")
                self.messages.append((int(ti), decode(term)))
            elif tag == "V":
                self.violations.append(rest)
            elif tag == "LOAD":
                w = rest.split()
                self.load = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}

    def tail(self):
        return "exit %s\n%s\n%s" % (self.returncode, self.stdout[-3000:], self.stderr[-6000:])

    def clean(self):
        """The run ended by itself, with the documented balance (all zero) and no sanitizer report."""
        return (self.returncode == 0 and self.balances and not any(self.balances[-1].values())
                and "Sanitizer" not in self.stderr and "WARNING" not in self.stderr)


def run(exe, script, timeout=120, env=None):
    p = subprocess.run([exe], input=script.text() if isinstance(script, Script) else script,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    return Run(p.returncode, p.stdout, p.stderr)


# ---- the references ---------------------------------------------------------------------------
def index_of(filters):
    trie = R.Trie()
    for f in set(filters):
        if R.wildcard(f):
            trie.insert(f)
    return trie, set(filters)


def want_match(index, topic):
    trie, keys = index
    return sorted(trie.match(topic)), boolean(topic in keys)


def got_match(msg):
    assert isinstance(msg, tuple) and len(msg) == 4 and msg[0] == MOD, msg
    return msg[1], (sorted(msg[2]), msg[3])


def mock_publish(filters, topic, nodes, groups, subs):
    """The mock engine's fan-out: ids are positions in the sorted committed set."""
    ids = {f: i for i, f in enumerate(sorted(set(filters)))}
    trie, keys = index_of(filters)
    matched = ([topic] if topic in keys else []) + trie.match(topic)
    ents, dels = [], []
    for f in matched:
        i = ids[f]
        ents.append((f, nodes[i % 3]))
        if i & 1:
            ents.append((f, groups[i % 2]))
        dels.append((f, subs[i % 5]))
    return ents, dels


# ---- A. match_async ---------------------------------------------------------------------------
MAX_LEVELS = 16
LIT16 = b"/".join(b"l%d" % i for i in range(16))
A_FILTERS = [b"#", b"+/#", b"a/+", b"a/#", b"a/b", b"+/b", b"+/+/+", b"$SYS/#", b"$SYS/+", b"", b"/",
             b"a//b", LIT16, b"w/" + b"x" * 300 + b"/+"]
A_TOPICS = [b"", b"/", b"a", b"a/b", b"a//b", b"x", b"$SYS", b"$SYS/x", b"a/+", LIT16,
            b"w/" + b"x" * 300 + b"/y"]
LONGEST = b"t" * 65535  # as long as a topic can be (a call of its own: it fills a window's bytes)
A_BURSTS = (1, 1, 63, 64, 65, 129)  # LONGEST alone, then the edges of a 64-topic window


def case_match(s, devices=(0,)):
    s.call("open", [list(devices), 64, 1 << 17, 3000, MAX_LEVELS, {}], bind="A")
    sync = s.call("route_sync", [Var("A"), [(f, TRUE) for f in A_FILTERS]])
    index = index_of(A_FILTERS)
    s.ref("X0")
    too_deep = s.call("match_async", [Var("A"), LIT16 + b"/more", Var("X0")], pid=9, valid=False)
    s.ref("X1")
    too_long = s.call("match_async", [Var("A"), b"t" * 65536, Var("X1")], pid=9, valid=False)
    sent, k = [], 0
    for b, burst in enumerate(A_BURSTS):
        calls = []
        for j in range(burst):
            name, topic, pid = "M%d" % k, LONGEST if b == 0 else A_TOPICS[k % len(A_TOPICS)], 10 + k % 3
            k += 1
            calls.append((s.ref(name), s.call("match_async", [Var("A"), topic, Var(name)], pid=pid), topic, pid))
        calls = [c + (s.recv(c[3], 20000),) for c in calls]
        sent.append(calls)
    members = [(f, s.call("trie_member", [Var("A"), f]), s.call("route_member", [Var("A"), f]))
               for f in A_FILTERS + [b"nope/#", b"nope"]]
    empty = s.call("empty", [Var("A")])
    s.sleep(20)  # the layer counts a window as reported after its last message was sent
    stats = s.call("stats", [Var("A")])
    s.drop("A")

    def check(r):
        assert r.out[sync][0] == OK, r.out[sync]
        assert r.out[too_deep] == (ERROR, Atom("e2big")) and r.out[too_long] == (ERROR, Atom("e2big"))
        for calls in sent:
            by_ref, by_pid = {}, collections.defaultdict(list)
            for ref_i, call_i, topic, pid, recv_i in calls:
                assert r.out[call_i][0] == OK and isinstance(r.out[call_i][1], Res), (topic[:40], r.out[call_i])
                by_ref[r.out[ref_i]] = topic
                by_pid[pid].append(r.out[recv_i])
            for pid, msgs in by_pid.items():
                for m in msgs:
                    assert m != TIMEOUT, "a call of process %d was not answered" % pid
                    ref, got = got_match(m)
                    topic = by_ref.pop(ref)  # KeyError: answered twice, or another process's call
                    assert got == want_match(index, topic), (topic[:40], got)
            assert not by_ref
        for f, tm, rm in members:
            assert r.out[tm] == boolean(f in A_FILTERS and R.wildcard(f)), f[:40]
            assert r.out[rm] == boolean(f in A_FILTERS), f[:40]
        assert r.out[empty] == FALSE
        st = r.out[stats]
        assert st[Atom("calls")] == st[Atom("reported")] == sum(A_BURSTS), st
        assert st[Atom("too_deep")] == 1 and st[Atom("failed")] == 0 and st[Atom("cancelled")] == 0, st
    return check


# ---- B. publish_async -------------------------------------------------------------------------
NODES = [Atom("n%d@host" % i) for i in range(3)]
GROUPS = [b"g0", b"g1"]
SUB_PIDS = [Pid(100 + i) for i in range(20)]
ALL5 = [(0, NONE), (1, NONE), (2, NONE), (0, 0), (1, 1)]  # three nodes, group 0 on n0, group 1 on n1
J_CHAIN = [b"/".join([b"j"] + [b"%d" % i for i in range(d)] + [b"#"]) for d in range(13)]
K_CHAIN = [b"/".join([b"k"] + [b"%d" % i for i in range(d)] + [b"#"]) for d in range(12)]
B_ROUTES = collections.OrderedDict(
    [(b"p/#", ALL5), (b"p/+/#", ALL5), (b"p/q/#", ALL5), (b"p/q/r", [(0, NONE)]),
     (b"p/q/t", [(0, NONE), (1, NONE)]), (b"u/v", [(0, NONE)])] +
    [(f, [(0, NONE)]) for f in J_CHAIN + K_CHAIN])
B_SUBS = collections.OrderedDict(
    [(b"p/#", [0, 1, 2, 3, 4, 5]), (b"p/+/#", [6, 7, 8, 9]), (b"p/q/#", [10, 11, 12, 13, 14]),
     (b"p/q/r", [15, 16, 17]), (b"p/q/t", [18]), (b"u/v", [19]), (J_CHAIN[3], [1, 2]), (K_CHAIN[0], [3])])
B_TOPICS = [b"p/q/r", b"p/q/t", b"p/x", b"u/v", b"none", b"p",
            # 11 chain filters each, first ids of opposite parity: 16 entries for one and 17 for the other on the mock
            b"/".join([b"j"] + [b"%d" % i for i in range(10)]), b"/".join([b"k"] + [b"%d" % i for i in range(10)]),
            b"j/0/1", b"k/0"]


def ref_publish(routes, subs, sub_terms, topic):
    """emqx_ref.publish over the handle tables: entries {To, Node | Group}, deliveries {To, Pid}."""
    router = R.Router()
    for f, dests in routes.items():
        for n, g in dests:
            router.add_route(f, str(NODES[n]) if g == NONE else (GROUPS[g], str(NODES[n])))
    ents, dels = R.publish(router, topic, str(NODES[0]), {f: [sub_terms[h] for h in hs] for f, hs in subs.items()})
    return [(to, Atom(d) if isinstance(d, str) else d) for to, d in ents], dels


def case_publish(s, mock, devices=(0,)):
    s.call("open", [list(devices), 64, 1 << 16, 200, 0, {Atom("publish"): TRUE, Atom("eager"): TRUE}], bind="P")
    allocs = [(kind, i, s.call("alloc_handle", [Var("P"), Atom(kind)]))
              for kind, n in (("node", 3), ("group", 2), ("sub", 20)) for i in range(n)]
    regs = [s.call("register", [Var("P"), Atom("node"), list(enumerate(NODES))]),
            s.call("register", [Var("P"), Atom("group"), list(enumerate(GROUPS))]),
            s.call("register", [Var("P"), Atom("sub"), list(enumerate(SUB_PIDS))]),
            s.call("set_local_node", [Var("P"), 0])]
    sets = [s.call("route_dests", [Var("P"), [(f, d) for f, d in B_ROUTES.items()], TRUE]),
            s.call("subscribers", [Var("P"), [(f, h) for f, h in B_SUBS.items()], TRUE])]
    sub_terms = dict(enumerate(SUB_PIDS))

    def want(topic, subs):
        if mock:
            return mock_publish(list(B_ROUTES), topic, NODES, GROUPS, SUB_PIDS)
        return ref_publish(B_ROUTES, subs, sub_terms, topic)

    first = []
    for k, t in enumerate(B_TOPICS):
        s.ref("P%d" % k)
        first.append((t, s.call("publish_async", [Var("P"), t, Var("P%d" % k)], pid=20), s.recv(20, 20000),
                      want(t, B_SUBS)))
    # the last subscriber of u/v leaves; its handle is released and a new term gets a handle
    subs2 = collections.OrderedDict(B_SUBS)
    subs2[b"u/v"] = []
    gone = [s.call("subscribers", [Var("P"), [(b"u/v", [])], TRUE]),
            s.call("release_handle", [Var("P"), Atom("sub"), 19])]
    again = s.call("alloc_handle", [Var("P"), Atom("sub")], bind="H")
    newcomer = Pid(777)
    gone.append(s.call("register", [Var("P"), Atom("sub"), [(Var("H"), newcomer)]]))
    s.ref("PU")
    after = (s.call("publish_async", [Var("P"), b"u/v", Var("PU")], pid=20), s.recv(20, 20000))
    s.balance()
    reset = s.call("reset_handles", [Var("P")])
    s.balance()
    s.drop("H")
    s.drop("P")

    def multiset(l):
        return collections.Counter(l)

    def check(r):
        for kind, i, o in allocs:
            assert r.out[o] == (OK, i), (kind, i, r.out[o])
        assert all(r.out[o] == OK for o in regs), [r.out[o] for o in regs]
        assert all(r.out[o][0] == OK for o in sets), [r.out[o] for o in sets]
        sizes = set()
        for t, c, m, (ents, dels) in first:
            assert r.out[c][0] == OK, (t, r.out[c])
            msg = r.out[m]
            assert msg != TIMEOUT and msg[0] == MOD and msg[2][0] == Atom("routes"), (t, msg)
            got_e, got_d = msg[2][1], msg[2][2]
            assert multiset(got_e) == multiset(ents), (t, got_e, ents)
            assert multiset(got_d) == multiset(dels), (t, got_d, dels)
            assert all(UNDEFINED not in e for e in got_e + got_d), (t, msg)
            assert {to for to, _ in got_d} <= {to for to, _ in got_e}, (t, msg)
            sizes.add(len(ents))
        assert {0, 16, 17} <= sizes, sizes  # both sides of on_window's to_small[16], and no route
        assert all(r.out[o] == OK or r.out[o][0] == OK for o in gone), [r.out[o] for o in gone]
        assert r.out[again][0] == OK
        msg = r.out[after[1]]
        assert msg != TIMEOUT and r.out[after[0]][0] == OK
        ents, dels = want(b"u/v", subs2)
        assert mock or dels == []  # (the mock's fan-out ignores the tables: as before)
        assert multiset(msg[2][2]) == multiset(dels), (msg, dels)
        assert newcomer not in [d for _, d in msg[2][2]]
        assert multiset(msg[2][1]) == multiset(ents)
        assert r.out[reset] == OK
        # the terms of the handle tables: 3 + 2 + 20 environments, none after reset_handles
        assert r.balances[0]["envs"] == 25 and r.balances[1]["envs"] == 0, r.balances[:2]
    return check


# ---- C. cancel --------------------------------------------------------------------------------
WINDOW_MS = 200


def case_cancel(s, devices=(0,)):
    s.call("open", [list(devices), 64, 4096, WINDOW_MS * 1000, 8, {}], bind="C")
    s.call("route_sync", [Var("C"), [(b"c/#", TRUE)]])
    s.ref("C1")
    c1 = s.call("match_async", [Var("C"), b"c/1", Var("C1")], pid=30, bind="K1")
    x1 = s.call("cancel", [Var("C"), Var("K1")], pid=30)
    none = s.recv(30, 3 * WINDOW_MS)
    x1b = s.call("cancel", [Var("C"), Var("K1")], pid=30)
    r2 = s.ref("C2")
    c2 = s.call("match_async", [Var("C"), b"c/2", Var("C2")], pid=30, bind="K2")
    m2 = s.recv(30, 20000)
    x2 = s.call("cancel", [Var("C"), Var("K2")], pid=30)
    again = s.recv(30, WINDOW_MS + WINDOW_MS // 2)
    stats = s.call("stats", [Var("C")])
    for n in ("K1", "K2", "C"):
        s.drop(n)

    def check(r):
        assert r.out[c1][0] == OK and r.out[c2][0] == OK
        assert r.out[x1] == TRUE, "a call in the open window was not cancelled"
        assert r.out[none] == TIMEOUT, "a cancelled call was answered"
        assert r.out[x1b] == FALSE, "a second cancel of the same call"
        assert r.out[m2] == (MOD, r.out[r2], [b"c/#"], FALSE), r.out[m2]
        assert r.out[x2] == FALSE, "a call whose message was received was cancelled"
        assert r.out[again] == TIMEOUT, "a call was answered twice"
        st = r.out[stats]
        assert (st[Atom("calls")], st[Atom("cancelled")], st[Atom("outstanding")]) == (2, 1, 0), st
    return check


# ---- D. resync on two engines -----------------------------------------------------------------
def case_resync(s, snapshot_path, mock, devices=(0, 0)):
    old = [b"gone/+", b"r/5/+", b"stay"]
    new = [(b"r/%d/+" % i) if i % 2 else (b"r/%d" % i) for i in range(GM_PAR_MIN - 1 + GM_PAR_MIN)]
    new += [b"stay"]
    topics = [b"r/5/x", b"r/5", b"r/6", b"r/1501/y", b"r/2046", b"r/2047/x", b"gone/1", b"stay", b"one/x"]
    s.call("open", [list(devices), 64, 4096, 200, 8, {Atom("eager"): TRUE}], bind="D")
    s.call("tune", [Var("D"), Atom("spin_us"), 0])
    first = s.call("route_sync", [Var("D"), [(f, TRUE) for f in old]])
    begin = s.call("sync_begin", [Var("D")], bind="G")
    chunks = [s.call("route_set_many", [Var("D"), new[:GM_PAR_MIN - 1], TRUE]),
              s.call("route_set_many", [Var("D"), new[GM_PAR_MIN - 1:2 * GM_PAR_MIN - 1], TRUE]),
              s.call("route_set_many", [Var("D"), new[2 * GM_PAR_MIN - 1:], TRUE]),
              s.call("route_set", [Var("D"), b"one/#", TRUE])]
    end = s.call("sync_end", [Var("D"), Var("G")])
    commit = s.call("commit", [Var("D")])
    index = index_of(new + [b"one/#"])
    gone = s.call("route_member", [Var("D"), b"gone/+"])

    def ask(res, tag):
        out = []
        for k, t in enumerate(topics):
            name = "%s%d" % (tag, k)
            out.append((s.ref(name), s.call("match_async", [Var(res), t, Var(name)], pid=40), s.recv(40, 20000), t))
        return out
    asked = ask("D", "D")
    save = s.call("snapshot_save", [Var("D"), snapshot_path])
    s.call("open", [list(devices), 64, 4096, 200, 8, {Atom("eager"): TRUE}], bind="E")
    load = s.call("snapshot_load", [Var("E"), snapshot_path])
    asked2 = [] if mock else ask("E", "E")  # the mock has no snapshots: its stubs only answer ok
    for n in ("G", "D", "E"):
        s.drop(n)

    def check(r):
        assert r.out[first][0] == OK and r.out[begin][0] == OK, (r.out[first], r.out[begin])
        assert all(r.out[c] == OK for c in chunks), [r.out[c] for c in chunks]
        assert r.out[end] == (OK, 1), r.out[end]  # gone/+ alone was not given again
        assert r.out[commit][0] == OK, r.out[commit]
        assert r.out[gone] == FALSE
        assert r.out[save] == OK and r.out[load] == OK, (r.out[save], r.out[load])
        for ref_i, call_i, recv_i, t in asked + asked2:
            assert r.out[call_i][0] == OK, (t, r.out[call_i])
            assert r.out[recv_i] != TIMEOUT, t
            ref, got = got_match(r.out[recv_i])
            assert ref == r.out[ref_i] and got == want_match(index, t), (t, got, want_match(index, t))
    return check
