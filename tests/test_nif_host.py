"""The NIF (c_src/emqx_trie_gpu_nif.c) linked and run on the CPU, under AddressSanitizer + UBSan
(with LeakSanitizer) and under ThreadSanitizer.

tests/host_harness/nif_driver.c executes scripts against the NIF on the fake erl_nif runtime
(tests/nif_stub/fake_erl_nif.c).  Below the NIF are the real async layer and handle registry
(emqx_amd/csrc/gm_async.cpp), the oracle-backed mock engine (tests/host_harness/mock_engine.h) and
null stubs for the other families (tests/host_harness/nif_driver_mock.cpp).  Stand-alone
executables, built by the recipe of tests/host_build.py and tests/test_async_harness.py; nothing
is loaded into Python.  Every expectation comes from oracle/emqx_ref.py (tests/nif_cases.py)."""
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import nif_cases as C  # noqa: E402
from nif_terms import Atom, Improper, Pid, Ref, Res, Var, decode, encode  # noqa: E402

ROOT = host_build.ROOT
H = host_build.H
STUB = os.path.join(ROOT, "tests", "nif_stub")
C_SRCS = [os.path.join(ROOT, "c_src", "emqx_trie_gpu_nif.c"), os.path.join(STUB, "fake_erl_nif.c"),
          os.path.join(H, "nif_driver.c")]
CXX_SRCS = [os.path.join(H, "nif_driver_mock.cpp"), os.path.join(ROOT, "emqx_amd", "csrc", "gm_async.cpp"),
            os.path.join(ROOT, "oracle", "ref_trie.cpp")]
DEPS = C_SRCS + CXX_SRCS + [os.path.join(ROOT, "include", "emqx_gpumatch.h"), os.path.join(H, "mock_engine.h"),
                            os.path.join(STUB, "erl_nif.h"), os.path.join(STUB, "fake_erl_nif.h"),
                            os.path.join(ROOT, "emqx_amd", "csrc", "gm_internal.h")]
CLANG = "/opt/rocm/llvm/bin/clang"
tsan = pytest.mark.skipif(not os.path.exists(CLANG), reason="clang (ThreadSanitizer runtime) absent")
SANS = ["asan", pytest.param("tsan", marks=tsan)]


def build(san):
    """The NIF is C (it is not valid C++): compiled as C, then linked with the C++ parts."""
    out = os.path.join(H, "build", "nif_driver_" + san)
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in DEPS):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cc, cxx = ("gcc", "g++") if san == "asan" else (CLANG, CLANG + "++")
    objs = []
    for src in C_SRCS:
        obj = os.path.join(H, "build", "nif_%s_%s.o" % (san, os.path.basename(src)[:-2]))
        r = subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-pthread"] + host_build.SAN[san] +
                           ["-I", STUB, "-I", os.path.join(ROOT, "include"), "-c", src, "-o", obj],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-4000:]
        objs.append(obj)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-DGM_DELIVER_MIN=4", "-Wno-subobject-linkage"] +
                       host_build.SAN[san] + objs + CXX_SRCS + ["-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return out


def run(san, script, timeout=300):
    return C.run(build(san), script, timeout=timeout, env=host_build.ENV)


def test_term_text_round_trip():
    terms = [Atom("ok"), Atom("n0@host"), Atom("Needs Quotes"), 0, -7, 2 ** 63 + 5, 0.5, -1e22, 3.0, b"", b"a/\x00\xff",
             (), (Atom("a"),), [], [1, [2, (b"x", Atom("true"))]], Improper([1, 2], Atom("t")),
             {Atom("k"): 1, b"b": [Atom("v")]}, {}, Ref(12), Pid(3), Res("emqx_trie_gpu_call", 9), Var("R_1")]
    for t in terms + [terms]:
        assert decode(encode(t)) == t, t
    assert encode(decode("{ a , [ <<6162>> | &4 ] , #{ k => 1.5e-07 } }")) == "{a,[<<6162>>|&4],#{k=>1.5e-07}}"


def test_driver_echoes_terms():
    """The driver's parser and printer agree with nif_terms: register/3 copies a term into a handle
    table and publish_async hands it back."""
    terms = [Atom("n@h"), (Atom("t"), -3, 2 ** 64 - 1, 0.25, b"\x00\xff", [1, 2], Improper([1], 2), {Atom("k"): b"v"}, Pid(5), Ref(77))]
    s = C.Script()
    s.call("open", [[0], 64, 4096, 200, 8, {Atom("publish"): C.TRUE, Atom("eager"): C.TRUE}], bind="R")
    s.call("route_sync", [Var("R"), [(b"", C.TRUE)]])  # the only filter: id 0 -> node 0, subscriber 0
    s.call("register", [Var("R"), Atom("node"), [(0, terms[0])]])
    s.call("register", [Var("R"), Atom("sub"), [(0, terms[1])]])
    s.ref("X")
    s.call("publish_async", [Var("R"), b"", Var("X")], pid=2)
    m = s.recv(2, 20000)
    r = run("asan", s)
    assert r.clean(), r.tail()
    assert r.out[m][2] == (Atom("routes"), [(b"", terms[0])], [(b"", terms[1])]), r.out[m]


def test_function_table_equals_the_erlang_exports():
    """A name/arity in one and not in the other makes on_load fail in a real broker."""
    src = open(os.path.join(ROOT, "src", "emqx_trie_gpu_nif.erl")).read()
    exports = set()
    for block in re.findall(r"-export\(\[(.*?)\]\)", src, re.S):
        exports |= set(re.findall(r"([a-z_0-9]+/\d+)", block))
    r = run("asan", C.Script())
    assert r.clean(), r.tail()
    assert set(r.table) == exports, (sorted(set(r.table) - exports), sorted(exports - set(r.table)))
    assert len(r.table) == len(re.findall(r"^T ", r.stdout, re.M))  # no entry twice


def _core(name, s, tmp_path):
    if name == "match":
        return C.case_match(s)
    if name == "publish":
        return C.case_publish(s, mock=True)
    if name == "cancel":
        return C.case_cancel(s)
    return C.case_resync(s, str(tmp_path / "snapshot").encode(), mock=True)


@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("name", ["match", "publish", "cancel", "resync"])
def test_core_scenario(name, san, tmp_path):
    s = C.Script()
    check = _core(name, s, tmp_path)
    r = run(san, s)
    assert r.clean() and r.mailbox == 0, r.tail()
    check(r)


def every_entry(s):
    """One call of every table entry with valid arguments (against the mock and the null stubs),
    every resource left open: the (name, argument list) pairs in call order."""
    V = Var
    a = Atom
    s.call("open", [[0], 64, 4096, 200, 8, {a("publish"): C.TRUE, a("eager"): C.TRUE, a("fail_threshold"): 0}], bind="R")
    s.call("retain_open", [0, [[1, 2], [3]]], bind="T")
    s.call("ruleset_open", [0, 0], bind="S")
    s.call("acl_open", [0, 0], bind="L")
    s.call("acldb_open", [0, 0], bind="D")
    s.call("share_open", [0, 0], bind="H")
    s.call("route_sync", [V("R"), [(b"a/+", C.TRUE), (b"b", C.FALSE)]])
    s.call("route_set", [V("R"), b"a", C.TRUE])
    s.call("route_set_many", [V("R"), [b"a", b"b/#"], C.TRUE])
    s.call("route_dests", [V("R"), [(b"a", [(0, C.NONE), (1, 0)]), (b"c", [])], C.TRUE])
    s.call("subscribers", [V("R"), [(b"a", [0, 1]), (b"c", [])], C.TRUE])
    s.call("alloc_handle", [V("R"), a("sub")])
    s.call("register", [V("R"), a("sub"), [(0, Pid(7))]])
    s.call("release_handle", [V("R"), a("sub"), 0])
    s.call("reset_handles", [V("R")])
    s.call("set_local_node", [V("R"), 0])
    s.call("sync_begin", [V("R")], bind="G")
    s.call("sync_end", [V("R"), V("G")])
    s.call("commit", [V("R")])
    s.call("snapshot_save", [V("R"), b"/nowhere/snapshot"])
    s.call("snapshot_load", [V("R"), b"/nowhere/snapshot"])
    s.call("empty", [V("R")])
    s.call("trie_member", [V("R"), b"a/+"])
    s.call("route_member", [V("R"), b"a"])
    s.ref("X")
    s.call("match_async", [V("R"), b"a/b", V("X")], pid=2, bind="K")
    s.recv(2, 20000)
    s.call("publish_async", [V("R"), b"a/b", V("X")], pid=2)
    s.recv(2, 20000)
    s.call("cancel", [V("R"), V("K")], pid=2)
    s.call("tune", [V("R"), a("spin_us"), 0])
    s.call("stats", [V("R")])
    s.call("retain_store", [V("T"), b"a/b", 0])
    s.call("retain_store", [V("T"), b"a", 0, 5])
    s.call("retain_delete", [V("T"), b"a/b"])
    s.call("retain_clean", [V("T")])
    s.call("retain_commit", [V("T")])
    s.call("retain_tune", [V("T"), a("delta_max"), 4])
    s.call("retain_match", [V("T"), [b"a/+", b"#"], 1000])
    s.call("retain_match_limit", [V("T"), [b"a/+", b"#"], 1000, [1, 0], [b"", b"\x00" * 16]])
    s.call("retain_clear_expired", [V("T"), 1000])
    s.call("retain_delete_matching", [V("T"), b"a/#"])
    s.call("retain_page_read", [V("T"), b"a/#", 1, 10, 1000])
    s.call("match_rules", [V("R"), [b"a/b", b"c"], [(b"a/+", a("words")), (b"a/b", a("eq")), (b"#", a("binary"))]])
    s.call("ruleset_set", [V("S"), [[(b"a/+", a("words"))], [], [(b"b", a("eq")), (b"#", a("binary"))]]])
    s.call("ruleset_match", [V("S"), [b"a/b", b"c"]])
    s.call("acl_set", [V("L"), [(a("allow"), a("all"), a("publish"), [(b"a/+", a("words"))]),
                                (a("deny"), (a("username"), b"u"), a("subscribe"), [(b"b", a("eq"))]),
                                (a("allow"), (a("slot"), 3), a("all"), [])]])
    s.call("acl_match", [V("L"), ([(b"c1", C.UNDEFINED, 5), (C.UNDEFINED, b"u", 0)],
                                  [(b"a/b", 0, a("publish")), (b"b", 1, a("subscribe"))])])
    s.call("acldb_store", [V("D"), a("clientid"), b"c1", [(a("allow"), a("publish"), b"a/+"), (a("deny"), a("all"), b"eq b")]])
    s.call("acldb_delete", [V("D"), a("username"), b"u"])
    s.call("acldb_purge", [V("D")])
    s.call("acldb_commit", [V("D")])
    s.call("acldb_match", [V("D"), ([(b"c1", C.UNDEFINED)], [(b"a/b", 0, a("subscribe"))])])
    s.call("share_subscribe", [V("H"), 1, b"t", 7, C.TRUE])
    s.call("share_unsubscribe", [V("H"), 1, b"t", 7])
    s.call("share_down", [V("H"), 7])
    s.call("share_strategy", [V("H"), a("default"), a("round_robin")])
    s.call("share_commit", [V("H")])
    s.call("share_pick", [V("H"), [(b"t", 1, 11, 22, 33, C.UNDEFINED), (b"t", 1, 11, 22, 33, 4)]])
    s.call("share_members", [V("H"), 1, b"t"])
    closes = [("ruleset_close", "S"), ("acl_close", "L"), ("acldb_close", "D"), ("share_close", "H")]
    for name, v in closes:
        s.last_valid[name + "/1"] = [V(v)]
    return closes


def refused(t):
    return t == C.BADARG or (isinstance(t, tuple) and len(t) == 2 and t[0] == C.ERROR)


def test_every_entry_accepts_its_valid_arguments():
    s = C.Script()
    closes = every_entry(s)
    for name, v in closes:
        s.call(name, [Var(v)])
    r = run("asan", s)
    assert r.clean() and r.mailbox == 0, r.tail()
    assert not [(line, t) for line, t in zip([ln for ln in s.lines if ln.split()[0] in ("call", "recv", "ref")], r.out)
                if refused(t) or t == C.TIMEOUT]
    assert all(n >= 1 for n in r.table.values()), [k for k, n in r.table.items() if not n]


def mutations(arg):
    bogus = Atom("bogus")
    out = [bogus, (bogus,)]
    if isinstance(arg, list):  # an improper list where a list is expected
        out.append(Improper(arg if arg else [bogus], bogus))
    return out


def test_malformed_arguments_are_refused():
    """Every table entry, its last valid argument list mutated at each position in turn to a
    wrong-typed term: badarg or {error, _}, no crash, no sanitizer report, nothing leaked."""
    s = C.Script()
    every_entry(s)
    n_valid = s.n_out
    sweep = []
    for entry, args in sorted(s.last_valid.items()):
        name = entry.split("/")[0]
        for pos in range(len(args)):
            for m in mutations(args[pos]):
                bad = args[:pos] + [m] + args[pos + 1:]
                sweep.append((entry, pos, m, s.call(name, bad, pid=2, valid=False)))
    r = run("asan", s)
    assert len(s.last_valid) == len(r.table) and n_valid < s.n_out
    assert r.clean(), r.tail()
    accepted = [(e, pos, encode(m)[:60], r.out[o]) for e, pos, m, o in sweep if not refused(r.out[o])]
    assert not accepted, accepted[:20]


# entries below which no C-ABI call can fail: handle tables and the registry, a close (its destroy
# returns nothing), cancel; the async entries answer by message (checked on their own)
NO_ABI_ERROR = {"register/3", "alloc_handle/2", "release_handle/3", "reset_handles/1", "cancel/2",
                "match_async/3", "publish_async/3", "ruleset_close/1", "acl_close/1", "acldb_close/1",
                "share_close/1"}
CREATES = {"ruleset_open/2", "acl_open/2", "acldb_open/2", "share_open/2"}  # nothing but their create below


@pytest.mark.parametrize("errno_,atom", [(12, "enomem"), (5, "eio")])
def test_error_returns(errno_, atom):
    """Every entry with valid arguments while its C-ABI call returns -ENOMEM / -EIO:
    {error, enomem | eio}, and nothing leaked (LeakSanitizer and the runtime's counters)."""
    s = C.Script()
    every_entry(s)
    failed = []
    for entry, args in sorted(s.last_valid.items()):
        if entry in NO_ABI_ERROR:
            continue
        (s.rc_create if entry in CREATES else s.rc)(-errno_)
        failed.append((entry, s.call(entry.split("/")[0], args, pid=2, valid=False)))
        if entry == "retain_open/2":  # its create, too
            s.rc(0)
            s.rc_create(-errno_)
            failed.append((entry, s.call("retain_open", args, pid=2, valid=False)))
        s.rc(0)
        s.rc_create(0)
    # a window whose pass fails: every caller gets {error, Reason} as its message, once
    msgs = []
    for k, fn in enumerate(("match_async", "publish_async")):
        s.ref("F%d" % k)
        s.rc(-errno_)
        call = s.call(fn, [Var("R"), b"a/b", Var("F%d" % k)], pid=3, valid=False)
        msgs.append((call, s.recv(3, 20000)))
        s.rc(0)
    r = run("asan", s)
    assert r.clean() and r.mailbox == 0, r.tail()
    want = (C.ERROR, Atom(atom))
    wrong = [(e, r.out[o]) for e, o in failed if r.out[o] != want]
    assert not wrong, wrong
    for call, m in msgs:
        assert r.out[call][0] == C.OK and r.out[m][0] == C.MOD and r.out[m][2] == want, (r.out[call], r.out[m])


def _load_index(seed):
    rng = random.Random(seed)
    words = [b"a", b"b", b"c", b"dd", b"", b"$s"]

    def name(filt):
        out = []
        for i in range(rng.randint(1, 5)):
            k = rng.randrange(8 if filt else 6)
            if k == 6:
                out.append(b"+")
            elif k == 7:
                out.append(b"#")
                break
            else:
                out.append(words[0 if k == 5 and i else k])
        return b"/".join(out)
    filters = sorted({name(True) for _ in range(120)})
    return filters, sorted({name(False) for _ in range(60)})


@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("threads,window,calls", [(16, 64, 300), (64, 16, 200), (4, 4096, 400)])
def test_concurrent_load(threads, window, calls, san):
    """T publisher processes on T threads against one resource, with cancels at random moments and
    the handle tables written on another thread throughout: every message is the oracle's answer
    for its topic; the driver reports a call answered twice, never, or after a successful cancel,
    and a second cancel that did not return false, as violations."""
    filters, topics = _load_index(threads)
    s = C.Script()
    s.call("open", [[0, 0], window, 64 * window, 100, 8, {Atom("report_threads"): 3,
                                                          Atom("fail_threshold"): 0}], bind="R")  # cancels are no timeouts here
    s.call("route_sync", [Var("R"), [(f, C.TRUE) for f in filters]])
    s.load("R", threads, calls, 15, threads + window, topics)
    stats = s.call("stats", [Var("R")])
    r = run(san, s)
    assert r.clean() and r.mailbox == 0, r.tail()
    assert not r.violations, r.violations[:10]
    ld = r.load
    assert ld["violations"] == 0 and ld["live_calls"] == 0, ld
    assert ld["accepted"] == ld["answered"] + ld["cancelled"] and ld["accepted"] + ld["refused"] == threads * calls, ld
    assert ld["answered"] == len(r.messages) and ld["cancelled"] > 0, ld
    index = C.index_of(filters)
    want = [C.want_match(index, t) for t in topics]
    for ti, m in r.messages:
        assert C.got_match(m)[1] == want[ti], (topics[ti], m)
    st = r.out[stats]
    assert st[Atom("calls")] == ld["accepted"] and st[Atom("cancelled")] == ld["cancelled"], (st, ld)
