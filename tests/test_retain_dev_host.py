"""The CPU gate of the retained-topic store: the device code of
emqx_amd/csrc/gm_retain.inc -- k_retain_walk, k_retain_runs, k_retain_ptr and the limited
reads' k_retain_runs_win / k_retain_win, 64 lanes per wave with the ballot computed by the
harness -- and the host code behind the emqxgm_retain_* C-ABI (emqx_amd/csrc/gm_retain.cpp,
every "device" array an allocation of exactly the bytes in use) run under ASan + UBSan in the
stand-alone program tests/host_harness/retain_dev_main.cpp, on exactly the inputs and checks of
tests/test_gpu_retain_pages.py (tests/retain_cases.py), against tests/retain_ref.py.  It also
runs the unlimited match, so the existing kernels pass the gate too.  No GPU."""
import contextlib
import os
import random
import subprocess

import pytest

import host_build
import retain_cases as RC
import retain_ref as RR

CSRC = host_build.CSRC
H = host_build.H
SRC = os.path.join(H, "retain_dev_main.cpp")
DEPS = [SRC, os.path.join(host_build.ROOT, "include", "emqx_gpumatch.h")] + [
    os.path.join(CSRC, f) for f in ("gm_retain.cpp", "gm_retain.inc", "gm_common.h", "gm_kernels.h")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "fakehip/hip/hip_runtime.h")]


@pytest.fixture(scope="module")
def exe():
    """The harness brings its own fake runtime and launchers: one source file, no other."""
    out = os.path.join(H, "build", "retain_dev_main_asan")
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in DEPS):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + host_build.SAN["asan"] + [
        "-Wno-subobject-linkage", "-I", os.path.join(H, "fakehip"), SRC, "-pthread", "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return out


class HarnessError(Exception):
    pass


def _hex(b):
    return b.hex() or "-"


def _unhex(h):
    return b"" if h == "-" else bytes.fromhex(h)


class Harness:
    """emqx_amd.Retainer's methods over the harness program (one command, one answer)."""

    def __init__(self, exe, index_specs=RC.DEFAULT):
        self.p = subprocess.Popen([exe, "-"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True, env=host_build.ENV)
        self.slots = 0
        self.set_index_specs(index_specs)

    def _ask(self, cmd, lines=1):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        out = []
        while len(out) < lines:
            ln = self.p.stdout.readline()
            if not ln:
                raise AssertionError("the harness died:\n" + self.p.stderr.read()[-6000:])
            out.append(ln.rstrip("\n"))
            if ln.startswith("E "):
                break
        return out

    def _k(self, cmd, what):
        a = self._ask(cmd)[0].split()
        if a[0] != "K" or int(a[1]) != 0:
            raise HarnessError(f"{what} failed: {a[1]}")

    def close(self):
        """End of input: the program destroys the store and exits 0 (leaks and all checked)."""
        self.p.stdin.close()
        rc = self.p.wait(timeout=300)
        err = self.p.stderr.read()
        assert rc == 0, err[-6000:]

    def set_index_specs(self, specs):
        self._k("indices %d\n" % len(specs) + "\n".join(
            " ".join(map(str, [len(s)] + list(s))) for s in specs), "retain_set_indices")

    def tune(self, key, value):
        self._k(f"tune {key} {int(value)}", "retain_tune")

    def set_max_retained(self, limit):
        self.tune("max_retained_messages", limit)

    def store_retained(self, topic, expiry_ms=0, ts_ms=0):
        a = self._ask(f"store {_hex(topic)} {expiry_ms} {ts_ms}")[0].split()
        if int(a[1]) == -28:
            return None
        if int(a[1]) != 0:
            raise HarnessError(f"retain_store failed: {a[1]}")
        return int(a[2])

    def delete_message(self, topic):
        if any(w in (b"+", b"#") for w in topic.split(b"/")):
            self._ids(f"delmatch {_hex(topic)}", "retain_delete_matching")
        else:
            self._k(f"delete {_hex(topic)}", "retain_delete")

    def clean(self):
        self._k("clean", "retain_clean")

    def commit(self):
        self._k("commit", "retain_commit")

    def size(self):
        self.commit()
        return int(self._ask("size")[0].split()[1])

    def stats(self):
        a = list(map(int, self._ask("stats")[0].split()[1:]))
        return {"full_builds": a[0], "delta_commits": a[1], "base_topics": a[2], "delta_topics": a[3]}

    def read_message(self, topic, now_ms):
        self.commit()
        return [topic] if int(self._ask(f"read {_hex(topic)} {now_ms}")[0].split()[1]) == 1 else []

    def _rows(self, out, n):
        if out[0].startswith("E "):
            raise HarnessError(f"retain_match failed: {out[0].split()[1]}")
        rows = []
        for ln in out[:n]:
            assert ln[0] == "R", ln
            rows.append([_unhex(h) for h in ln.split()[1:]])
        return rows

    def match_messages_batch(self, filters, now_ms):
        self.commit()
        n = len(filters)
        out = self._ask(f"match {now_ms} {n}\n" + "\n".join(_hex(f) for f in filters), n + 1)
        rows = self._rows(out, n)
        assert int(out[n].split()[1]) == sum(len(r) for r in rows)
        return rows

    def match_messages(self, topic, now_ms):
        return self.match_messages_batch([topic], now_ms)[0]

    def match_pages_batch(self, filters, limits, cursors, now_ms):
        self.commit()
        n = len(filters)
        base = self.slots  # fresh cursor slots for this call: the cursors travel by value
        self.slots += n
        for k, c in enumerate(cursors):
            if c is not None:
                self._k("setcur %d %d %d %d" % ((base + k,) + tuple(c)), "setcur")
        out = self._ask(f"limit {now_ms} {n}\n" + "\n".join(
            f"{_hex(f)} {l} {base + k}" for k, (f, l) in enumerate(zip(filters, limits))), 2 * n + 1)
        rows = self._rows(out, n)
        cur = [tuple(map(int, ln.split()[1:])) for ln in out[n:2 * n]]
        # only the windows come back
        assert int(out[2 * n].split()[1]) == sum(len(r) for r in rows)
        return rows, cur

    def match_messages_cursor(self, topic, cursor, batch_read_number, now_ms):
        rows, cur = self.match_pages_batch([topic], [batch_read_number], [cursor], now_ms)
        assert cur[0][1] != RC.RC_STALE
        return rows[0], (None if cur[0][1] == RC.RC_DONE else cur[0])

    def _ids(self, cmd, what):
        a = self._ask(cmd)[0].split()
        if int(a[1]) != 0:
            raise HarnessError(f"{what} failed: {a[1]}")
        return [_unhex(h) for h in a[2:]]

    def clear_expired(self, now_ms):
        return self._ids(f"clear {now_ms}", "retain_clear_expired")

    def page_read(self, topic, page, limit, now_ms):
        return self._ids(f"page {'*' if topic is None else _hex(topic)} {page} {limit} {now_ms}",
                         "retain_page_read")


def einval():
    return pytest.raises(HarnessError, match="-22")


@contextlib.contextmanager
def harness(exe, specs=RC.DEFAULT):
    h = Harness(exe, specs)
    try:
        yield h
    except BaseException:
        h.p.kill()
        h.p.wait()
        raise
    else:
        h.close()


@pytest.fixture(scope="module", params=[RC.DEFAULT, []], ids=["index", "scan"])
def built(request, exe):
    """One built store per index setting, shared by the read-only page tests."""
    with harness(exe, request.param) as dev:
        ref = RR.Retainer(request.param)
        RC.build(dev, ref, request.param)
        yield dev, ref


@pytest.mark.parametrize("limit", RC.LIMITS)
def test_page_identity(built, limit):
    dev, ref = built
    RC.check_page_identity(dev, ref, RC.FILTERS, [limit] * len(RC.FILTERS))


@pytest.mark.parametrize("n", RC.BATCHES)
def test_page_identity_mixed_batches(built, n):
    dev, ref = built
    fs, ls = RC.mixed_batch(n)
    RC.check_page_identity(dev, ref, fs, ls)


def test_forged_cursors(built):
    RC.check_forged(built[0], einval)


def test_unlimited_match_edges(exe):
    """The existing kernels under the gate: the edge topics of tests/test_gpu_retainer.py."""
    from oracle import emqx_ref as R
    topics = [b"a", b"a/b", b"a/b/c", b"a//c", b"/", b"", b"$SYS/x", b"$SYS", b"b/a",
              b"long-level-word/x", b"long-level-wordy/x", b"a/b/c/d/e/f/g/h/i/j/k/l/m/n/o/p/q"]
    filters = [b"#", b"+", b"a/#", b"a/+", b"a/+/c", b"+/+", b"", b"/", b"/#", b"a/#/c",
               b"long-level-word/+", b"+/+/+/+/+/+/+/+/+/+/+/+/+/+/+/+/+", b"$SYS/#"]
    for specs in ([], RC.DEFAULT):
        with harness(exe, specs) as dev:
            assert dev.match_messages(b"#", 1) == []  # the empty store
            ref = R.Retainer(specs)
            for t in topics:
                dev.store_retained(t)
                ref.store_retained(t)
            for f, g in zip(filters, dev.match_messages_batch(filters, 1)):
                assert sorted(g, key=RR.wkey) == sorted(ref.match_messages(f, 1), key=RR.wkey), f
                if not specs:
                    assert g == sorted(g, key=RR.wkey), f
            assert dev.match_messages_batch([], 1) == []


@pytest.mark.parametrize("seed,dmax,specs", [(1, -1, RC.DEFAULT), (6, 10**9, []), (3, 0, RC.DEFAULT)])
def test_unlimited_match_random(exe, seed, dmax, specs):
    """Stores, deletes, patches and delta rebuilds against the oracle, as
    tests/test_gpu_retainer.py's random test does on the device (smaller)."""
    from oracle import emqx_ref as R
    rng = random.Random(seed)
    vocab = [b"a", b"b", b"", b"$s", b"cc", b"long-word-%d" % seed, b"long-word-x"]
    with harness(exe, specs) as dev:
        ref = R.Retainer(specs)
        dev.tune("delta_max", dmax)
        for step in range(4):
            for _ in range(rng.randint(40, 120)):
                t = b"/".join(rng.choice(vocab) for _ in range(rng.randint(1, 6)))
                if rng.random() < 0.75:
                    e = rng.choice([0, 0, 0, 50, 150])
                    ref.store_retained(t, e)
                    dev.store_retained(t, e)
                else:
                    ref.delete_message(t)
                    dev.delete_message(t)
            if dmax == 10**9 and step == 1:
                dev.tune("delta_max", 0)
                dev.commit()
                dev.tune("delta_max", dmax)
            if step == 2:
                ref.delete_message(b"a/+/#")
                dev.delete_message(b"a/+/#")
            filters = []
            for _ in range(100):
                ws = [rng.choice([b"+", b"a", b"b", b"", b"$s", b"cc", b"long-word-x"])
                      for _ in range(rng.randint(1, 6))]
                if rng.random() < 0.3:
                    ws[-1] = b"#"
                filters.append(b"/".join(ws))
            for f, g in zip(filters, dev.match_messages_batch(filters, 100)):
                assert sorted(g, key=RR.wkey) == sorted(ref.match_messages(f, 100), key=RR.wkey), (step, f)
                assert len(set(g)) == len(g)
            assert dev.size() == ref.size()


def test_cursors_under_change(exe):
    with harness(exe) as dev:
        ref = RR.Retainer(RC.DEFAULT)
        RC.build(dev, ref, RC.DEFAULT)
        RC.check_cursors_under_change(dev, ref)


def test_clear_expired(exe):
    with harness(exe) as dev:
        RC.check_clear_expired(dev, RR.Retainer(RC.DEFAULT))


@pytest.mark.parametrize("limit", [1, 3])
def test_table_full(exe, limit):
    with harness(exe) as dev:
        RC.check_table_full(dev, RR.Retainer(RC.DEFAULT), limit)


@pytest.mark.parametrize("specs", [RC.DEFAULT, []], ids=["index", "scan"])
def test_page_read(exe, specs):
    with harness(exe, specs) as dev:
        RC.check_page_read(dev, RR.Retainer(specs))
        RC.check_page_read_invalid(dev, einval)


@pytest.mark.parametrize("specs", [RC.DEFAULT, []], ids=["index", "scan"])
def test_delete_matching(exe, specs):
    with harness(exe, specs) as dev:
        RC.check_delete_matching(dev, RR.Retainer(specs), specs)


@pytest.mark.parametrize("name", sorted(RC.golden()))
def test_suite_vectors(exe, name):
    with harness(exe) as dev:
        RC.run_golden(dev, RC.golden()[name])
