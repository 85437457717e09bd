"""Closed edge buckets (gm_common.h EDGE_CLOSED), under ASan + UBSan, on the CPU.

tests/host_harness/closed_harness.cpp includes emqx_amd/csrc/gm_engine.cpp and runs it against the
fake HIP runtime, like rph_harness.cpp: a stand-alone program, run directly.  A cfg3 miniature and
a random cfg2-like trie -- plain and with 3-bit collision tokens, keyed on / auto, fat buckets on /
off -- are built and churned by delta commits: inserts whose home bucket is full and closed (the
word is chosen by its edge_home, so the edge lands past the bucket and the commit must open it),
deletes, re-inserts into TOMB slots, a fat half moving out, a node gaining and losing its '+'
child while its bucket is closed, a background full build with catch-up, a snapshot save and load
with further deltas.  After every commit no live edge lies past a marked bucket on its own chain,
marks sit only on live slots without a '+' child, model and table agree slot by slot, and the rows
of the plain reader (harness_walk.h CpuWalk), of the restatement of k_walk's iteration (SlotWalk)
with the rule on and off, and of the oracle are equal."""
import subprocess

import pytest

import closed_cases
import host_build


@pytest.mark.timeout(600)
def test_closed_buckets_under_asan_ubsan():
    exe = host_build.build("closed_harness.cpp")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=540)
    assert r.returncode == 0, r.stdout[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK", r.stdout[-2000:]
    commits, deltas, opened, past, stops, rows = map(int, last[1:])
    print(r.stdout[-400:])
    # both commit paths ran, deltas opened buckets, edges landed past full closed buckets, the
    # rule ended lookups, rows were compared
    assert commits > deltas > 0 and opened > 0 and past > 0 and stops > 0 and rows > 0


@pytest.mark.timeout(600)
def test_census_of_the_miniature_restated(tmp_path):
    """The restated walk's bucket loads and lane iterations on the miniature cfg3 that
    tests/test_gpu_closed.py runs on the device: with the rule off the figures recorded for the
    parent's census on the device, with it on the figures the device census must equal."""
    exe = host_build.build("closed_harness.cpp")
    filters, topics = closed_cases.miniature()
    ff, tf = tmp_path / "filters.txt", tmp_path / "topics.txt"
    ff.write_text("".join(f + "\n" for f in filters))
    tf.write_text("".join(t + "\n" for t in topics))
    r = subprocess.run([exe, "--count", str(ff), str(tf)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, env=host_build.ENV, timeout=540)
    assert r.returncode == 0, r.stdout[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "COUNT", r.stdout[-2000:]
    l0, i0, l1, i1, stops = map(int, last[1:])
    print(last)
    assert (l0, i0) == closed_cases.CENSUS[0] and (l1, i1) == closed_cases.CENSUS[1]
    assert l1 < l0 and i1 < i0 and stops > 0
