"""The bytes the kernels read, commit by commit, against a recorded run (CPU, ASan + UBSan).

tests/host_harness/image_main.cpp includes emqx_amd/csrc/gm_engine.cpp and runs it against the
fake HIP runtime, like harness.cpp: a stand-alone program, run directly.  It drives one engine
through a fixed, seeded script -- a full build, delta commits of mixed trie and route-key adds and
deletes, a snapshot half-way, a full build of the churned registry; word_hash_bits 0 and 3, keyed 1
and 2 -- and prints after every commit a digest of the committed tables and of the scalar fields
of the index.  tests/golden/table_images.json holds the lines of the commit before the host
model's placement and path code moved into gm_model.h: host code that leaves the table layout
alone prints the same lines."""
import json
import os
import subprocess

import pytest

import host_build

GOLDEN = os.path.join(host_build.ROOT, "tests", "golden", "table_images.json")


@pytest.mark.timeout(600)
def test_table_images_equal_the_recorded_run(tmp_path):
    exe = host_build.build("image_main.cpp")
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=host_build.ENV, timeout=540)
    assert r.returncode == 0, r.stdout[-6000:]
    got = r.stdout.strip().splitlines()
    with open(GOLDEN) as f:
        want = json.load(f)["lines"]
    # the script did what the record is about: per run one full build first, at least 20 deltas,
    # a snapshot, a full build last
    for run in ("h0 k1", "h0 k2", "h3 k1", "h3 k2"):
        mine = [l.split() for l in want if l.startswith(run + " ")]
        commits = [l for l in mine if l[2] == "commit"]
        assert commits[0][4] == "full" and commits[-1][4] == "full"
        assert sum(l[4] == "delta" for l in commits) >= 20
        assert sum(l[2] == "snapshot" for l in mine) == 1
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, "first differing line %d: got %r, recorded %r" % diff[0]
    assert len(got) == len(want)
