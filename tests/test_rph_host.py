"""The root's '+' half and the shared line of keyed siblings, under ASan + UBSan, on the CPU.

tests/host_harness/rph_harness.cpp includes emqx_amd/csrc/gm_engine.cpp and runs it against the
fake HIP runtime, like psig_harness.cpp.  A cfg3-shaped trie (G = site, p = site/+, H =
site/+/device) and a small one are built and churned by delta commits: H gains a '#' filter, a
terminal filter, a '+' child, a literal child; p gains a second and a third literal child and
loses them; the root's half moves out; p goes and comes.  After the full build and after every
step the copy in the arguments (DevIndex::rp0/rp1) is absent or equals node_slot of p's only
live literal child and that child's slot in the committed table; a second literal child clears
it in the same commit.  A restatement of k_walk's iteration (two slots, the fill, the resolves in
slot order, the late match of keyed siblings) returns the same rows with both rules on, either
one, and neither -- the rows of the reader that knows neither rule (harness_walk.h, unchanged) and
the oracle's -- with every eligible node keyed, with the automatic choice, without fat buckets and
in the 3-bit collision-token mode (full home buckets: the sibling goes on to its own probe)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "tests", "host_harness")
OUT = os.path.join(H, "build", "rph_harness_asan")
SRCS = [os.path.join(H, "rph_harness.cpp"), os.path.join(H, "fake_hip.cpp"),
        os.path.join(ROOT, "oracle", "ref_trie.cpp")]
DEPS = SRCS + [os.path.join(H, "fakehip", "hip", "hip_runtime.h"), os.path.join(H, "harness_walk.h")] + [
    os.path.join(ROOT, "emqx_amd", "csrc", f) for f in ("gm_engine.cpp", "gm_common.h", "gm_kernels.h")
] + [os.path.join(ROOT, "include", "emqx_gpumatch.h")]


def _build():
    if os.path.exists(OUT) and all(os.path.getmtime(d) <= os.path.getmtime(OUT) for d in DEPS):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-subobject-linkage",
           "-I", os.path.join(H, "fakehip")] + SRCS + ["-pthread", "-o", OUT]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return OUT


@pytest.mark.timeout(600)
def test_root_plus_half_and_keyed_share_under_asan_ubsan():
    exe = _build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                       timeout=540)
    assert r.returncode == 0, r.stdout[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK", r.stdout[-2000:]
    commits, deltas, present, rp_hits, shared, rows = map(int, last[1:])
    # both commit paths ran, the copy was there and was used, siblings shared a line, rows compared
    assert deltas > 0 and commits > deltas and present > 0 and rp_hits > 0 and shared > 0 and rows > 0
