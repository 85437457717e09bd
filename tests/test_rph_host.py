"""The root's '+' half and the shared line of keyed siblings, under ASan + UBSan, on the CPU.

tests/host_harness/rph_harness.cpp includes emqx_amd/csrc/gm_engine.cpp and runs it against the
fake HIP runtime, like psig_harness.cpp.  A cfg3-shaped trie (G = site, p = site/+, H =
site/+/device) and a small one are built and churned by delta commits: H gains a '#' filter, a
terminal filter, a '+' child, a literal child; p gains a second and a third literal child and
loses them; the root's half moves out; p goes and comes.  After the full build and after every
step the copy in the arguments (DevIndex::rp0/rp1) is absent or equals node_slot of p's only
live literal child and that child's slot in the committed table; a second literal child clears
it in the same commit.  The restatement of k_walk's iteration (harness_walk.h SlotWalk: two
slots, the fill, the resolves in slot order, the late match of keyed siblings) returns the same
rows with both rules on, either one, and neither -- the rows of the reader that knows neither
rule (harness_walk.h CpuWalk) and the oracle's -- with every eligible node keyed, with the
automatic choice, without fat buckets and in the 3-bit collision-token mode (full home buckets:
the sibling goes on to its own probe)."""
import subprocess

import pytest

import host_build


@pytest.mark.timeout(600)
def test_root_plus_half_and_keyed_share_under_asan_ubsan():
    exe = host_build.build("rph_harness.cpp")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=540)
    assert r.returncode == 0, r.stdout[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK", r.stdout[-2000:]
    commits, deltas, present, rp_hits, shared, rows = map(int, last[1:])
    # both commit paths ran, the copy was there and was used, siblings shared a line, rows compared
    assert deltas > 0 and commits > deltas and present > 0 and rp_hits > 0 and shared > 0 and rows > 0
