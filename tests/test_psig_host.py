"""Lent signatures (gm_common.h): the edge table's invariant under ASan + UBSan, on the CPU.

tests/host_harness/psig_harness.cpp includes emqx_amd/csrc/gm_engine.cpp and runs it against the
fake HIP runtime, like harness.cpp.  A cfg3-shaped trie (4 sites x 8 devices, the five patterns of
workloads/gen.cpp gen_cfg3) is built and churned by delta commits -- a literal child under an
existing D/+, a literal-less D gaining and losing its first literal child, the '+' child coming
and going, a keyed parent losing all its literal children, a fat node's half and its move out,
a root without literal children whose '+' child has some -- with every eligible node keyed and
with the automatic choice, with and without fat buckets, and in the 3-bit collision-token mode.
After the full build and after every step every live slot of the committed tables is scanned: with
CF_LIT clear and a carried '+' child the lent bits contain the class of every live literal child
of that '+' node, with CF_LIT set the field is the node's own (or the keyed 0), and every slot
equals what the model gives for its node.  The rows of the CPU walk that ignores lent bits
(harness_walk.h CpuWalk) stay equal to the oracle's."""
import subprocess

import pytest

import host_build


@pytest.mark.timeout(600)
def test_lent_signature_invariant_under_asan_ubsan():
    exe = host_build.build("psig_harness.cpp")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=540)
    assert r.returncode == 0, r.stdout[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK", r.stdout[-2000:]
    commits, deltas, slots, lending, rows = map(int, last[1:])
    # both commit paths ran, slots that lend a signature were scanned, rows were compared
    assert deltas > 0 and commits > deltas and slots > 0 and lending > 0 and rows > 0
