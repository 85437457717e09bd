"""Topic records in the parts the index can read (gm_common.h rec_parts), under ASan + UBSan, on
the CPU.

tests/host_harness/recparts_main.cpp is a stand-alone program, run directly (nothing is
preloaded).  It includes emqx_amd/csrc/gm_tok.inc unchanged behind hip_shim.h and
emqx_amd/csrc/gm_engine.cpp against the fake HIP runtime, and checks
  * rec_parts(max_depth) for max_depth 0..10 (compared here too);
  * the store / load round trip of a 64-topic block, of ragged tails and of the block edges
    (1, 63, 64, 65, 101, 129 topics) for 3 and 4 parts, plain and non-temporal stores, through
    k_tok's store_rec and the walk's rec_load: stored tokens come back, the rest read 0, the header
    word is equal, wbase is there exactly with 4 parts, nothing else is written;
  * that the restated walk (harness_walk.h SlotWalk) with every token from level max_depth on
    zeroed gives the rows, bucket loads and iterations of the same walk with full tokens -- which
    are the plain reader's and the oracle's -- after every commit of a churn of full builds and
    delta commits that deepens a five- and a six-level index to 7 and 8 levels, deletes at an
    unchanged max_depth and rebuilds, with every walk rule on."""
import os
import re
import subprocess

import pytest

import host_build

KERNELS = os.path.join(host_build.CSRC, "gm_kernels.hip")
CONSTS = os.path.join(host_build.H, "build", "tok_consts.inc")
REC_TOKS, REC_U4, REC_PARTS_MIN = 7, 4, 3  # gm_common.h


def _consts():
    """The constants gm_tok.inc takes from gm_kernels.hip, as tests/test_tok_host.py cuts them out
    (the same file, rewritten only when its text differs)."""
    src = open(KERNELS).read()
    lines = []
    for name in ("WG", "TILE_BYTES", "TILE_CHUNKS"):
        m = re.findall(r"^constexpr uint32_t %s = [^;]*;" % name, src, re.M)
        assert len(m) == 1, name
        lines.append(m[0])
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(CONSTS), exist_ok=True)
    if not os.path.exists(CONSTS) or open(CONSTS).read() != text:
        with open(CONSTS, "w") as f:
            f.write(text)


def _want_parts(depth):
    return max(REC_PARTS_MIN, (min(depth, REC_TOKS) + 1) // 2)


@pytest.mark.timeout(900)
def test_partial_records_under_asan_ubsan():
    _consts()
    exe = host_build.build("recparts_main.cpp", deps=[
        CONSTS, os.path.join(host_build.H, "hip_shim.h"), os.path.join(host_build.CSRC, "gm_tok.inc")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    out = r.stdout.strip().splitlines()
    parts = [l for l in out if l.startswith("parts ")]
    assert len(parts) == 1
    got = [int(x) for x in parts[0].split()[1:]]
    assert got == [_want_parts(d) for d in range(11)]
    assert got == [3] * 7 + [4] * 4  # all four parts exactly from seven levels on
    last = out[-1].split()
    assert last[0] == "OK", r.stdout[-2000:]
    commits, deltas, rows, p3, p4, zeroed = map(int, last[1:])
    print(out[-1])
    # full builds and deltas ran, rows were compared on both sides of the 3 | 4 boundary, and
    # tokens the walk must not read were really taken away
    assert commits > deltas > 0 and rows > 0 and p3 > 0 and p4 > 0 and zeroed > 0
