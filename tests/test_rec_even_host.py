"""Even-elided topic records (gm_common.h: two parts and a header bit for each of the words 0 and
2, for an index whose literal edges of level 0, and those of level 2, each carry at most one
token), under ASan + UBSan, on the CPU.

tests/host_harness/receven_main.cpp is a stand-alone program, run directly (nothing is
preloaded).  It includes emqx_amd/csrc/gm_tok.inc unchanged behind hip_shim.h and
emqx_amd/csrc/gm_engine.cpp against the fake HIP runtime, and checks
  * the round trip store_rec<EVEN> -> rec_load_even -> rec_tokens_even for 1, 63, 64, 65
    and 129 topics, plain and non-temporal stores: tokens 1, 3, 4, 5 and the header exact, tok0 /
    tok2 equal to c_k exactly for the topics whose word equals it and 0 otherwise, part 2 and the
    tail of the last block untouched;
  * the host model's level state (none / one / many) after every commit of a churn of full builds,
    deltas, deletions, rebuilds and a snapshot load over indexes of 1 to 8 levels: equal to one
    recomputed from the live filters, or higher where a deletion would have lowered it, never
    backwards within deltas -- and that the restated walk fed with reconstructed tokens returns the
    rows of the plain reader and of the oracle."""
import os
import re
import subprocess

import pytest

import host_build

KERNELS = os.path.join(host_build.CSRC, "gm_kernels.hip")
CONSTS = os.path.join(host_build.H, "build", "tok_consts.inc")
RECPARTS_COMMITS = 144  # tests/host_harness/recparts_main.cpp: 8 rigs x 2 indexes x 9 commits


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


@pytest.mark.timeout(900)
def test_even_elided_records_under_asan_ubsan():
    _consts()
    exe = host_build.build("receven_main.cpp", deps=[
        CONSTS, os.path.join(host_build.H, "hip_shim.h"), os.path.join(host_build.CSRC, "gm_tok.inc")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=840)
    assert r.returncode == 0, r.stdout[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK", r.stdout[-2000:]
    commits, deltas, rows, even, three, rebuilt, loads = map(int, last[1:])
    print(" ".join(last), "(bucket loads apart, summed:", loads, ")")
    # a churn at least as long as recparts_main.cpp's, full builds and deltas, topics walked on
    # reconstructed tokens and on three parts, and words that really were rebuilt as 0
    assert commits >= RECPARTS_COMMITS and commits > deltas > 0
    assert rows > 0 and even > 0 and three > 0 and rebuilt > 0
