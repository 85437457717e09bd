"""The CPU gate of the shared-subscription device path (DESIGN.md 6b "Shared subscriptions"):
k_share's phase functions (emqx_amd/csrc/gm_share.inc) run lane by lane, phase by phase, and the
host code behind the emqxgm_share_* C-ABI (emqx_amd/csrc/gm_share.cpp, every "device" array an
allocation of exactly the bytes in use) run under ASan + UBSan in
tests/host_harness/share_dev_main.cpp, a stand-alone program, on exactly the inputs of
tests/test_gpu_share.py (tests/share_cases.py), against the reference semantics of
tests/share_ref.py.  The program also makes the refused calls, after which the table in force
still answers, and feeds the kernel's phases the tables the C-ABI cannot build.  No GPU; this
passes before the kernel runs on one."""
import os
import subprocess

import pytest

import host_build
import share_cases as SC

CSRC = host_build.CSRC
H = host_build.H
DEPS = [os.path.join(CSRC, f) for f in ("gm_share.cpp", "gm_share.inc", "gm_share_match.h", "gm_match.h")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "acl_input.h")]


@pytest.fixture(scope="module")
def exe():
    return host_build.build("share_dev_main.cpp", deps=DEPS)


@pytest.fixture
def play(exe, tmp_path):
    def run(script, hash_bits=0, pass_names=0):
        path = tmp_path / "share_in.txt"
        path.write_text(SC.input_text(script, hash_bits, pass_names))
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=host_build.ENV, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:]
        return SC.parse_output(r.stdout, script)
    return run


def test_structures_the_abi_cannot_build(exe):
    r = subprocess.run([exe, "--structures"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=300)
    assert r.returncode == 0 and "structures ok" in r.stdout, r.stdout[-4000:]


def test_strategies_sizes_and_edges(play):
    SC.check_strategies(play)


@pytest.mark.parametrize("stage", [False, True])
@pytest.mark.parametrize("hash_bits", [0, 4])
def test_topic_lengths_and_key_identity(play, hash_bits, stage):
    SC.check_topics(play, hash_bits, stage)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_mutations(play, hash_bits):
    SC.check_mutations(play, hash_bits)


@pytest.mark.parametrize("split", [False, True])
def test_round_robin_per_group_golden(play, split):
    SC.check_golden_rr(play, split)


def test_round_robin_per_group_counters(play):
    SC.check_counters(play)


@pytest.mark.parametrize("n", SC.BATCH_SIZES)
def test_block_edges(play, n):
    SC.check_block(play, n)


@pytest.mark.parametrize("stage", [False, True])
@pytest.mark.parametrize("hash_bits", [0, 4])
def test_random_case(play, hash_bits, stage):
    SC.check_random(play, hash_bits, stage=stage)


def test_fourteen_passes_against_one(play):
    assert SC.check_random(play, 0, 287) == SC.check_random(play, 0)


def test_growth_and_garbage_rebuild(play):
    SC.check_big(play)


def test_refused_calls(play):
    SC.check_refused(play)
