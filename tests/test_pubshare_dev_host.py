"""The CPU gate of the pick inside the publish (DESIGN.md 6b "The pick inside the publish"):
k_pubshare's phase functions (emqx_amd/csrc/gm_pubshare.inc over gm_share.inc) run lane by lane,
phase by phase, and the host code that drives them (share_pub_pass of
emqx_amd/csrc/gm_pubshare.cpp, the counter steps of gm_share.cpp, every "device" array an
allocation of exactly the bytes in use) run under ASan + UBSan in
tests/host_harness/pubshare_dev_main.cpp, a stand-alone program, on exactly the inputs of
tests/test_gpu_pubshare.py (tests/pubshare_cases.py), against oracle.emqx_ref.publish and
tests/share_ref.py.  The program writes the fan-out's entry arrays and the string pool itself, as
the reference's fan-out has them, and also feeds the kernel's phases the structures the C-ABI cannot
build.  No GPU; this passes before the kernel runs on one."""
import os
import subprocess

import pytest

import host_build
import pubshare_cases as PC
import share_cases as SC

CSRC = host_build.CSRC
H = host_build.H
DEPS = [os.path.join(CSRC, f) for f in ("gm_share.cpp", "gm_pubshare.cpp", "gm_share.inc", "gm_pubshare.inc",
                                        "gm_share_match.h", "gm_share_handle.h", "gm_match.h")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "acl_input.h")]


@pytest.fixture(scope="module")
def exe():
    return host_build.build("pubshare_dev_main.cpp", deps=DEPS)


@pytest.fixture
def play(exe, tmp_path):
    def run(script, hash_bits=0, chunk=0):
        path = tmp_path / "pubshare_in.txt"
        path.write_text(PC.input_text(script, hash_bits, chunk))
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=host_build.ENV, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:]
        return PC.parse_output(r.stdout, script)
    return run


def same_in_order(play, script, **kw):
    """The program answers in the reference's entry order: equal without sorting."""
    got, ref = play(script, **kw), PC.run_ref(script)
    assert got == ref, [(i, j, g, r) for i, (a, b) in enumerate(zip(got, ref)) for j, (g, r) in enumerate(zip(a, b))
                        if g != r][:3]
    return got


def test_structures_the_abi_cannot_build(exe):
    r = subprocess.run([exe, "--structures"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=300)
    assert r.returncode == 0 and "structures ok" in r.stdout, r.stdout[-4000:]


@pytest.mark.parametrize("n", SC.BATCH_SIZES)
@pytest.mark.parametrize("layout", ["spread", "one", "gaps"])
def test_entry_counts(play, n, layout):
    same_in_order(play, PC.count_script(n, layout))


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_to_lengths_and_key_identity(play, hash_bits):
    same_in_order(play, PC.to_length_script(), hash_bits=hash_bits)


def test_strategies_sizes_and_edges(play):
    same_in_order(play, PC.strategy_script())


def test_state_lists(play):
    same_in_order(play, PC.state_script())


def test_round_robin_per_group_three_chunks_against_one(play):
    one = same_in_order(play, PC.rr_group_script())
    assert same_in_order(play, PC.rr_group_script(), chunk=171) == one


def test_mutations(play):
    same_in_order(play, PC.mutation_script())


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_random_case(play, hash_bits):
    same_in_order(play, PC.random_script(), hash_bits=hash_bits)


def test_random_case_in_chunks(play):
    same_in_order(play, PC.random_script(), chunk=97)
