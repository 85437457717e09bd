"""The CPU gate of the built-in database's device path (DESIGN.md 6b "Built-in database"):
k_acldb's phase functions (emqx_amd/csrc/gm_acldb.inc) run lane by lane, phase by phase, and the
host code behind the emqxgm_acldb_* C-ABI (emqx_amd/csrc/gm_acldb.cpp, every "device" array an
allocation of exactly the bytes in use) run under ASan + UBSan in
tests/host_harness/acldb_dev_main.cpp, a stand-alone program, on exactly the inputs of
tests/test_gpu_acldb.py (tests/acldb_cases.py, the update script included), against the reference
semantics of tests/acl_ref.py.  The program also makes the refused calls, after which the database
in force still answers.  No GPU; this passes before the kernel runs on one."""
import os
import subprocess

import pytest

import acldb_cases as DC
import acldb_checks as K
import host_build

CSRC = host_build.CSRC
H = host_build.H
DEPS = [os.path.join(CSRC, f) for f in ("gm_acldb.cpp", "gm_acldb.inc", "gm_acldb_match.h", "gm_acl_match.h",
                                        "gm_ruleset_match.h", "gm_match.h")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "ruleset_shim.h", "acl_input.h")]


@pytest.fixture(scope="module")
def exe():
    return host_build.build("acldb_dev_main.cpp", deps=DEPS)


@pytest.fixture
def play(exe, tmp_path):
    def run(script):
        path = tmp_path / "acldb_in.txt"
        path.write_text(DC.input_text(script))
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=host_build.ENV, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:]
        return DC.parse_output(r.stdout, script)
    return run


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_key_lengths_and_filter_forms(play, hash_bits):
    K.check_keys(play, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_source_order_and_empty_records(play, hash_bits):
    K.check_order(play, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_random_case(play, hash_bits):
    K.check_random(play, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_depth(play, hash_bits):
    K.check_depth(play, hash_bits)


def test_run_sizes(play):
    K.check_runs(play, 0)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_all_tiles(play, hash_bits):
    K.check_tiling(play, hash_bits)


def test_empty_all_record(play):
    K.check_empty_all(play)


def test_all_record_edited_repeatedly(play):
    K.check_all_edits(play)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_table_shapes(play, hash_bits):
    K.check_shapes(play, hash_bits)


@pytest.mark.parametrize("n", DC.BATCH_SIZES)
def test_block_edges(play, n):
    K.check_block(play, n)


def test_passes(play):
    K.check_passes(play)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_update_script(play, hash_bits):
    K.check_update(play, hash_bits, exact_alloc=True)
