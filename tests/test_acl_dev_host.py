"""The CPU gate of the ACL device path (DESIGN.md 6b "ACL lists"): k_acl's phase functions
(emqx_amd/csrc/gm_acl.inc) run lane by lane, phase by phase, and the host code behind the
emqxgm_acl_* C-ABI (emqx_amd/csrc/gm_acl.cpp, every "device" array an allocation of exactly the
bytes in use) run under ASan + UBSan in tests/host_harness/acl_dev_main.cpp, on exactly the inputs
of tests/test_gpu_acl.py (tests/acl_cases.py), against the reference semantics of
tests/acl_ref.py.  The program also checks the refused sets (a slot of 64 among them) and refused
requests, after which the list in force still answers.  No GPU; this passes before the kernel
runs on one."""
import os

import pytest

import acl_cases as AC
import acl_host_checks as K
import host_build

CSRC = host_build.CSRC
H = host_build.H
DEPS = [os.path.join(CSRC, f) for f in ("gm_acl.cpp", "gm_acl.inc", "gm_acl_match.h", "gm_ruleset_match.h",
                                        "gm_match.h")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "ruleset_shim.h", "acl_input.h")]


@pytest.fixture(scope="module")
def exe():
    return host_build.build("acl_dev_main.cpp", deps=DEPS)


@pytest.fixture
def run(exe, tmp_path):
    return K.runner(exe, tmp_path)


@pytest.mark.parametrize("hash_bits", [0, 4])
@pytest.mark.parametrize("n_rules", AC.LIST_SIZES)
def test_random_cases(run, n_rules, hash_bits):
    K.check_random(run, n_rules, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_client_values(run, hash_bits):
    K.check_values(run, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_first_match_order(run, hash_bits):
    K.check_named(run, "order", hash_bits)


def test_who_slots(run):
    K.check_named(run, "slots", 0)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_tiling(run, hash_bits):
    K.check_tiling(run, hash_bits)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_depth(run, hash_bits):
    K.check_depth(run, hash_bits)


@pytest.mark.parametrize("n", AC.BATCH_SIZES)
def test_block_edges(run, n):
    K.check_block(run, n)


def test_passes(run):
    K.check_passes(run)


@pytest.mark.parametrize("rules", AC.EMPTY_LISTS)
def test_empty_lists(run, rules):
    K.check_empty(run, rules)


def test_clients(run):
    K.check_clients(run)
