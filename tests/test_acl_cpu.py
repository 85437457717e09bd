"""ACL rule lists (DESIGN.md 6b "ACL lists") on the CPU: the list compiler, the client derivation,
the token predicates and the byte checks of emqx_amd/csrc/gm_acl_match.h alone, run by
tests/host_harness/acl_main.cpp under ASan + UBSan on the inputs of tests/acl_cases.py, against
the reference semantics of tests/acl_ref.py.  No HIP, no kernel, no C-ABI."""
import os
import subprocess

import pytest

import acl_cases as AC
import acl_host_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "tests", "host_harness")
EXE = os.path.join(H, "build", "acl_main_asan")
SRC = os.path.join(H, "acl_main.cpp")
DEPS = [SRC, os.path.join(H, "acl_input.h")] + [
    os.path.join(ROOT, "emqx_amd", "csrc", f)
    for f in ("gm_acl_match.h", "gm_ruleset_match.h", "gm_match.h", "gm_common.h")]


@pytest.fixture(scope="module")
def exe():
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in DEPS):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", SRC, "-o", EXE]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return EXE


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


@pytest.mark.parametrize("rules", AC.EMPTY_LISTS)
def test_empty_lists(run, rules):
    K.check_empty(run, rules)


def test_clients(run):
    K.check_clients(run)
