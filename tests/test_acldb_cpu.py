"""emqx_amd/csrc/gm_acldb_match.h alone on the CPU (DESIGN.md 6b "Built-in database"): the probe,
the run walk and the relative indices in the stand-alone tests/host_harness/acldb_main.cpp under
ASan + UBSan, on the chain keys of tests/acldb_cases.py.  What the table holds is read from the
table: the chain that wraps past its end, the deleted key lying between a key's home and its slot,
the key stored again into that slot.  The program also feeds the walk and the kernel's lookup
phase the malformed runs and slots that the C-ABI cannot build (a run past the pool's end, fields
that are not the rule's position, a filter or key index at or past its array's end): each is
refused before it is followed, with every array an allocation of its exact size."""
import os
import subprocess

import pytest

import acldb_cases as DC
import host_build

CSRC = host_build.CSRC
H = host_build.H
DEPS = [os.path.join(CSRC, f) for f in ("gm_acldb.inc", "gm_acldb_match.h", "gm_acl_match.h", "gm_ruleset_match.h",
                                        "gm_match.h")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "ruleset_shim.h", "acl_input.h")]
N = DC.MIN_SLOTS


@pytest.fixture(scope="module")
def exe():
    return host_build.build("acldb_main.cpp", deps=DEPS)


def run(exe, hash_bits):
    ks = DC.chain_keys(hash_bits)
    r = subprocess.run([exe, str(hash_bits)] + [k.hex() for k in ks], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=host_build.ENV, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    return ks, r.stdout.split("\n")


def ints(line, tag):
    assert line.startswith(tag + " "), line
    return [int(x) for x in line.split()[1:]]


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_probe_chain_wrap_delete_and_store_again(exe, hash_bits):
    ks, out = run(exe, hash_bits)
    home = ints(out[0], "HOME")
    h = DC.home(ks[0], hash_bits, N)
    assert home == [h] * 4                                  # the header's adb_home is the cases' home
    slots = ints(out[1], "SLOTS")
    assert slots == [(h + k) % N for k in range(4)] and slots[-1] < slots[0]   # read from the table: it wraps
    states = out[2].split()[1:]
    assert [states[s] for s in slots] == ["0", "1", "2", "3"] and states.count("E") == N - 4
    assert ints(out[3], "FOUND") == slots and ints(out[4], "STEPS") == [1, 2, 3, 4]   # a chain of four
    assert ints(out[5], "DELETED") == [slots[1]]
    states = out[6].split()[1:]
    # the deleted key lies between the home of keys 2 and 3 and their slots
    assert states[slots[1]] == "D" and states[slots[2]] == "2" and states[slots[3]] == "3"
    assert (slots[1] - h) % N < (slots[2] - h) % N
    assert ints(out[7], "FOUND") == slots[2:] and ints(out[8], "STEPS") == [3, 4]      # found past it
    assert ints(out[9], "AGAIN") == [slots[1]]                                         # into the deleted slot
    assert out[10].split()[1:].count("D") == 0
    assert ints(out[11], "FOUND") == slots and ints(out[12], "STEPS") == [1, 2, 3, 4]


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_run_walk_and_malformed_runs_and_slots(exe, hash_bits):
    _, out = run(exe, hash_bits)
    assert "WALK ok" in out
    bad = [line[4:] for line in out if line.startswith("BAD ")]
    assert len(bad) == 17
    for must in ("a run that starts at the pool's end", "a run longer than the pool",
                 "a rule field that is not the position", "a filter field that is not the position",
                 "a filter base at the offset array's end", "the second filter at the offset array's end"):
        assert must in bad
    slot = [line[5:] for line in out if line.startswith("SLOT ")]
    assert slot == ["a well-formed slot", "a key index at the key array's end", "a key index far past the key array",
                    "a run at the pool's end", "a run far past the pool"]
