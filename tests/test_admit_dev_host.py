"""The CPU gate of the admission pass (DESIGN.md 6b "Admission"): k_admit's phase functions
(emqx_amd/csrc/gm_admit.inc, gm_admit_match.h, stage_tile of gm_tok.inc) run lane by lane, phase by
phase, and the host code behind the emqxgm_admit_* C-ABI (emqx_amd/csrc/gm_admit.cpp, every
"device" array an allocation of exactly the bytes in use) run under ASan + UBSan in
tests/host_harness/admit_dev_main.cpp, a stand-alone program, on exactly the inputs of
tests/test_gpu_admit.py (tests/admit_cases.py), for the LDS path and the global path, against the
reference semantics of tests/admit_ref.py, word for word.  No GPU; this passes before the kernel
runs on one."""
import os
import re
import subprocess

import pytest

import admit_cases as AC
import admit_ref as R
import host_build

CSRC = host_build.CSRC
H = host_build.H
KERNELS = os.path.join(CSRC, "gm_kernels.hip")
CONSTS = os.path.join(H, "build", "tok_consts.inc")
DEPS = [os.path.join(CSRC, f) for f in ("gm_admit.cpp", "gm_admit.inc", "gm_admit_match.h", "gm_tok.inc")] + [
    os.path.join(H, f) for f in ("hip_shim.h", "acl_input.h")]


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
    return CONSTS


@pytest.fixture(scope="module")
def exe():
    return host_build.build("admit_dev_main.cpp", deps=DEPS + [_consts()])


def input_text(batches, force_global):
    out = []
    for b in batches:
        n = len(b["items"])
        out.append("B %d %d %d %d %d %d %d %d" % (b["mode"], int(force_global), b["base"], b["pass_items"],
                                                 len(b["caps"]), n, b["flags"] is not None, b["zones"] is not None))
        for c in b["caps"]:
            out.append("%d %d %d %d %d %d" % (c["max_topic_levels"], c["max_qos_allowed"], c["retain_available"],
                                              c["wildcard_subscription"], c["shared_subscription"],
                                              c["exclusive_subscription"]))
        for i, it in enumerate(b["items"]):
            out.append("%s %d %d" % (it.hex() or "-", b["flags"][i] if b["flags"] is not None else 0,
                                     b["zones"][i] if b["zones"] is not None else 0))
    out.append("E")
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("force_global", [False, True])
@pytest.mark.parametrize("table", sorted(AC.TABLES))
def test_table(exe, tmp_path, table, force_global):
    """Every batch of the table in one run of the program; the records and emqxgm_admit_reason."""
    batches = AC.TABLES[table]()
    path = tmp_path / "admit_in.txt"
    path.write_text(input_text(batches, force_global))
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = iter(r.stdout.split("\n"))
    paths = []

    def run(b, _fg):
        got = [tuple(int(x) for x in next(lines).split()) for _ in b["items"]]
        end = next(lines).split()
        assert end[0] == "END"
        paths.append((int(end[1]), int(end[2])))
        for g in got:
            assert g[4] == R.reason(b["mode"], g[:4])
        return [g[:4] for g in got]

    assert AC.check_table(run, table, force_global) > 0
    if table == "lengths":
        # a tile with an item longer than the LDS tile reads global memory, the others LDS
        for b, (tiled, glob) in zip(batches, paths):
            long = max(len(it) for it in b["items"]) > 16384
            assert (glob > 0) == (long or force_global) and (tiled > 0) == (not long and not force_global)


def test_refused_calls_and_offsets_never_followed(exe):
    r = subprocess.run([exe, "--refused"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=host_build.ENV, timeout=300)
    assert r.returncode == 0 and "refused ok" in r.stdout, r.stdout[-4000:]
