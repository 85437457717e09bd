"""The NIF (c_src/emqx_trie_gpu_nif.c) compiles without a warning: gcc -fsyntax-only -Wall -Wextra
-Werror against tests/nif_stub/erl_nif.h (the erl_nif declarations it uses, OTP's signatures)
and include/emqx_gpumatch.h.  The same header is the fake runtime's (tests/nif_stub/
fake_erl_nif.c), on which tests/test_nif_host.py and tests/test_gpu_nif.py link and run the NIF."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_nif_compiles_against_erl_nif_declarations():
    r = subprocess.run(["gcc", "-fsyntax-only", "-std=c11", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "tests", "nif_stub"),
                        "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "c_src", "emqx_trie_gpu_nif.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
