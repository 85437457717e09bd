"""The build recipe of the stand-alone host harness programs (tests/host_harness/*.cpp that
include emqx_amd/csrc/gm_engine.cpp): one g++ line against the fake HIP runtime and the oracle's
C++ restatement, under a sanitizer.  The programs are executables, run directly with ENV."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "tests", "host_harness")
CSRC = os.path.join(ROOT, "emqx_amd", "csrc")

SAN = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                "-fno-omit-frame-pointer"],
       "tsan": ["-fsanitize=thread"]}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
           TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")

LINKED = [os.path.join(H, "fake_hip.cpp"), os.path.join(ROOT, "oracle", "ref_trie.cpp")]
DEPS = LINKED + [os.path.join(ROOT, "include", "emqx_gpumatch.h")] + [
    os.path.join(H, f) for f in ("fakehip/hip/hip_runtime.h", "harness_walk.h", "harness_rig.h")] + [
    os.path.join(CSRC, f) for f in ("gm_engine.cpp", "gm_model.h", "gm_common.h", "gm_kernels.h",
                                    "gm_internal.h", "gm_roctx.h")]


def build(main, san="asan", deps=()):
    """tests/host_harness/<main> -> tests/host_harness/build/<main without .cpp>_<san>, rebuilt
    when a source or header it is made of (deps: what this program includes beyond DEPS) is
    newer."""
    src = os.path.join(H, main)
    out = os.path.join(H, "build", main.replace(".cpp", "") + "_" + san)
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in DEPS + [src] + list(deps)):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + SAN[san] + [
        "-Wno-subobject-linkage", "-I", os.path.join(H, "fakehip"), src] + LINKED + ["-pthread", "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return out
