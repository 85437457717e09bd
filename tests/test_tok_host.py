"""The per-lane functions of emqx_amd/csrc/gm_tok.inc on the CPU, under ASan + UBSan, over the
case batches of tests/tok_cases.py (tests/host_harness/tok_main.cpp includes the file unchanged
behind hip_shim.h; nothing is preloaded, the program is run directly).

Tokeniser: every topic of every batch through tok_words_rec over a staged LDS tile (a heap block
of exactly the kernel's size) and through tok_words over global memory, at the batch address
residues 0, 1, 5 and 15; levels, flags, the seven record tokens and the deep tokens must equal the
Python word_token reference and each other, the fit decision of every tile must be tok_cases', and
the copy-through staging must store the bytes it read.  Once more with 3-bit test tokens.

Probe: the route-key table built by the engine's own host code (fake HIP runtime) with 64- and
2-bit key hashes, for plain-only, wild-only and both regions; every K-family name through
exact_lookup over global memory and over the LDS tile, exact_lookup_wild, k_xhash + exact_probe
and k_exact_owned must give the id a std::map of the keys gives.  Each batch ends in the last
dword of its heap block, so a read past a batch's last name trips ASan."""
import os
import re
import subprocess
import time

import pytest

import host_build
import tok_cases as T
from postwalk_cases import word_token, word_token_bits

ROOT = host_build.ROOT
KERNELS = os.path.join(host_build.CSRC, "gm_kernels.hip")
CONSTS = os.path.join(host_build.H, "build", "tok_consts.inc")
BASES = (0, 1, 5, 15)
T_WILD, T_DOLLAR = 1, 2  # gm_common.h


def _hex(x: bytes) -> str:
    return x.hex() or "-"


@pytest.fixture(scope="module")
def exe():
    """The constants gm_tok.inc takes from gm_kernels.hip, cut out of that file line by line, and
    the program."""
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
    t0 = time.time()
    out = host_build.build("tok_main.cpp", deps=[
        CONSTS, os.path.join(host_build.H, "hip_shim.h"), os.path.join(host_build.CSRC, "gm_tok.inc")])
    print("tok_main build: %.1f s" % (time.time() - t0))
    return out


def _run(exe, path, lines):
    path.write_text("\n".join(lines) + "\n")
    t0 = time.time()
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, errors="replace", env=host_build.ENV, timeout=540)
    print("tok_main run: %.1f s" % (time.time() - t0))
    assert r.returncode == 0, r.stdout[-6000:]
    out = r.stdout.split("\n")
    assert out[-2:] == ["OK", ""], r.stdout[-2000:]
    return out[:-2]


def _want(topic: bytes, bits: int):
    ws = topic.split(b"/")
    toks = [(1 << 63) | word_token_bits(w, bits) if bits else word_token(w) for w in ws]
    flags = (T_WILD if any(w in (b"+", b"#") for w in ws) else 0) | \
        (T_DOLLAR if topic[:1] == b"$" else 0)
    rec = (toks + [0] * T.REC_TOKS)[:T.REC_TOKS]
    return [len(ws), flags] + rec + toks[T.REC_TOKS:]


def test_constants_and_tokens_equal_the_reference(exe, tmp_path):
    runs = [(name, base, 0) for name in T.tok_batches() for base in BASES] + [("main", 0, 3)]
    flagged = (b"$SYS/a", b"$", b"a/+/b", b"#", b"+", b"a/#", b"$x/+", b"a+/b#", b"")
    lines = []
    for name, base, bits in runs:
        topics = T.tok_batches()[name][0] + (flagged if name == "main" else ())
        lines.append("tok %d %x %d" % (base, (1 << bits) - 1 if bits else 0, len(topics)))
        lines += [_hex(t) for t in topics]
    out = _run(exe, tmp_path / "tok_in.txt", lines)
    assert out[0] == "consts %d %d %d %d %d %d" % (T.TILE_BYTES, T.TILE_CHUNKS, T.REC_TOKS,
                                                  T.TOK_INLINE_MAX, T.XINL, T.WG)
    at, paths = 1, {"R": 0, "W": 0}
    for name, base, bits in runs:
        topics = T.tok_batches()[name][0] + (flagged if name == "main" else ())
        assert out[at].split() == ["tok", str(base), "%x" % ((1 << bits) - 1 if bits else 0),
                                   str(len(topics))]
        at += 1
        tiles = T.tiles_of(topics, base)
        if base == 0 and name != "main":  # the intended fit decisions, both kinds
            assert {f for _, _, f in tiles} == {True, False}
        for k, (sh, nbytes, fit) in enumerate(tiles):
            # the fit decision is tok_cases' rule (sh + bytes <= 16400), at every base
            assert fit == (sh + nbytes <= T.TILE_FIT)
            assert out[at] == "tile %d %d %d" % (k, sh, fit), (name, base, k, out[at])
            at += 1
            for t in range(k * T.WG, min((k + 1) * T.WG, len(topics))):
                want = _want(topics[t], bits)
                for path in ("RW" if fit else "W"):  # a non-fitting tile: tok_words alone
                    got = out[at].split()
                    at += 1
                    assert got[0] == path and int(got[1]) == t, (name, base, t, got[:2])
                    vals = [int(got[2]), int(got[3])] + [int(x, 16) for x in got[4:]]
                    assert vals == want, (name, base, bits, path, t, topics[t][:60].hex(),
                                          ["%x" % v for v in vals], ["%x" % v for v in want])
                    paths[path] += 1
    assert at == len(out)
    assert paths["R"] > 30000 and paths["W"] > paths["R"] + 4000  # both paths, and W alone


def test_probe_functions_equal_the_key_map(exe, tmp_path):
    lines, runs = [], []
    for tail in range(4):
        names, _ = T.probe_batch(tail)
        nbytes = sum(len(n) for n in names)
        b0 = -nbytes % 16  # the batch ends where its heap block ends, or 1..3 bytes before
        for base in ((b0, (b0 + 5) % 16) if tail == 0 else [(b0 - d) % 16 for d in range(4)]):
            for bits in (64, 2):
                for kinds in ("plain", "wild", "both"):
                    if tail and (bits, kinds) not in ((64, "both"), (2, "both"), (64, "wild")):
                        continue
                    keys = T.probe_keys(T.probe_batch(tail), kinds)
                    lines.append("probe %d %s %d %d %d" % (bits, kinds, base, len(keys), len(names)))
                    lines += [_hex(k) for k in keys] + [_hex(n) for n in names]
                    runs.append((tail, bits, kinds, base))
    out = _run(exe, tmp_path / "probe_in.txt", lines)
    assert len(out) == 1 + len(runs)
    for line, (tail, bits, kinds, base) in zip(out[1:], runs):
        got = line.split()
        assert got[:4] == ["probe", str(bits), kinds, str(base)]
        names = T.probe_batch(tail)[0]
        n, w = len(names), sum(nm.startswith(b"+/") for nm in names)
        # every function answered: with plain keys two lookups and the partitioned probe per name
        # (a wildcard name without wildcard keys is decided unprobed) and six owned-probe passes;
        # with wildcard keys the wildcard names' own probe
        assert int(got[4]) == {"both": 9 * n + w, "plain": 3 * (n - w) + 6 * n, "wild": w}[kinds], line
        assert w > 0.2 * n
