"""Inputs for the post-walk kernels' variant matrix (tests/test_gpu_postwalk.py), with the
conditions they rest on asserted on the CPU oracle alone (tests/test_postwalk_cases_cpu.py).

The grouped scatter (k_scatter_grp, gm_verify.inc) sorts its stores only for a batch of more
than 4,096 topics with at least 16 pairs per topic, the packed staging is redone wide only when
a topic has more pairs than the rank field holds, and the in-line rank adjustment runs only for
1..4,096 rejected pairs: the index and batches here are the smallest that reach all of that.

Index: {a,+}^k/# for k = 0..5 plus {a,+}^6, 127 filters.  Topics: 1..8 levels, each word 'a'
with probability 0.7, else one of 24 decoys d00..d23; topics of 7 or 8 levels end in a unique
word.  With collision-test tokens (Engine(word_hash_bits=3)) a decoy whose 3-bit token equals
a's follows a's edges, and every pair staged that way has to be rejected on bytes.
"""
import functools
import itertools
import random

import numpy as np

from oracle.cref import RefIndex

SIZES = (4096, 4097, 6000)  # one fused scan tile; one topic more; a partial last scan tile
SEED = 11
DECOYS = ["d%02d" % i for i in range(24)]
GRP_MIN = 16           # gm_verify.inc: pairs per topic from which k_scatter_grp groups
REJ_SCAN_MAX = 4096    # gm_kernels.h: rejects the scatter adjusts in line
# topics of a "few rejects" batch that keep a decoy colliding with 'a' under 3-bit tokens; the
# rest have theirs replaced by decoys that do not collide.  Rejected pairs per batch, predicted on
# the oracle (predicted_rejects):
#   few rejects: 446 at n = 4096, 4097 and 6000 (the same 32 topics lead every batch); the
#                engine's rejected_pairs grew by 446 in all 18 in-line cells on the MI355X
#                (3 sizes x 2 walks x packed / redone wide / wide), legacy_batches by 0;
#   all decoys:  6,025 at n = 4096 and 4097, 8,839 at n = 6000: past a reject capacity of 16 (and
#                past REJ_SCAN_MAX), the legacy hand-over -- legacy_batches grew by 1 in all 18
#                cells (a legacy pass does not add to rejected_pairs)
FEW_COLLIDERS = 32

_M64 = (1 << 64) - 1


def word_token_bits(word: bytes, bits: int) -> int:
    """word_token (emqx_amd/csrc/gm_common.h) in its collision-test mode: the low `bits` bits of
    fmix64 over the word's FNV-1a state."""
    h = 0xcbf29ce484222325
    for b in word:
        h = ((h ^ b) * 0x100000001b3) & _M64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & _M64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & _M64
    h ^= h >> 33
    return h & ((1 << bits) - 1)


def word_token(word: bytes) -> int:
    """word_token (gm_common.h) in production mode: a word of at most TOK_INLINE_MAX = 7 bytes is
    its bytes little-endian in bits 0..55 and its length in bits 56..62; a longer one is bit 63
    and fmix64 of its FNV-1a state, shifted right by one."""
    if len(word) <= 7:
        return int.from_bytes(word, "little") | (len(word) << 56)
    return (1 << 63) | (word_token_bits(word, 64) >> 1)


def _fmix64(k: int) -> int:
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M64
    return k ^ (k >> 33)


def key_hash(key: bytes, bits: int = 64) -> int:
    """key_hash (gm_common.h): the key's bytes as little-endian dwords, the last zero-padded, in
    two 32-bit multiply-rotate lanes folded through fmix64; the low `bits` bits are kept."""
    m = 0xFFFFFFFF
    a, b = 0x9747b28c ^ len(key), (0x85ebca6b + len(key)) & m
    for i in range(0, len(key), 4):
        w = int.from_bytes(key[i:i + 4], "little")
        a ^= (w * 0xcc9e2d51) & m
        a = ((((a << 15) | (a >> 17)) & m) * 5 + 0xe6546b64) & m
        b = (b + w * 0x1b873593) & m
        b = (((((b << 13) | (b >> 19)) & m) * 0x85ebca6b) & m) ^ 0xc2b2ae35
    return _fmix64((a << 32) | b) & ((1 << bits) - 1)


def filters():
    out = []
    for k in range(6):
        out += ["/".join(list(c) + ["#"]).encode() for c in itertools.product("a+", repeat=k)]
    out += ["/".join(c).encode() for c in itertools.product("a+", repeat=6)]
    assert len(out) == len(set(out)) == 127
    return out


@functools.lru_cache(maxsize=None)
def topics(n: int, few_rejects: bool = False):
    """The batch of n topics; few_rejects: only the first FEW_COLLIDERS topics that hold a
    decoy colliding with 'a' under 3-bit tokens keep it."""
    rng = random.Random(SEED)
    ta = word_token_bits(b"a", 3)
    collide = {d for d in DECOYS if word_token_bits(d.encode(), 3) == ta}
    free = [d for d in DECOYS if d not in collide]
    out, kept = [], 0
    for i in range(n):
        levels = rng.randint(1, 8)
        ws = ["a" if rng.random() < 0.7 else rng.choice(DECOYS) for _ in range(levels)]
        sub = rng.choice(free)  # (drawn for every topic: both variants share the random stream)
        if levels >= 7:
            ws[-1] = "u%d" % i
        if few_rejects and any(w in collide for w in ws[:6]):
            kept += 1
            if kept > FEW_COLLIDERS:
                ws = [sub if w in collide else w for w in ws]
        out.append("/".join(ws).encode())
    return tuple(out)


def pack(items, off_dtype):
    off = np.zeros(len(items) + 1, off_dtype)
    np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), np.uint8).copy(), off


def ref_index(fs):
    ref = RefIndex(True)
    fb, fo = pack(list(fs), np.uint64)
    ref.add_many(fb, fo, np.ones(len(fs), np.uint8))
    return ref


@functools.lru_cache(maxsize=None)
def expected(n: int, few_rejects: bool = False):
    """(tbytes, toff, row_ptr, ids sorted per row) of the batch on the oracle."""
    tb, to = pack(list(topics(n, few_rejects)), np.uint32)
    row, ids, _ = ref_index(filters()).match(tb, to, threads=8)
    for a in (tb, to, row, ids):
        a.setflags(write=False)
    return tb, to, row, ids


def _by_token(s: bytes, bits: int) -> bytes:
    return b"/".join(w if w in (b"+", b"#") else b"t%d" % word_token_bits(w, bits)
                     for w in s.split(b"/"))


def staged_pairs(fs, ts, bits: int) -> int:
    """Pairs the walk stages under `bits`-bit tokens: the oracle's pairs with every literal word
    of the filters and topics replaced by its token.  Those that are no matches of the words
    themselves are what the byte verification has to reject."""
    mapped = [_by_token(f, bits) for f in fs]
    uniq = list(dict.fromkeys(mapped))  # filters that share every token share a trie node, and
    mult = np.array([mapped.count(u) for u in uniq])  # a topic reaching it is staged for each
    tb, to = pack([_by_token(t, bits) for t in ts], np.uint32)
    _, ids, _ = ref_index(uniq).match(tb, to, threads=8)
    return int(mult[ids].sum())


@functools.lru_cache(maxsize=None)
def predicted_rejects(n: int, few_rejects: bool, bits: int = 3) -> int:
    return staged_pairs(filters(), topics(n, few_rejects), bits) - int(expected(n, few_rejects)[2][-1])
