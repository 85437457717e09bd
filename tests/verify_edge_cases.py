"""Inputs aimed at verify_one (emqx_amd/csrc/gm_verify.inc): a staged pair is re-checked on bytes
in LDS when the topic has at most 64 bytes and the filter at most VINL = 60, from global memory
otherwise, and the LDS topic window starts at the topic's address rounded down to 16 bytes.

With one-bit tokens (Engine(word_hash_bits=1)) a near-miss word shares its token with the
filter's word half of the time; only those are kept, so every near miss here is staged and has
to be rejected on bytes.  Two filter families reach the topic lengths independently of the
filter length:

  P  "+/<W>"   topic "<p..>/<V>": the bytes that decide sit at the window's end
  H  "<W>/#"   topic "<V>/<r..>": they sit at its start, offset by the address residue

W has fl - 2 bytes for fl = 59, 60, 61; V is W (the true match) or differs from it in the first,
the last or a middle byte, or in length by one; p or r pad the topic to 63, 64 or 65 bytes.
Every (family, fl, tl) group is placed at every residue 0..15 of the packed batch by a filler
topic of 1..16 bytes in front of it.  One batch per (family, tl) keeps the rejects of a batch
within what the scatter adjusts in line, so the rows come from k_verify, not from the legacy
pass.
"""
import functools

from oracle import emqx_ref as R
from postwalk_cases import word_token_bits

FLS = (59, 60, 61)  # VINL = 60: inline verification record / string pool
TLS = (63, 64, 65)  # 64: LDS window / global memory
BITS = 1
CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"
KINDS = ("first", "last", "middle", "length")
PER_KIND = 4        # 16 near misses per group


def word(fam: str, fl: int) -> bytes:
    lw = fl - 2
    return (("%s%d-" % (fam, fl)) + "".join(CHARS[(7 * i + fl) % 36] for i in range(lw)))[:lw].encode()


def filt(fam: str, fl: int) -> bytes:
    f = b"+/" + word(fam, fl) if fam == "P" else word(fam, fl) + b"/#"
    assert len(f) == fl
    return f


def filters():
    return [filt(fam, fl) for fam in "PH" for fl in FLS]


@functools.lru_cache(maxsize=None)
def near_words(fam: str, fl: int):
    """[(kind, V)]: PER_KIND words per kind that differ from W as the kind says and share its
    one-bit token."""
    w = word(fam, fl)
    tok = word_token_bits(w, BITS)
    mid = len(w) // 2
    cand = {
        "first": [c.encode() + w[1:] for c in CHARS],
        "last": [w[:-1] + c.encode() for c in CHARS],
        "middle": [w[:mid] + c.encode() + w[mid + 1:] for c in CHARS],
        "length": [w[:-1], w[1:]] + [w + c.encode() for c in CHARS],
    }
    out = []
    for kind in KINDS:
        hit = [v for v in cand[kind] if v != w and word_token_bits(v, BITS) == tok][:PER_KIND]
        assert len(hit) == PER_KIND, (fam, fl, kind)
        out += [(kind, v) for v in hit]
    return tuple(out)


def _topic(fam: str, v: bytes, tl: int) -> bytes:
    pad = tl - 1 - len(v)
    assert pad >= 1
    t = b"p" * pad + b"/" + v if fam == "P" else v + b"/" + b"r" * pad
    assert len(t) == tl
    return t


@functools.lru_cache(maxsize=None)
def batch(fam: str, tl: int):
    """(topics, info): info[i] = None for a filler, else (fl, residue, kind) with kind "true"
    for the match.  Asserts the coverage from the inputs themselves."""
    topics, info, off = [], [], 0
    for fl in FLS:
        w, f = word(fam, fl), filt(fam, fl)
        for r in range(16):
            fill = (r - off - 1) % 16 + 1  # 1..16 bytes bring the next topic to residue r
            topics.append(b"f" * fill)
            info.append(None)
            off += fill
            for kind, v in (("true", w),) + near_words(fam, fl):
                t = _topic(fam, v, tl)
                assert R.match(t, f) is (kind == "true"), (t, f)
                topics.append(t)
                info.append((fl, off % 16, kind))
                off += tl
    # coverage: the match at every (fl, residue); per fl, near misses of every kind, at least
    # 16 per group, and at every residue too; the last topic of the batch is an edge topic
    true_at = {(i[0], i[1]) for i in info if i and i[2] == "true"}
    assert true_at == {(fl, r) for fl in FLS for r in range(16)}
    for fl in FLS:
        near = [i for i in info if i and i[0] == fl and i[2] != "true"]
        assert len(near) == 16 * 16 and {i[2] for i in near} == set(KINDS)
        assert {i[1] for i in near} == set(range(16))
    assert {len(t) for t, i in zip(topics, info) if i} == {tl}
    assert all(1 <= len(t) <= 16 for t, i in zip(topics, info) if not i)
    assert info[-1] is not None
    return tuple(topics), tuple(info)


def batches():
    return [(fam, tl) for fam in "PH" for tl in TLS]
