"""The emqx_topic:match/2 conformance set shared by tests/test_match2_cpu.py (mqtt_match of
emqx_amd/csrc/gm_match.h on the CPU) and tests/test_gpu_match2.py (the same function in k_rules
on the device): every string of 1..3 words over an alphabet that holds plain words, the empty
word, both wildcards, a '$' word, words that merely start with a wildcard character and words
long enough for a hashed token.  The strings serve as names and as filters, so the set holds
wildcard names (match/2 compares their '+' and '#' literally) and filters with '#' in any
position."""
import functools
import itertools

import numpy as np

from oracle import emqx_ref as R

WORDS = ["a", "b", "", "+", "#", "$a", "+x", "#x", "long-word-1", "long-word-2"]


@functools.lru_cache(maxsize=None)
def strings():
    """All 10 + 100 + 1,000 strings; no word holds a '/', so they are distinct."""
    out = [("/".join(ws)).encode() for k in (1, 2, 3) for ws in itertools.product(WORDS, repeat=k)]
    assert len(out) == len(set(out)) == 1110
    return out


@functools.lru_cache(maxsize=None)
def oracle(words: bool) -> np.ndarray:
    """bool [filter, name]: oracle.emqx_ref.match(name, filter) on binaries, or on R.words lists
    (the '$' clauses are the binary form's alone)."""
    s = strings()
    if words:
        s = [R.words(x) for x in s]
    out = np.zeros((len(s), len(s)), bool)
    for j, f in enumerate(s):
        out[j] = [R.match(n, f) for n in s]
    out.setflags(write=False)
    return out


def hash_under_hash(name: bytes, filt: bytes, prefix: bool = True) -> bool:
    """The filter ends in '#', the name's word at that position is '#' and the name goes on
    after it: match([H | T1], [H | T2]) (emqx_topic.erl:78) decides before match(_, ['#'])
    (:82), and the answer is false.  prefix: the words before it match too, so nothing else
    decides the pair."""
    nw, fw = R.words(name), R.words(filt)
    k = len(fw) - 1
    if fw[k] != R.HASH or len(nw) <= k + 1 or nw[k] != R.HASH:
        return False
    return not prefix or R.match(nw[:k], fw[:k])


def first_match(mat: np.ndarray, order) -> np.ndarray:
    """Index into `order` of the first filter matching each name (0xFFFFFFFF: none), from an
    oracle() matrix."""
    m = mat[np.asarray(order)]
    hit = m.any(axis=0)
    return np.where(hit, m.argmax(axis=0), 0xFFFFFFFF).astype(np.uint32)
