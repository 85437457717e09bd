"""Inputs aimed at the first two kernels of a pass (emqx_amd/csrc/gm_tok.inc): the tokeniser
k_tok and the exact route-key probe (k_exact, k_exact_part + k_xhash, k_exact_owned and
exact_lookup_wild), shared by the CPU harness (test_tok_host.py) and the device test
(test_gpu_tok_edges.py).  Deterministic: no random numbers, every family numbers its topics from
a base of its own.

Tokeniser families.  A case topic T has no '+' or '#' word and a 3-byte id word no other topic
has, so the filter "T/#" matches T alone, and only if every level token the device computed equals
the host builder's; one filter with a mutated word per case must match nothing.

  W  a word of 0..9, 15, 16, 17 bytes at each level 0..8 of a 9-level topic, the topic at each
     residue 0..15 of the packed batch (a filler topic of 1..16 bytes in front, as
     verify_edge_cases.batch does); and topics of exactly 6, 7, 8, 9 levels that end at the word,
     with and without a trailing empty level (REC_TOKS = 7: record tokens / token array)
  B  the bytes 0x00 0x01 0x2E 0x30 0x7F 0x80 0xAF 0xFF (0xAF = '/' | 0x80, 0x2E and 0x30 are the
     neighbours of '/') at each position 0..3 of a dword, directly before and directly after a
     '/', in words of 1, 4, 7, 8 and 9 bytes.  No entry point refuses a byte value (0x00 included:
     every entry takes a pointer and a length), so none is left out.
  N  near misses: a filter word that differs from the topic's only in the 8th byte of 8, in the
     9th of 9, in the last of 17, by one appended or dropped byte at 6/7/8 bytes, 'a' against
     'a\\x00' -- none may match
  T  256-topic tiles, index-aligned to 256, whose sh + bytes is 16384, 16399, 16400, 16401, 16416
     for sh = 0, 1, 15 (the fit rule of stage_tile: sh + bytes <= 16400), the tile's last topic
     ending in turn in an empty level, a 1-byte, an 8-byte, a 9-byte word.  Fitting and
     non-fitting case tiles alternate (while both kinds last); where the tile before does not end
     at a tile's sh, a spacer tile of 256 short topics (it fits) brings it there.  The batch ends
     in a ragged tile (100 topics), ending in each of the four ways across the batches "tiles",
     "ragged1", "ragged2", "ragged3" (those three: one non-fitting tile and the ragged one).
     sh is off[t0] & 15 for the host API: the engine copies a batch to the start of a device
     allocation of its own (emqxgm_match_batch: d_in_bytes), which is 16-byte aligned.

Probe family K (names to look up, route keys present): key lengths 0..45 at the batch residues 0,
1, 2, 3 (the dword residues) and 15, a present key and an absent name of each length; near-miss
pairs (one a key, the other only looked up) equal except the last byte, byte 19, 20 or 21
(XINL = 20: inline bytes / string pool), a key and its extension or prefix by one byte, a pair
equal in the first 20 bytes and in length that differs at byte 40; all of it again as wildcard
strings ("+/" + body) for the wildcard-key region; and the batch's very last name with
len % 4 = 0, 1, 2, 3 across the four probe batches.  Fillers alternate between keys and absent
names, so about half of the names are present.
"""
import functools

from oracle import emqx_ref as R
from postwalk_cases import key_hash, word_token  # noqa: F401  (the token / hash references)

TILE_BYTES = 16384      # gm_kernels.hip TILE_BYTES: the tokeniser's LDS tile
TILE_CHUNKS = TILE_BYTES // 16 + 2  # gm_kernels.hip TILE_CHUNKS: 16-B chunks of the LDS buffer
TILE_FIT = 16400        # gm_tok.inc stage_tile: nch + 1 <= TILE_CHUNKS <=> sh + bytes <= 16400
REC_TOKS = 7            # gm_common.h: level tokens in the 64-B topic record
TOK_INLINE_MAX = 7      # gm_common.h: longest word whose token is its bytes
XINL = 20               # gm_common.h: key bytes inline in an exact-table entry
WG = 256                # gm_kernels.hip WG: topics per tile (one per lane)

CHARS = b"0123456789abcdefghijklmnopqrstuvwxyz"
W_LENS = tuple(range(10)) + (15, 16, 17)
B_BYTES = (0x00, 0x01, 0x2E, 0x30, 0x7F, 0x80, 0xAF, 0xFF)
B_LENS = (1, 4, 7, 8, 9)
T_TOTALS = (16384, 16399, 16400, 16401, 16416)
T_SH = (0, 1, 15)
ENDINGS = ("empty", "w1", "w8", "w9")
RAGGED = 100
K_LENS = tuple(range(46))
K_RES = (0, 1, 2, 3, 15)


def fits(sh: int, nbytes: int) -> bool:
    """stage_tile's decision, as the kernel computes it."""
    return ((sh + nbytes + 15) >> 4) + 1 <= TILE_CHUNKS


def _idw(n: int) -> bytes:
    assert 0 <= n < 36 ** 3
    return bytes((CHARS[n // 1296], CHARS[n // 36 % 36], CHARS[n % 36]))


def _fill(off: int, r: int) -> int:
    return (r - off - 1) % 16 + 1  # 1..16 bytes bring the next topic to residue r


def _mut(w: bytes) -> bytes:
    """A word of the same length (one byte for the empty word) that differs in its last byte."""
    return w[:-1] + bytes((w[-1] ^ 1,)) if w else b"0"


def _levels(idw: bytes, lvl: int, w: bytes, n: int, salt: int):
    """n levels with `w` at level lvl, the id at the first other level, 1..2-byte words else."""
    lv = [bytes((CHARS[(salt + 5 * j) % 36],)) * (1 + (salt + j) % 2) for j in range(n)]
    lv[0 if lvl else 1] = idw
    lv[lvl] = w
    return lv


class _Batch:
    def __init__(self):
        self.topics, self.info, self.off = [], [], 0

    def add(self, t: bytes, info=None):
        self.topics.append(t)
        self.info.append(info)
        self.off += len(t)

    def at(self, r: int):
        self.add(b"f" * _fill(self.off, r))

    def done(self):
        return tuple(self.topics), tuple(self.info)


def _case(fam, key, topic, own, mutant, extra=None):
    """info of a case topic: its family, what it covers, the filter that has to match it and the
    filters that must not."""
    d = {"fam": fam, "key": key, "own": own, "not": (mutant,) + ((extra,) if extra else ())}
    assert R.match(topic, own), (topic, own)
    for f in d["not"]:
        assert not R.match(topic, f), (topic, f)
    return d


def _w_family(b: _Batch):
    n = 0
    for L in W_LENS:
        for lvl in range(9):
            for r in range(16):
                w = bytes(CHARS[(5 * i + 3 * L + 7 * lvl + r) % 36] for i in range(L))
                lv = _levels(_idw(n), lvl, w, 9, n)
                t = b"/".join(lv)
                lv[lvl] = _mut(w)
                b.at(r)
                assert b.off % 16 == r
                b.add(t, _case("W", (L, lvl, r), t, t + b"/#", b"/".join(lv) + b"/#"))
                n += 1
    for L in W_LENS:
        for nlev in (6, 7, 8, 9):
            for trail in (False, True):
                w = bytes(CHARS[(7 * i + L + nlev) % 36] for i in range(L))
                lv = _levels(_idw(n), nlev - 1, w, nlev, n)
                t = b"/".join(lv) + (b"/" if trail else b"")
                lv[nlev - 1] = _mut(w)
                m = b"/".join(lv) + (b"/" if trail else b"")
                b.at((L + nlev) % 16)
                b.add(t, _case("Wd", (L, nlev, trail), t, t + b"/#", m + b"/#"))
                n += 1


def _b_family(b: _Batch):
    n = 10000
    for vi, v in enumerate(B_BYTES):
        for wl in B_LENS:
            for side in ("before", "after"):
                for p in range(4):
                    body = bytes(CHARS[(3 * i + vi + wl) % 36] for i in range(wl - 1))
                    w = body + bytes((v,)) if side == "before" else bytes((v,)) + body
                    v2 = v ^ 0x80 if v >= 0x80 else v ^ 0x40  # (0xAF -> '/': another split)
                    w2 = body + bytes((v2,)) if side == "before" else bytes((v2,)) + body
                    idw = _idw(n - 10000 + 3000)
                    at = 4 + (wl - 1 if side == "before" else 0)  # the byte's offset in the topic
                    b.at((p - at) % 4 + 4 * ((vi + wl) % 4))
                    assert (b.off + at) % 4 == p
                    t = idw + b"/" + w + b"/k"
                    assert t[at] == v and t[at + 1 if side == "before" else at - 1] == 0x2F
                    b.add(t, _case("B", (v, p, wl, side), t, t + b"/#", idw + b"/" + w2 + b"/k/#"))
                    n += 1


def _n_kinds():
    k8, k17 = b"nearmis8", b"seventeen-bytes-w"
    out = [("b8", k8, k8[:7] + b"9"), ("b9", k8 + b"a", k8 + b"b"),
           ("b17", k17, k17[:16] + b"v")]
    for L in (6, 7, 8):
        w = b"lengthxy"[:L]
        out += [("app%d" % L, w, w + b"q"), ("drop%d" % L, w, w[:-1])]
    out += [("nul", b"a", b"a\x00"), ("nul-r", b"a\x00", b"a")]
    assert len(k17) == 17
    return out


def _n_family(b: _Batch):
    n = 0
    for kind, v, w in _n_kinds():
        for lvl in (0, 3, 6, 7, 8):
            for r in range(4):
                idw = _idw(5000 + n)
                lv = _levels(idw, lvl, v, 9, n)
                t = b"/".join(lv)
                lv[lvl] = w
                near = b"/".join(lv) + b"/#"
                lv[lvl] = _mut(v)
                b.at(r + 4 * (n % 4))
                b.add(t, _case("N", (kind, lvl, r), t, t + b"/#", b"/".join(lv) + b"/#", near))
                n += 1


@functools.lru_cache(maxsize=None)
def main_batch():
    """(topics, info) of the W, B and N families; info[i] is None for a filler."""
    b = _Batch()
    _w_family(b)
    _b_family(b)
    _n_family(b)
    topics, info = b.done()
    # coverage, from the inputs
    keys = lambda fam: {i["key"] for i in info if i and i["fam"] == fam}  # noqa: E731
    assert keys("W") == {(L, lvl, r) for L in W_LENS for lvl in range(9) for r in range(16)}
    assert keys("Wd") == {(L, n, t) for L in W_LENS for n in (6, 7, 8, 9) for t in (False, True)}
    assert keys("B") == {(v, p, wl, s) for v in B_BYTES for p in range(4) for wl in B_LENS
                         for s in ("before", "after")}
    assert keys("N") == {(k, lvl, r) for k, _, _ in _n_kinds() for lvl in (0, 3, 6, 7, 8)
                         for r in range(4)}
    off = 0
    for t, i in zip(topics, info):
        if i and i["fam"] == "W":
            L, lvl, r = i["key"]
            ws = t.split(b"/")
            assert off % 16 == r and len(ws) == 9 and len(ws[lvl]) == L
        if i and i["fam"] == "Wd":
            L, n, trail = i["key"]
            ws = t.split(b"/")
            assert len(ws) == n + trail and len(ws[n - 1]) == L and (not trail or ws[-1] == b"")
        if i and i["fam"] == "B":
            v, p, wl, side = i["key"]
            at = 4 + (wl - 1 if side == "before" else 0)
            assert t[at] == v and (off + at) % 4 == p and len(t.split(b"/")[1]) == wl
        if i is None:
            assert 1 <= len(t) <= 16
        off += len(t)
    cases = [t for t, i in zip(topics, info) if i]
    assert len(set(cases)) == len(cases)
    assert not any(R.wildcard(t) for t in topics)
    return topics, info


def _end(ending: str) -> bytes:
    return {"empty": b"/", "w1": b"/z", "w8": b"/endword8", "w9": b"/endword9x"}[ending]


def _shape(idw: bytes, length: int, ending: str) -> bytes:
    """A topic of `length` bytes: id / ab / a pad word / the ending."""
    suf = _end(ending)
    t = idw + b"/ab/" + b"p" * (length - 7 - len(suf)) + suf
    assert len(t) == length and length - 7 - len(suf) >= 1
    return t


def _tile_case(idw, length, ending, key):
    t = _shape(idw, length, ending)
    m = t[:-1] + bytes((t[-1] ^ 1,)) if ending != "empty" else t + b"0"
    return t, _case("T", key, t, t + b"/#", m + b"/#")


def _tile_specs():
    """(sh, total) of the case tiles: fitting and non-fitting in turn, as far as they go, and
    where it can be a tile whose sh is the residue the tile before it ends at (total & 15), so
    that no spacer tile is needed in front of it."""
    fit = [(sh, tot) for tot in T_TOTALS for sh in T_SH if tot <= TILE_FIT]
    non = [(sh, tot) for tot in T_TOTALS for sh in T_SH if tot > TILE_FIT]
    out, res, want_fit = [], 0, True
    while fit or non:
        pool = fit if (want_fit and fit) or not non else non
        pick = next((s for s in pool if s[0] == res), pool[0])
        pool.remove(pick)
        out.append(pick)
        res, want_fit = pick[1] & 15, pick[1] > TILE_FIT
    return out


@functools.lru_cache(maxsize=None)
def tile_batch(ragged: int, full: bool = True):
    """(topics, info, spec): the T family with its ragged last tile ending in ENDINGS[ragged];
    full=False: one case tile only (the batches that exist for their ragged tile).  spec[k] =
    (sh, total, ending) of tile k for a case tile, None for a spacer or the ragged tile."""
    b = _Batch()
    spec, n = [], 0
    tiles = _tile_specs() if full else [(0, 16401)]
    for k, (sh, total) in enumerate(tiles):
        if b.off % 16 != sh:  # a spacer tile: 256 short topics that end at residue sh
            for i in range(WG):
                b.add(b"s/" + b"p" * (6 + (_fill(b.off + 8 * WG, sh) % 16 if i == 0 else 0)))
            spec.append(None)
        assert len(b.topics) % WG == 0 and b.off % 16 == sh
        ending = ENDINGS[(k + k // 2 + ragged) % 4]  # (every ending on tiles of both kinds)
        nbytes = total - sh
        for i in range(WG - 1):
            t, info = _tile_case(_idw(n), 64, ENDINGS[i % 4], (k, i))
            b.add(t, info if i % 37 == 0 else None)
            n += 1
        t, info = _tile_case(_idw(n), nbytes - 64 * (WG - 1), ending, (k, WG - 1))
        b.add(t, info)
        n += 1
        spec.append((sh, total, ending))
    for i in range(RAGGED):
        last = i == RAGGED - 1
        t, info = _tile_case(_idw(n), 40 + i % 5, ENDINGS[ragged] if last else ENDINGS[i % 4],
                             ("ragged", i))
        b.add(t, info if last or i % 37 == 0 else None)
        n += 1
    spec.append(None)
    topics, info = b.done()
    # coverage, from the inputs: each case tile's sh + bytes and fit are the intended ones
    tl = tiles_of(topics)
    assert len(tl) == len(spec) and len(topics) % WG == RAGGED
    for (sh, nbytes, fit), s, k in zip(tl, spec, range(len(spec))):
        if s:
            assert (sh, sh + nbytes) == s[:2] and fit == (s[1] <= TILE_FIT)
            assert topics[k * WG + WG - 1].endswith(_end(s[2]))
        else:
            assert fit
    if full:
        assert {s[:2] for s in spec if s} == {(sh, t) for sh in T_SH for t in T_TOTALS}
        assert {s[2] for s in spec if s} == set(ENDINGS)
        fitting = [s[1] <= TILE_FIT for s in spec if s]
        assert all(a != c for a, c in zip(fitting[:12], fitting[1:12]))  # they alternate
    assert topics[-1].endswith(_end(ENDINGS[ragged])) and info[-1] is not None
    return topics, info, tuple(spec)


def tiles_of(topics, base: int = 0):
    """[(sh, bytes, fits)] of each 256-topic tile of a packed batch whose first byte lies at
    address residue `base` (0 for the host API: see the module docstring)."""
    out, off = [], base
    for t0 in range(0, len(topics), WG):
        nbytes = sum(len(t) for t in topics[t0:t0 + WG])
        out.append((off % 16, nbytes, fits(off % 16, nbytes)))
        off += nbytes
    return out


def tok_batches():
    """{name: (topics, info)} of every tokeniser batch."""
    out = {"main": main_batch(), "tiles": tile_batch(0)[:2]}
    for r in (1, 2, 3):
        out["ragged%d" % r] = tile_batch(r, False)[:2]
    return out


@functools.lru_cache(maxsize=None)
def tok_filters():
    """Every filter of the tokeniser families, in insertion order, without repeats."""
    fs = []
    for topics, info in tok_batches().values():
        for i in info:
            if i:
                fs.append(i["own"])
                fs.extend(i["not"])
    fs = tuple(dict.fromkeys(fs))
    assert sum(len(t) for t, _ in tok_batches().values()) <= 12500 and len(fs) <= 8000
    return fs


@functools.lru_cache(maxsize=None)
def expected_rows(name: str):
    """Per topic of batch `name`: the sorted filters of tok_filters() that oracle.emqx_ref's trie
    gives.  Computed once (the trie is shared by every batch) and never changed."""
    return tuple(tuple(sorted(_trie().match(t))) for t in tok_batches()[name][0])


@functools.lru_cache(maxsize=None)
def _trie():
    trie = R.Trie()
    for f in tok_filters():
        trie.insert(f)
    return trie


# ---- the probe family -------------------------------------------------------------------------

def _kbody(L: int, salt: int, absent: bool = False) -> bytes:
    """L bytes, no '/', '+', '#', 'f' or 'g' (the fillers): the salt in the first three (an
    absent name's first byte from the alphabet's other half), a pattern in the rest."""
    al = b"0123456789abcdehijklmnopqrstuvwxyz"
    assert salt < 17 * 34 * 34
    head = (al[salt % 17 + (17 if absent else 0)], al[salt // 17 % 34], al[salt // 578 % 34])
    return bytes(head[i] if i < 3 else al[(7 * i + salt) % 34] for i in range(L))


def _pairs():
    """(key, name only looked up) near-miss pairs over bodies; `what` names the difference."""
    out = []

    def flip(s, i):
        return s[:i] + bytes((s[i] ^ 1,)) + s[i + 1:]
    for L in (1, 4, 5, 19, 20, 21, 24, 25, 45):
        k = _kbody(L, 900 + L)
        out.append(("last", k, flip(k, L - 1)))
    for at, lens in ((19, (20, 21, 30)), (20, (21, 30)), (21, (22, 30))):
        for L in lens:
            k = _kbody(L, 1000 + 50 * at + L)
            out.append(("byte%d" % at, k, flip(k, at)))
    for L in (3, 4, 19, 20, 21, 23, 24):
        k = _kbody(L, 1200 + L)
        out.append(("ext", k, k + b"x"))
        k = _kbody(L + 1, 1300 + L)
        out.append(("prefix", k, k[:-1]))
    k = _kbody(45, 1400)
    out.append(("byte40", k, flip(k, 40)))
    return out


@functools.lru_cache(maxsize=None)
def probe_batch(tail: int):
    """(names, keys): names to look up (packed in this order) and the route keys present.  tail
    0: the whole K family; 1..3: a short batch.  The last name is a key with len % 4 == tail."""
    names, keys, st = [], {}, {"off": 0, "fill": 0, "at": set()}

    def put(nm, present):
        if present:
            keys[nm] = None
        names.append(nm)
        st["off"] += len(nm)

    def at(r):  # fillers are keys and absent names in turn
        st["fill"] += 1
        k = _fill(st["off"], r)
        put((b"f" if st["fill"] % 2 else b"g") * k, bool(st["fill"] % 2))

    for wild in (False, True):
        pre = b"+/" if wild else b""
        for L in (K_LENS if tail == 0 else (19, 20, 21)):
            for r in K_RES:
                at(r)
                st["at"].add((wild, L, r, st["off"] % 16))
                put(pre + _kbody(L, 40 * L + r), True)
                if L:
                    at(r)
                    put(pre + _kbody(L, 40 * L + r, absent=True), False)
        if tail == 0:
            for what, k, nm in _pairs():
                for r in range(4):
                    at(r + 4 * (len(k) % 4))
                    put(pre + k, True)
                    at(r + 4 * (len(k) % 4))
                    put(pre + nm, False)
    at(tail)  # (the last name at a residue that changes with it)
    put(_kbody(24 + tail, 7777), True)
    keys = tuple(keys)
    ks = set(keys)
    # coverage, from the inputs
    if tail == 0:
        assert {x[:3] for x in st["at"]} == {(w, L, r) for w in (False, True) for L in K_LENS
                                             for r in K_RES}
        assert all(x[2] == x[3] for x in st["at"])
        assert {w for w, _, _ in _pairs()} == {"last", "byte19", "byte20", "byte21", "ext",
                                               "prefix", "byte40"}
    for what, k, nm in _pairs():
        assert k != nm and (tail or (k in ks and nm not in ks and b"+/" + nm not in ks))
        if what.startswith("byte"):
            assert len(k) == len(nm) and k[:int(what[4:])] == nm[:int(what[4:])]
    assert len(names[-1]) % 4 == tail and names[-1] in ks
    share = sum(nm in ks for nm in names) / len(names)
    assert 0.40 <= share <= 0.60, share
    assert len(names) <= 3000
    assert all(R.wildcard(k) == k.startswith(b"+/") for k in keys)
    return tuple(names), keys


def probe_keys(names_keys, kinds: str):
    """The keys of a probe batch that a `kinds` index ("plain", "wild", "both") holds."""
    return [k for k in names_keys[1] if kinds == "both" or (kinds == "wild") == k.startswith(b"+/")]
