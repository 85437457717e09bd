"""Inputs aimed at the filter-byte gather (emqx_amd/csrc/gm_kernels.hip: k_filter_len,
k_filter_gather, k_fb_pack, k_fb_small, their shared copy_filter, and the device-counted length
scan; the host's sizing and fallback in gm_engine.cpp: host_pipe_enqueue_gather, host_pipe_gather,
host_pipe_complete, FbLayout), with the reference they are judged by.  Shared by the CPU test of
the cases (test_fb_cases_cpu.py) and the device test (test_gpu_filter_bytes.py).  Deterministic,
pure Python / numpy; nothing here comes from a device.

Filters, in insertion order (a filter's id is its position: all_filters()):

  E  the edge set for copy_filter.  Lengths LENS; for L >= 3 the four filters <c><'x'*(L-3)>/#,
     c in a..d, each matched by the topic equal to its prefix ("p/#" matches "p"), so the
     65535-byte filter (the engine's length limit) by a 65533-byte topic.  These topics have one
     level, so '#' and '+' match them too.  For L = 2 the literals $a..$d: emqx_trie returns a
     literal only for a one-word '$' topic (emqx_trie.erl:286-287), which '#' and '+' do not
     match.  For L = 1 '#', '+' and '$': no fourth one-byte filter exists that any topic matches,
     so this class alone has three members.  Never-matched pad literals of 2 and 3 bytes ('~',
     '^' or '!' first) stand in front of each edge filter so that member k of a class lies at
     pool offset (k + rot) mod 4: the host pool is the filters' bytes concatenated, filter 0 at
     offset 0, and the device pool mirrors it.  rot = 0 is the set every engine gets; the L = 1
     class reaches its fourth residue in edge_set(1), which a test commits alone.
  M  511 filters $m/<9 levels, each 'a' or '+', at least one '+'>, 20 bytes each: the topic
     $m/<s times a, then b> matches 2^s of them (511 for s = 9) -- many pairs from few topics.
  K  for the pair-capacity sweep: family d = 0..9 has exactly K0 + d filters $<d>/..., all
     matching the one topic $<d>/a/a/a/a/a/a/a (7-level masks of 'a' / '+', and their prefixes
     closed by '/#'; the shortest first, so that the pairs' bytes stay below the byte capacity).
  B  for the byte-capacity sweep: $y/#  (4 bytes) and one $y/<j><'x'...>/# per total, matched by
     the topic $y/<j><'x'...>: two pairs whose bytes add up to B0 + j.

No zero-length filter: the oracle never returns it (a literal is returned only for a one-word
'$' topic), so copy_filter's n == 0 branch has no case the reference could judge.

Names `$n/<i>` match nothing.  Route keys (route_keys()) are some of the topics, registered after
every filter so that they move no filter's pool offset.

The two capacities of a fresh pipe are read from host_pipe_enqueue_gather (fresh_caps); the sweeps
are centred on them and the device test checks that the fallback switches exactly there.
"""
import functools

import numpy as np

from oracle import emqx_ref as R

NONE = 0xFFFFFFFF
LENS = ((1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17) + tuple(range(27, 38)) + tuple(range(63, 69)) +
        tuple(range(95, 101)) + (255, 256, 257, 1023, 65535))
MAX_LEN = 65535          # gm_engine.cpp trie_insert_locked: emqx_topic.erl:47 MAX_TOPIC_LEN
SCAN_TILE = 4096         # gm_kernels.hip: WG * SCAN_ITEMS; = FB_SMALL_PAIRS (gm_kernels.h)
FB_SMALL_PAIRS = 4096
PAIR_COUNTS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8193)
CH = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"


def fresh_caps(n: int):
    """(want_p, want_b) of host_pipe_enqueue_gather for a window of n topics on a pipe without
    history (fb_ppt = fb_bpp = 0: 4 pairs per topic, 32 bytes per pair), in its own double
    arithmetic.  The pass's staging capacity (at least 2^20 pairs) never binds here."""
    exp_p = 4.0 * n
    return int(1.2 * exp_p) + 256, int(1.2 * 32.0 * exp_p) + 4096


K0 = fresh_caps(1)[0] - 4    # the pair sweep: K0 .. K0 + 9 pairs around the capacity (260)
B0 = fresh_caps(1)[1] - 4    # the byte sweep: B0 .. B0 + 8 bytes around the capacity (4249)
K_SWEEP = tuple(range(K0, K0 + 10))
B_SWEEP = tuple(range(B0, B0 + 9))


def _pad(i: int, size: int) -> bytes:
    assert size in (2, 3) and i < 3 * 62
    p = bytes((b"~^!"[i // 62], CH[i % 62]))
    return p if size == 2 else p + b"~"


def edge_topic(L: int, k: int) -> bytes:
    if L == 1:
        return (None, None, b"$")[k]   # '#' and '+' have no topic of their own
    if L == 2:
        return b"$" + b"abcd"[k:k + 1]
    return b"abcd"[k:k + 1] + b"x" * (L - 3)


def edge_filter(L: int, k: int, chars: bytes = b"abcd") -> bytes:
    if L == 1:
        return (b"#", b"+", b"$")[k]
    if L == 2:
        return b"$" + chars[k:k + 1]
    return chars[k:k + 1] + b"x" * (L - 3) + b"/#"


@functools.lru_cache(maxsize=None)
def edge_set(rot: int = 0):
    """((filter, info), ...) in insertion order; info = (L, k, residue) for an edge filter, None
    for a pad.  The residue is the filter's offset mod 4 in a pool that starts with this set."""
    out, off, npad = [], 0, [0, 0]
    for L in LENS:
        for k in range(3 if L == 1 else 4):
            want = (k + rot) % 4
            for size in {0: (), 1: (2, 3), 2: (2,), 3: (3,)}[(want - off) % 4]:
                out.append((_pad(npad[size - 2], size), None))
                npad[size - 2] += 1
                off += size
            assert off % 4 == want
            f = edge_filter(L, k)
            assert len(f) == L <= MAX_LEN
            out.append((f, (L, k, want)))
            off += L
    fs = [f for f, _ in out]
    assert len(set(fs)) == len(fs)
    return tuple(out)


DELTA_LENS = (3, 4, 5, 16, 17, 31, 32, 33, 64, 65, 255, 256, 257, 1023)


@functools.lru_cache(maxsize=None)
def delta_filters():
    """Further edge filters (first bytes e..h) for a second commit, 3-byte pads between them (the
    first as well: after all_filters() and route_keys() they lie where the pool then ends)."""
    out = []
    for i, L in enumerate(DELTA_LENS):
        for k in range(4):
            if (i + k) % 3 == 0:
                out.append(b"!" + bytes((CH[i], CH[k])))
            out.append(edge_filter(L, k, b"efgh"))
    return tuple(out)


def delta_topics():
    return tuple(b"efgh"[k:k + 1] + b"x" * (L - 3) for L in DELTA_LENS for k in range(4))


def m_topic(s: int) -> bytes:
    """Matches 2^s of the M filters (all 511 for s = 9)."""
    return b"$m" + b"/a" * s + b"/b" * (9 - s)


def _masks(levels: int):
    return [b"".join(b"/+" if m >> j & 1 else b"/a" for j in range(levels))
            for m in range(1 << levels)]


@functools.lru_cache(maxsize=None)
def m_filters():
    fs = tuple(b"$m" + m for m in _masks(9) if b"+" in m)
    assert len(fs) == 511 and all(len(f) == 20 for f in fs)
    return fs


def k_topic(d: int) -> bytes:
    return b"$%d" % d + b"/a" * 7


@functools.lru_cache(maxsize=None)
def k_filters(d: int):
    """The K0 + d shortest wildcard filters that match k_topic(d)."""
    cand = [m + b"/#" for lv in range(8) for m in _masks(lv)]
    cand += [m for m in _masks(7) if b"+" in m]
    cand.sort(key=lambda f: (len(f), f))
    fs = tuple(b"$%d" % d + f for f in cand[:K_SWEEP[d]])
    assert len(fs) == len(set(fs)) == K_SWEEP[d]
    # the pairs' bytes stay clear of the byte capacity: only the pair count moves the outcome
    assert sum(len(f) for f in fs) <= fresh_caps(1)[1] - 64
    return fs


def b_topic(j: int) -> bytes:
    return b"$y/%d" % j + b"x" * (B_SWEEP[j] - 10)   # "$y/#" + "$y/<j>" + "/#": 10 bytes


def b_filter(j: int) -> bytes:
    f = b_topic(j) + b"/#"
    assert len(f) + len(b"$y/#") == B_SWEEP[j]
    return f


@functools.lru_cache(maxsize=None)
def all_filters():
    fs = [f for f, _ in edge_set(0)]
    fs += m_filters()
    for d in range(len(K_SWEEP)):
        fs += k_filters(d)
    fs += [b"$y/#"] + [b_filter(j) for j in range(len(B_SWEEP))]
    assert len(set(fs)) == len(fs) and len(fs) <= 4500
    return tuple(fs)


def miss(i: int) -> bytes:
    return b"$n/%d" % i


@functools.lru_cache(maxsize=None)
def edge_topics():
    """Every edge topic: each L >= 3 four times, $a..$d, and '$'."""
    return tuple(edge_topic(L, k) for L in LENS for k in range(3 if L == 1 else 4)
                 if edge_topic(L, k) is not None)


def _short_edges(count: int, start: int = 0):
    """Edge topics of three pairs each (own filter, '#', '+'), the 65533-byte ones left out."""
    ts = [edge_topic(L, (i + start) % 4) for i, L in enumerate(LENS[2:-1])]
    return ts[start:start + count]


@functools.lru_cache(maxsize=None)
def route_keys():
    """Topics that are route keys too (non-NONE exact ids in the block): every fifth edge topic
    below 300 bytes, every third miss name below 30, two M topics."""
    ks = [t for t in edge_topics() if len(t) < 300][::5]
    ks += [miss(i) for i in range(0, 30, 3)] + [m_topic(9), m_topic(3)]
    assert len(set(ks)) == len(ks)
    return tuple(ks)


# ---- the reference ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trie(delta: bool, rot: int):
    trie = R.Trie()
    for f in ([f for f, _ in edge_set(rot)] if rot else all_filters()):
        trie.insert(f)
    if delta:
        for f in delta_filters():
            trie.insert(f)
    return trie


@functools.lru_cache(maxsize=None)
def row_of(topic: bytes, delta: bool = False, rot: int = 0):
    """The filters oracle.emqx_ref's trie returns for the topic, sorted.  Over all_filters(), with
    delta_filters() too (delta), or over edge_set(rot) alone (rot != 0)."""
    return tuple(sorted(_trie(delta, rot).match(topic)))


def pair_bytes(ids, tab_off, tab_pool):
    """(foff, bytes) of pairs in the given order from an id -> bytes table held as one pool
    (filter i = tab_pool[tab_off[i]:tab_off[i + 1]]): foff is the exclusive prefix sum of the
    pairs' lengths, bytes their concatenation."""
    ids = np.asarray(ids, np.int64)
    start, lens = tab_off[ids], tab_off[ids + 1] - tab_off[ids]
    foff = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(lens, out=foff[1:])
    idx = np.repeat(start - foff[:-1], lens) + np.arange(int(foff[-1]), dtype=np.int64)
    return foff, tab_pool[idx]


def table(fid):
    """{filter: id} as (tab_off, tab_pool) for pair_bytes; ids without a filter have no bytes."""
    lens = np.zeros(max(fid.values()) + 1, np.int64)
    by_id = sorted((i, f) for f, i in fid.items())
    for i, f in by_id:
        lens[i] = len(f)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    pool = np.zeros(int(off[-1]), np.uint8)
    for i, f in by_id:
        pool[off[i]:off[i + 1]] = np.frombuffer(f, np.uint8)
    return off, pool


def expected(topics, fid, keys=None, delta: bool = False, rot: int = 0):
    """(row, ids, exact, foff, bytes) of a window: row pointers, each row's filter ids ascending,
    exact ids, and the pairs' byte offsets and bytes in that order.  fid: {filter: id}, keys:
    {route key: id}; both are the caller's own records of what it inserted."""
    rows = [sorted(fid[f] for f in row_of(t, delta, rot)) for t in topics]
    row = np.zeros(len(topics) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=row[1:])
    ids = np.array([i for r in rows for i in r], np.uint32)
    exact = np.array([(keys or {}).get(t, NONE) for t in topics], np.uint32)
    foff, by = pair_bytes(ids, *table(fid))
    assert foff[0] == 0 and foff[-1] == len(by) and len(foff) == len(ids) + 1
    return row, ids, exact, foff, by


def pairs_of(topics, delta: bool = False, rot: int = 0) -> int:
    return sum(len(row_of(t, delta, rot)) for t in topics)


def bytes_of(topics) -> int:
    return sum(len(f) for t in topics for f in row_of(t))


# ---- the window plans ---------------------------------------------------------------------------

def _fill(base, target: int):
    """base plus M topics (and the one-pair '$a') up to exactly `target` pairs."""
    ts, r = list(base), target - pairs_of(base)
    assert r >= 0
    ts += [m_topic(9)] * (r // 511)
    r %= 511
    ts += [m_topic(s) for s in range(9) if r >> s & 1]
    return ts


def _spread(dense, n: int):
    """The dense topics spread evenly among miss names, n topics in all."""
    ts = [miss(i) for i in range(n - len(dense))]
    step = max(1, len(ts) // (len(dense) + 1))
    for j, t in enumerate(dense):
        ts.insert((j + 1) * step + j, t)
    assert len(ts) == n
    return ts


@functools.lru_cache(maxsize=None)
def plans():
    """{name: (topics, pairs)}; the pair count is the one the plan is built for, checked against
    the oracle by the CPU test and again before the first device call."""
    e = list(edge_topics())
    p = {
        "empty": ([], 0),
        "p0": ([miss(i) for i in range(5)], 0),
        "p1": ([miss(0), b"$a", miss(1)], 1),
        "p15": (_short_edges(5), 15),
        "p16": (_short_edges(5, 5) + [b"$b"], 16),
        "p17": ([b"$c"] + _short_edges(5, 10) + [b"$"], 17),
        # every edge filter once, among them the four 65535-byte ones
        "lengths": (e, 3 * (len(e) - 5) + 5),
        # far more topics than pairs: for the small kernel, and for k_fb_pack (its grid follows
        # max(cap_p, n) + 1) with more than SCAN_TILE topics
        "sparse-small": (_spread(_short_edges(1, 20), 301), 3),
        "sparse-big": (_spread([b"$d"] + _short_edges(2, 24), 4500), 7),
        # far more pairs than topics
        "dense": ([m_topic(9)] * 3, 1533),
        # the scan's tile edges, every edge filter in them
        "p4095": (_fill(e, 4095), 4095),
        "p4096": (_fill(e, 4096), 4096),
        "p4097": (_fill(e, 4097), 4097),
        "p8193": (_fill(e, 8193), 8193),
        # fresh-pipe windows (fresh_caps): 800 topics are the most whose block k_fb_small packs,
        # with room for exactly FB_SMALL_PAIRS pairs; 900 topics go to the device-counted scan
        # and k_fb_pack with room for 4576 pairs
        "small-4096": (_spread(_fill([], 4096), 800), 4096),
        "small-4097": (_spread(_fill([], 4097), 800), 4097),
        "pack-4097": (_spread(_fill([], 4097), 900), 4097),
    }
    assert {c for _, c in p.values()} >= set(PAIR_COUNTS)
    return {k: (tuple(t), c) for k, (t, c) in p.items()}


def pack(items, off_dtype=np.uint32):
    off = np.zeros(len(items) + 1, off_dtype)
    np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), np.uint8).copy(), off
