"""tests/fb_cases.py judged on its inputs and on the oracle alone: every length class is there at
the four pool residues, every edge filter is matched by its own topic and by no other, each window
plan has the pair count it claims, the sweeps straddle the capacities read from the engine, and
the reference's offsets and bytes are consistent with a plain per-pair restatement."""
import numpy as np

import fb_cases as F
from oracle import emqx_ref as R


def test_every_length_is_present_four_times_at_every_residue():
    for rot in (0, 1):
        seen, off = {}, 0
        for f, info in F.edge_set(rot):
            if info:
                L, k, res = info
                assert len(f) == L and off % 4 == res
                seen.setdefault(L, []).append(res)
            else:
                assert len(f) in (2, 3) and f[:1] in (b"~", b"^", b"!")
            off += len(f)
        assert set(seen) == set(F.LENS)
        for L, rs in seen.items():
            # ('#', '+' and '$' are the only one-byte filters a topic can match: see fb_cases)
            assert sorted(rs) == ([0, 1, 2, 3] if L > 1 else sorted((k + rot) % 4 for k in range(3)))
    one = {i[2] for r in (0, 1) for _, i in F.edge_set(r) if i and i[0] == 1}
    assert one == {0, 1, 2, 3}
    # all_filters() starts with the set, so these are the offsets of an engine's pool
    es = F.edge_set(0)
    assert F.all_filters()[:len(es)] == tuple(f for f, _ in es)
    assert F.MAX_LEN in F.LENS and max(len(f) for f in F.all_filters()) == F.MAX_LEN


def test_each_edge_filter_is_matched_by_exactly_its_own_topic():
    topics = F.edge_topics()
    assert len(set(topics)) == len(topics) == 4 * (len(F.LENS) - 1) + 1
    edge = {f: i for f, i in F.edge_set(0) if i}
    hits = {f: [] for f in edge}
    for t in topics:
        row = F.row_of(t)
        assert set(row) <= set(edge), t[:40]
        for f in row:
            hits[f].append(t)
            assert R.match(t, f)
        one_level = not t.startswith(b"$")
        assert (b"#" in row) == one_level and (b"+" in row) == one_level
        assert len(row) == (3 if one_level else 1)
    for f, (L, k, _) in edge.items():
        if f in (b"#", b"+"):
            assert len(hits[f]) == 4 * (len(F.LENS) - 2)
        else:
            assert hits[f] == [F.edge_topic(L, k)], f[:40]
    # the limit case is one topic per filter: 65533 bytes matched by 65535
    assert sum(len(t) == F.MAX_LEN - 2 for t in topics) == 4
    # pads and miss names never take part
    pads = [f for f, i in F.edge_set(0) if not i]
    # (a literal is returned for a one-word '$' topic only, and a pad as a topic gets no pad back)
    assert pads and not any(R.wildcard(p) or p[:1] == b"$" or p in F.row_of(p) for p in pads)
    assert not any(F.row_of(F.miss(i)) for i in range(0, 4500, 97))
    # a zero-length filter is not one the oracle returns: no case for it (fb_cases docstring)
    t = R.Trie()
    t.insert(b"")
    assert t.match(b"") == []


def test_dense_and_sweep_families():
    assert [len(F.row_of(F.m_topic(s))) for s in range(10)] == [1, 2, 4, 8, 16, 32, 64, 128, 256, 511]
    assert F.fresh_caps(1) == (260, 4249) and F.fresh_caps(800)[0] == F.FB_SMALL_PAIRS
    assert F.fresh_caps(900) == (4576, 142336) and F.fresh_caps(801)[0] > F.FB_SMALL_PAIRS
    cap_p, cap_b = F.fresh_caps(1)
    assert F.K_SWEEP[0] < cap_p < F.K_SWEEP[-1] and F.B_SWEEP[0] < cap_b < F.B_SWEEP[-1]
    for d, k in enumerate(F.K_SWEEP):
        row = F.row_of(F.k_topic(d))
        assert len(row) == k and set(row) == set(F.k_filters(d))
        assert sum(len(f) for f in row) < cap_b - 32
    for j, b in enumerate(F.B_SWEEP):
        row = F.row_of(F.b_topic(j))
        assert len(row) == 2 and sum(len(f) for f in row) == b


def test_each_plan_has_the_pair_count_it_claims():
    plans = F.plans()
    for name, (topics, pairs) in plans.items():
        assert F.pairs_of(topics) == pairs, name
    assert {c for _, c in plans.values()} >= set(F.PAIR_COUNTS)
    n = {k: len(t) for k, (t, _) in plans.items()}
    assert n["empty"] == 0 and n["sparse-small"] > 100 * plans["sparse-small"][1]
    assert n["sparse-big"] > F.SCAN_TILE and plans["sparse-big"][1] < 10
    assert plans["dense"][1] > 500 * n["dense"]
    # the fresh-pipe windows sit where their names say (fb_cases.fresh_caps)
    for name, fits in (("small-4096", True), ("small-4097", False), ("pack-4097", True),
                       ("sparse-small", True), ("sparse-big", True)):
        cap_p, cap_b = F.fresh_caps(n[name])
        assert (plans[name][1] <= cap_p) == fits and F.bytes_of(plans[name][0]) <= cap_b, name
        assert (cap_p <= F.FB_SMALL_PAIRS) == (name != "pack-4097" and name != "sparse-big")
    # every edge filter travels in the tile-edge windows, and some topics are route keys
    for name in ("lengths", "p4095", "p4096", "p4097", "p8193"):
        assert set(F.edge_topics()) <= set(plans[name][0])
    keys = set(F.route_keys())
    for name in ("lengths", "sparse-small", "sparse-big", "p8193", "p0"):
        assert keys & set(plans[name][0]), name
    assert max(n.values()) <= 4500 and max(c for _, c in plans.values()) == 8193


def test_reference_offsets_and_bytes_are_self_consistent():
    fid = {f: i for i, f in enumerate(F.all_filters())}
    keys = {k: 10_000 + i for i, k in enumerate(F.route_keys())}
    for name in ("empty", "p0", "p17", "lengths", "p4097"):
        topics = F.plans()[name][0]
        row, ids, exact, foff, by = F.expected(topics, fid, keys)
        assert row[0] == 0 and row[-1] == len(ids) == F.plans()[name][1]
        assert foff[0] == 0 and foff[-1] == len(by) and (np.diff(foff) >= 0).all()
        # pair by pair, in plain Python
        flat = [f for t in topics for f in sorted(F.row_of(t), key=fid.get)]
        assert [fid[f] for f in flat] == ids.tolist()
        assert by.tobytes() == b"".join(flat)
        assert foff.tolist() == [0] + list(np.cumsum([len(f) for f in flat], dtype=np.int64))
        assert [int(e) for e in exact] == [keys.get(t, F.NONE) for t in topics]
    # delta filters: matched by their topics once they are in, invisible before
    for t, f in zip(F.delta_topics(), [f for f in F.delta_filters() if f.endswith(b"/#")]):
        assert f in F.row_of(t, delta=True) and f not in F.row_of(t)
        assert len(F.row_of(t, delta=True)) == 3
