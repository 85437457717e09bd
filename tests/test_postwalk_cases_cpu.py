"""The inputs of the post-walk variant matrix (tests/postwalk_cases.py) reach the code they are
meant for, judged on the CPU oracle alone: enough pairs per topic for the grouped scatter, rows
longer than a 3-bit rank field, and reject counts on either side of the in-line limit."""
import numpy as np
import pytest

import postwalk_cases as P
import verify_edge_cases as V


@pytest.mark.parametrize("fam,tl", V.batches())
def test_verify_edge_batches_cover_their_edges(fam, tl):
    """Lengths and residues are asserted by the builder from the inputs; here: every near miss
    is staged under one-bit tokens, and the rejects of a batch stay within the in-line limit (so
    that k_verify's answers, not the legacy pass's, make the rows)."""
    topics, info = V.batch(fam, tl)
    fs = V.filters()
    assert sorted(len(f) for f in fs) == [59, 59, 60, 60, 61, 61]
    n_true = sum(1 for x in info if x and x[2] == "true")
    n_near = sum(1 for x in info if x and x[2] != "true")
    assert (n_true, n_near) == (48, 768)
    rej = P.staged_pairs(fs, topics, V.BITS) - n_true
    assert n_near <= rej <= P.REJ_SCAN_MAX, rej
    assert rej > 16  # past Engine(reject_cap=16)


def test_sizes_and_index():
    assert P.SIZES == (4096, 4097, 6000)  # the fused scan's last size, the first past it, a partial tile
    assert len(P.filters()) == 127
    # word_token of emqx_amd/csrc/gm_common.h with test masks 7 and 1, computed by the header
    pinned = {b"a": (3, 1), b"d00": (4, 0), b"d01": (7, 1), b"d07": (1, 1), b"d23": (1, 1),
              b"long-word-1": (0, 0), b"u6000": (0, 0)}
    for w, (t3, t1) in pinned.items():
        assert (P.word_token_bits(w, 3), P.word_token_bits(w, 1)) == (t3, t1), w


@pytest.mark.parametrize("few", [False, True])
@pytest.mark.parametrize("n", P.SIZES)
def test_batches_reach_the_grouped_scatter(n, few):
    tb, to, row, ids = P.expected(n, few)
    assert len(to) == n + 1 and len(row) == n + 1 and len(ids) == row[-1]
    cnt = np.diff(row.astype(np.int64))
    # GRP_MIN pairs per topic after any rejects are gone, with margin
    assert row[-1] >= 18 * n > P.GRP_MIN * n, row[-1] / n
    assert cnt.min() >= 1 and cnt.max() > 8  # no empty row; a rank past a 3-bit field
    assert (cnt > 8).mean() > 0.5
    levels = {t.count(b"/") + 1 for t in P.topics(n, few)}
    assert levels == set(range(1, 9))
    assert len(set(P.topics(n, few))) > n // 4


@pytest.mark.parametrize("n", P.SIZES)
def test_reject_counts_on_both_sides_of_the_inline_limit(n):
    few, full = P.predicted_rejects(n, True), P.predicted_rejects(n, False)
    assert 1 <= few <= P.REJ_SCAN_MAX, few     # adjusted in line by the scatter
    assert few > 64                            # (more than a handful of ranks move)
    assert full > 16                           # past Engine(reject_cap=16): the legacy hand-over
    # rows differ between the two batches only in decoys: the same pairs
    assert P.expected(n, True)[2][-1] == P.expected(n, False)[2][-1]
