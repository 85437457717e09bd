"""The post-walk kernels (k_verify, the row scan, k_scatter / k_scatter_grp, the legacy
verify + compaction) in every variant the engine can choose, each against the oracle's rows
bit for bit (row_ptr equal, ids equal per row once sorted).  tests/postwalk_cases.py builds the
index and the batches; tests/test_postwalk_cases_cpu.py asserts on the oracle that they reach
the branches: more than 16 pairs per topic (the grouped stores of k_scatter_grp), rows longer
than a 3-bit rank field (wide staging), rejects within and beyond the in-line limit.

The matrix: batch size (4,096: scan fused into k_scatter; 4,097; 6,000: several scatter steps
per block, a partial scan tile) x walk (pair walk, one lane per topic) x verification (none;
rejects adjusted in line; the legacy hand-over raised by the scatter itself) x staging (packed,
then wide by way of a rank-field overflow).  The engine's own counters say which path ran."""
import os

import numpy as np
import pytest

import postwalk_cases as P

pytestmark = pytest.mark.gpu

# verification case -> (Engine arguments, batch with few colliding decoys)
VERIFY = {
    "none": (dict(word_hash_bits=0), False),
    "inline": (dict(word_hash_bits=3), True),
    "legacy": (dict(word_hash_bits=3, reject_cap=16), False),
}


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _rows_sorted(row_ptr, ids):
    seg = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr.astype(np.int64)))
    return ids[np.lexsort((ids, seg))]


def _match_and_check(eng, n, few):
    tb, to, row, ids = P.expected(n, few)
    res = eng.match_packed(tb, to)
    assert np.array_equal(res.row_ptr, row)
    assert np.array_equal(_rows_sorted(res.row_ptr, res.filter_id), ids)


def _delta(eng, before):
    st = eng.stats()
    return {k: st[k] - before[k] for k in ("reruns", "rejected_pairs", "legacy_batches", "batches")}


@pytest.mark.parametrize("verify", list(VERIFY))
@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("n", P.SIZES)
def test_postwalk_variants_vs_oracle(emqx, n, pair, verify):
    # both are read once per process and would silently select the A/B kernels
    assert "EMQXGM_SCATTER_DIRECT" not in os.environ and "EMQXGM_STAGE_WIDE" not in os.environ
    kw, few = VERIFY[verify]
    eng = emqx.Engine(**kw)
    for i, f in enumerate(P.filters()):
        assert eng.trie_insert(f) == i  # the oracle's ids
    eng.commit()
    eng.tune("walk_pair", pair)
    legacy = 1 if verify == "legacy" else 0
    want_rej = P.predicted_rejects(n, few) if verify == "inline" else 0

    def check(what, reruns):
        st = eng.stats()
        _match_and_check(eng, n, few)
        d = _delta(eng, st)
        print(f"postwalk n={n} pair={pair} verify={verify} {what}: {d}")
        assert d["batches"] == 1
        if verify == "inline":
            assert 1 <= d["rejected_pairs"] <= P.REJ_SCAN_MAX and d["legacy_batches"] == 0
            assert d["rejected_pairs"] == want_rej  # exactly the pairs only a token collision staged
        elif verify == "legacy":
            assert d["legacy_batches"] == 1
        else:
            assert d["rejected_pairs"] == 0 and d["legacy_batches"] == 0
        if reruns is not None:
            assert d["reruns"] == reruns + legacy  # (the hand-over redoes the pass once)

    try:
        # (the first pass of an index may also be redone with a deeper walk stack, kept for the
        # epoch: the filters' frontier doubles per level)
        check("packed", None)
        eng.tune("stage_rank_bits", 3)
        check("rank overflow, redone wide", 1)
        check("wide", 0)  # the epoch stays wide: no redo
    finally:
        eng.tune("stage_rank_bits", 0)
        eng.close()
