"""verify_one's size switch and window alignment (emqx_amd/csrc/gm_verify.inc) against the
oracle: filters of 59/60/61 bytes (inline record against string pool), topics of 63/64/65 bytes
(LDS window against global memory) at every 16-byte residue of the packed batch, true matches
beside near misses that one-bit tokens let through to the byte check
(tests/verify_edge_cases.py).  Once with the rejects adjusted in line (k_verify decides), once
with a reject capacity of 16 (the legacy pass: k_verify_scatter decides the same pairs)."""
import numpy as np
import pytest

import postwalk_cases as P
import verify_edge_cases as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _rows_sorted(row_ptr, ids):
    seg = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr.astype(np.int64)))
    return ids[np.lexsort((ids, seg))]


@pytest.mark.parametrize("reject_cap", [0, 16])
def test_verify_window_edges_vs_oracle(emqx, reject_cap):
    fs = V.filters()
    eng = emqx.Engine(word_hash_bits=V.BITS, reject_cap=reject_cap)
    for i, f in enumerate(fs):
        assert eng.trie_insert(f) == i
    eng.commit()
    ref = P.ref_index(fs)
    for fam, tl in V.batches():
        topics, info = V.batch(fam, tl)
        tb, to = P.pack(list(topics), np.uint32)
        assert all(to[i] % 16 == x[1] for i, x in enumerate(info) if x)
        row, ids, _ = ref.match(tb, to, threads=8)
        n_true = sum(1 for x in info if x and x[2] == "true")
        assert row[-1] == n_true  # (each match matches its own filter alone)
        want_rej = P.staged_pairs(fs, topics, V.BITS) - n_true
        assert sum(1 for x in info if x and x[2] != "true") <= want_rej <= P.REJ_SCAN_MAX
        st = eng.stats()
        res = eng.match_packed(tb, to)
        d = {k: eng.stats()[k] - st[k] for k in ("rejected_pairs", "legacy_batches", "reruns")}
        print(f"verify edges {fam} tl={tl} reject_cap={reject_cap}: predicted {want_rej}, {d}")
        assert np.array_equal(res.row_ptr, row)
        assert np.array_equal(_rows_sorted(res.row_ptr, res.filter_id), ids)
        if reject_cap:
            assert d["legacy_batches"] == 1
        else:
            assert d["rejected_pairs"] > 0 and d["legacy_batches"] == 0
            assert d["rejected_pairs"] == want_rej
    eng.close()
