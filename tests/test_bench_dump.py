"""bench.py --dump-outputs, the host half (bench._write_outputs): which topics of a batch's CSR are
written, in which formats, and that the files stay inside the size limit.  CPU only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

NONE = 0xFFFFFFFF


def _csr(nt, max_len, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, nt)
    row = np.zeros(nt + 1, np.uint32)
    np.cumsum(lens, out=row[1:])
    fid = rng.integers(0, 2**32 - 1, int(row[-1]), dtype=np.uint32)  # ids past 2^24: f64 on disk
    exact = np.where(rng.random(nt) < 0.3, rng.integers(0, 2**31, nt), NONE).astype(np.uint32)
    words = rng.integers(1, 9, nt).astype(np.uint32)
    return row, fid, exact, words


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def _check(out, row, fid, exact, words):
    sel = out["topics"].astype(np.int64)
    assert np.all(np.diff(sel) > 0)
    assert out["n_pairs"].tolist() == [float(len(fid))]
    assert np.array_equal(out["row_len"], (row[sel + 1].astype(np.int64) - row[sel]))
    assert np.array_equal(out["exact_id"], exact[sel].astype(np.float64))
    assert np.array_equal(out["n_words"], words[sel])
    want = np.concatenate([np.sort(fid[row[i]:row[i + 1]]) for i in sel] + [np.zeros(0, np.uint32)])
    assert np.array_equal(out["filter_id"], want.astype(np.float64))
    assert {k: v.dtype for k, v in out.items()} == {
        "n_pairs": np.float64, "topics": np.float64, "row_len": np.float32,
        "filter_id": np.float64, "exact_id": np.float64, "n_words": np.float32}


def test_small_batch_is_written_whole(tmp_path):
    row, fid, exact, words = _csr(1000, 5, 1)
    bench._write_outputs(str(tmp_path / "d"), row, fid, exact, words)
    out = _load(tmp_path / "d")
    assert np.array_equal(out["topics"], np.arange(1000))
    _check(out, row, fid, exact, words)


def test_empty_rows_and_no_pairs(tmp_path):
    row = np.zeros(8, np.uint32)
    z = np.zeros(0, np.uint32)
    bench._write_outputs(str(tmp_path / "d"), row, z, np.full(7, NONE, np.uint32), np.ones(7, np.uint32))
    out = _load(tmp_path / "d")
    assert out["filter_id"].size == 0 and out["n_pairs"].tolist() == [0.0]
    assert np.array_equal(out["exact_id"], np.full(7, float(NONE)))


def test_large_batch_is_sampled_the_same_way_every_time(tmp_path, monkeypatch):
    """More topics than DUMP_ROWS: a seeded sample, the same in every run; halved until the files
    fit DUMP_MAX_BYTES."""
    monkeypatch.setattr(bench, "DUMP_ROWS", 512)
    row, fid, exact, words = _csr(5000, 6, 2)
    bench._write_outputs(str(tmp_path / "a"), row, fid, exact, words)
    bench._write_outputs(str(tmp_path / "b"), row, fid, exact, words)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a["topics"].size == 512
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _check(a, row, fid, exact, words)
    # a limit that 512 rows (about 3 pairs each: ~24 KB of ids) exceed
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16384)
    bench._write_outputs(str(tmp_path / "c"), row, fid, exact, words)
    c = _load(tmp_path / "c")
    assert 0 < c["topics"].size < 512
    _check(c, row, fid, exact, words)
    size = sum(os.path.getsize(tmp_path / "c" / n) for n in os.listdir(tmp_path / "c"))
    assert size <= 16384


def test_row_pointers_that_do_not_fit_the_pairs_are_refused(tmp_path):
    row, fid, exact, words = _csr(100, 4, 3)
    with pytest.raises(RuntimeError):
        bench._write_outputs(str(tmp_path / "d"), row, fid[:-1], exact, words)
