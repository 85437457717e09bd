"""k_tok and the exact route-key probe (emqx_amd/csrc/gm_tok.inc) on the device, bit-exact
against the oracle, over the edge sweep of tests/tok_cases.py: word lengths around the inline /
hashed boundary at every level and batch residue, byte values around '/', near-miss words, tiles
at the LDS fit boundary, and route keys of 0..45 bytes at every dword residue with near misses
around the XINL = 20 inline bytes.

Expected rows are oracle.emqx_ref.Trie's over all case filters (tok_cases.expected_rows, computed
once); expected exact ids come from the key set.  Every entry path stages the bytes at another
address: the host API (the engine's own copy), the device API with the caller's pointer advanced
by 0, 1, 5 and 15 bytes, and the host pipes with and without copy-through."""
import ctypes

import numpy as np
import pytest

import postwalk_cases as P
import tok_cases as T

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
PATHS = ("host", "dev0", "dev1", "dev5", "dev15", "copy-through", "host-pipe-dma")


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


@pytest.fixture(scope="module")
def want():
    """{batch: (bytes, u32 offsets, row pointers, filter ids sorted per row)} on the oracle; a
    filter's id is its position in tok_filters() (the engines insert them in that order)."""
    fid = {f: i for i, f in enumerate(T.tok_filters())}
    out = {}
    for name, (topics, _) in T.tok_batches().items():
        rows = T.expected_rows(name)
        tb, to = P.pack(list(topics), np.uint32)
        row = np.zeros(len(topics) + 1, np.uint64)
        np.cumsum([len(r) for r in rows], out=row[1:])
        ids = np.array([i for r in rows for i in sorted(fid[f] for f in r)], np.uint32)
        for a in (tb, to, row, ids):
            a.setflags(write=False)
        out[name] = (tb, to, row, ids)
    return out


@pytest.fixture(scope="module", params=[(0, False), (0, True), (3, False), (3, True)],
                ids=["tokens", "tokens+plain-key", "3-bit", "3-bit+plain-key"])
def engine(emqx, request):
    """word_hash_bits 0 (production tokens) or 3 (every word hashed, the collisions restored by
    the byte verification); with a plain route key committed k_tok<DEFER> runs and k_exact
    after it, without one k_tok probes wildcard names itself."""
    bits, plain_key = request.param
    eng = emqx.Engine(word_hash_bits=bits)
    fb, fo = P.pack(list(T.tok_filters()), np.uint64)
    assert np.array_equal(eng.trie_insert_many(fb, fo), np.arange(len(fo) - 1))
    if plain_key:
        eng.route_ref(b"a/plain/route/key")
    eng.commit()
    yield eng
    eng.close()


def _rows_sorted(row_ptr, ids):
    seg = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr.astype(np.int64)))
    return ids[np.lexsort((ids, seg))]


def _check_rows(what, topics, row, fid, want_row, want_ids):
    """Row by row, the first topic that differs named by its first 60 bytes."""
    row = np.asarray(row).astype(np.uint64)
    if np.array_equal(row, want_row) and np.array_equal(_rows_sorted(row, fid), want_ids):
        return
    fs = T.tok_filters()
    for i, t in enumerate(topics):
        got = sorted(int(x) for x in fid[int(row[i]):int(row[i + 1])])
        exp = [int(x) for x in want_ids[int(want_row[i]):int(want_row[i + 1])]]
        assert got == exp, (what, i, t[:60].hex(), [fs[g][:60].hex() for g in got[:4]],
                            [fs[e][:60].hex() for e in exp[:4]])
    raise AssertionError((what, "row pointers differ"))


def _dev_to_host(d, n):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    row, fid = np.empty(n + 1, np.uint32), np.empty(d.n_pairs, np.uint32)
    ex = np.empty(n, np.uint32)
    for a, p in ((row, d.row_ptr), (fid, d.filter_id), (ex, d.exact_id)):
        if a.nbytes:
            assert hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0
    return row, fid, ex


def _mapped(a) -> bool:
    """Whether the runtime gives the host array a device address (pinned, mapped memory)."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipHostGetDevicePointer.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                            ctypes.c_uint]
    d = ctypes.c_void_p()
    return hip.hipHostGetDevicePointer(ctypes.byref(d), a.ctypes.data, 0) == 0 and bool(d.value)


def _on_device(tb, to, shift):
    """The packed batch in device memory, its bytes `shift` bytes into a larger tensor."""
    import torch
    big = torch.full((len(tb) + 64,), 0x2F, dtype=torch.uint8, device="cuda")
    big[shift:shift + len(tb)].copy_(torch.from_numpy(np.array(tb)))
    do = torch.from_numpy(np.array(to).view(np.int32)).cuda()
    torch.cuda.synchronize()
    assert big.data_ptr() % 16 == 0
    return big, do


@pytest.mark.parametrize("path", PATHS)
def test_tokeniser_edges_vs_oracle(engine, want, path):
    eng = engine
    for name, (topics, _) in T.tok_batches().items():
        tb, to, wrow, wids = want[name]
        n = len(topics)
        if path == "host":
            res = eng.match_packed(tb, to)
            row, fid, ex = res.row_ptr, res.filter_id, res.exact_id
        elif path.startswith("dev"):
            shift = int(path[3:])
            big, do = _on_device(tb, to, shift)
            d = eng.match_device(big.data_ptr() + shift, do.data_ptr(), n, int(to[-1]))
            row, fid, ex = _dev_to_host(d, n)
        else:
            # the host pipes (test_gpu_batcher reaches them the same way): a window in pinned
            # memory is read by k_tok's copy-through instantiation unless zc_topics is 0
            eng.tune("zc_topics", 65536 if path == "copy-through" else 0)
            hb, ho = eng.pinned(len(tb)), eng.pinned(n + 1, np.uint32)
            hb[:], ho[:] = tb, to
            # the engine's own conditions for reading a window in place (batch_submit): both
            # buffers have a device address, the bytes are 16-byte aligned, the window is small
            assert _mapped(hb) and _mapped(ho) and hb.ctypes.data % 16 == 0
            assert n <= 65536 and int(to[-1]) <= 8 << 20
            res, _, _ = eng.match_batch_wait_filters(eng.match_batch_submit(hb, ho, filters=True))
            eng.tune("zc_topics", 65536)
            row, fid, ex = res.row_ptr, res.filter_id, res.exact_id
        _check_rows((path, name), topics, row, fid, wrow, wids)
        assert (np.asarray(ex) == NONE).all(), (path, name)


def test_large_batch_nontemporal_records(emqx, want):
    """TOK_NT_MIN = 2 Mi topics: from there k_tok stores its records non-temporally.  The main
    batch repeated to just over 2 Mi topics; every repetition's rows are the small batch's."""
    tb, to, wrow, wids = want["main"]
    n = len(to) - 1
    reps = (2 << 20) // n + 1
    assert reps * n >= (2 << 20) and reps * int(to[-1]) < 1 << 31
    eng = emqx.Engine()
    fb, fo = P.pack(list(T.tok_filters()), np.uint64)
    eng.trie_insert_many(fb, fo)
    eng.commit()
    small = eng.match_packed(tb, to)
    _check_rows("small", T.tok_batches()["main"][0], small.row_ptr, small.filter_id, wrow, wids)
    big_b = np.tile(tb, reps)
    big_o = np.empty(reps * n + 1, np.uint32)
    big_o[:-1] = (np.arange(reps, dtype=np.uint32)[:, None] * np.uint32(to[-1]) + to[None, :-1]).ravel()
    big_o[-1] = reps * int(to[-1])
    res = eng.match_packed(big_b, big_o, copy=False)
    cnt = np.diff(res.row_ptr.astype(np.int64)).reshape(reps, n)
    assert (cnt == np.diff(wrow.astype(np.int64))[None, :]).all()
    ids = _rows_sorted(res.row_ptr, res.filter_id).reshape(reps, len(wids))
    assert (ids == wids[None, :]).all()
    assert (res.exact_id == NONE).all()
    eng.close()


@pytest.mark.parametrize("range_kb", [0, 1])
@pytest.mark.parametrize("full_bits", [64, 2])
@pytest.mark.parametrize("kinds", ["plain", "wild", "both"])
def test_probe_edges_vs_key_set(emqx, kinds, full_bits, range_kb):
    """Every K-family name gets its key's id or NONE from the pass (k_exact, or k_xhash +
    k_exact_part with range_kb 1, and k_tok's own probe of wildcard names without plain keys),
    and from emqxgm_exact_owned_device exactly by the part emqxgm_key_owners names."""
    import torch
    eng = emqx.Engine(full_hash_bits=full_bits)
    eng.tune("exact_range_kb", range_kb)
    ids = {}
    for tail in range(4):
        for k in T.probe_keys(T.probe_batch(tail), kinds):
            ids[k] = eng.route_ref(k)
    eng.commit()
    for tail in range(4):
        names = T.probe_batch(tail)[0]
        exp = np.array([ids.get(nm, NONE) for nm in names], np.uint32)
        # (half of the names are keys with both kinds; a quarter of the names are wildcard
        # strings, so wildcard keys alone answer an eighth)
        assert 0.1 < (exp != NONE).mean() < 0.6
        nb, no = P.pack(list(names), np.uint32)
        got = eng.match_packed(nb, no).exact_id
        for i in np.flatnonzero(got != exp):
            raise AssertionError((tail, int(i), names[i][:60].hex(), int(got[i]), int(exp[i])))
        for shift in (0, 3):  # (the owned probe reads global memory: another dword residue)
            db, do = _on_device(nb, no, shift)
            for parts in (1, 2, 3):
                own = eng.key_owners(nb, no.astype(np.uint64), parts)
                plain = np.array([not nm.startswith(b"+/") for nm in names])
                for part in range(parts):
                    out = torch.full((len(names),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    eng.exact_owned_device(db.data_ptr() + shift, do.data_ptr(), len(names), parts,
                                           part, out.data_ptr())
                    g = out.cpu().numpy().view(np.uint32)
                    e = np.where((own == part) & plain, exp, NONE).astype(np.uint32)
                    for i in np.flatnonzero(g != e):
                        raise AssertionError((tail, shift, parts, part, int(i),
                                              names[i][:60].hex(), int(g[i]), int(e[i])))
    eng.close()
