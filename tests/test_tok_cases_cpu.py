"""tests/tok_cases.py judged on its inputs and on the oracle alone: the coverage it claims is
there, every case topic matches its own filter and none of its near misses, the pairs that match
are few but not none, and the Python restatements of word_token / key_hash give the values worked
out from gm_common.h."""
import postwalk_cases as P
import tok_cases as T
from oracle import emqx_ref as R


def test_tokeniser_families_cover_what_they_claim():
    topics, info = T.main_batch()  # (asserts every (length, level, residue) and byte position)
    fams = [i["fam"] for i in info if i]
    assert fams.count("W") == len(T.W_LENS) * 9 * 16 and fams.count("Wd") == len(T.W_LENS) * 8
    assert fams.count("B") == len(T.B_BYTES) * len(T.B_LENS) * 2 * 4
    assert fams.count("N") == 11 * 5 * 4
    # every byte value sits at every dword position, before and after a '/'
    off, seen = 0, set()
    for t, i in zip(topics, info):
        if i and i["fam"] == "B":
            for at in range(len(t)):
                if t[at] in T.B_BYTES and at and at + 1 < len(t):
                    if t[at + 1] == 0x2F:
                        seen.add((t[at], (off + at) % 4, "before"))
                    if t[at - 1] == 0x2F:
                        seen.add((t[at], (off + at) % 4, "after"))
        off += len(t)
    assert seen >= {(v, p, s) for v in T.B_BYTES for p in range(4) for s in ("before", "after")}
    # the record / token-array boundary: topics of 6..9 levels and one more (a trailing empty one)
    assert {len(t.split(b"/")) for t, i in zip(topics, info) if i and i["fam"] == "Wd"} == \
        {6, 7, 8, 9, 10}


def test_tiles_sit_where_intended():
    topics, info, spec = T.tile_batch(0)
    tl = T.tiles_of(topics)
    got = {(sh, sh + nb): fit for (sh, nb, fit), s in zip(tl, spec) if s}
    assert got == {(sh, tot): tot <= T.TILE_FIT for sh in T.T_SH for tot in T.T_TOTALS}
    assert T.fits(0, 16400) and not T.fits(0, 16401) and T.fits(15, 16385) and not T.fits(15, 16386)
    for r in range(4):
        tp, inf, sp = T.tile_batch(r, r == 0)
        assert len(tp) % T.WG == T.RAGGED and tp[-1].endswith(T._end(T.ENDINGS[r])) and inf[-1]
        assert any(s and s[1] > T.TILE_FIT for s in sp)  # a non-fitting tile before the ragged one
    # both kinds of tile end in every ending
    for fit in (True, False):
        assert {s[2] for s in spec if s and (s[1] <= T.TILE_FIT) == fit} == set(T.ENDINGS)
    n_topics = sum(len(t) for t, _ in T.tok_batches().values())
    assert n_topics <= 12500 and len(T.tok_filters()) <= 8000


def test_probe_family_covers_what_it_claims():
    for tail in range(4):
        names, keys = T.probe_batch(tail)  # (asserts lengths x residues, pairs, the share)
        ks = set(keys)
        share = sum(nm in ks for nm in names) / len(names)
        assert 0.40 <= share <= 0.60
        assert len(names[-1]) % 4 == tail and names[-1] in ks and len(names) <= 3000
    names, keys = T.probe_batch(0)
    ks, off, seen = set(keys), 0, set()
    for nm in names:
        seen.add((nm.startswith(b"+/"), len(nm) - 2 * nm.startswith(b"+/"), off % 16, nm in ks))
        off += len(nm)
    for wild in (False, True):
        for L in T.K_LENS:
            for r in T.K_RES:
                assert (wild, L, r, True) in seen
                assert not L or (wild, L, r, False) in seen
    assert {len(k) for k in keys} >= set(range(2, 46))
    for kinds, n in (("plain", False), ("wild", True)):
        assert all(k.startswith(b"+/") == n for k in T.probe_keys((names, keys), kinds))


def test_set_is_not_vacuous_on_the_oracle():
    """Each case topic matches its own T/# and no near miss or mutant.  Every case topic matches
    its own filter alone, so of the (topic, filter) pairs of all batches about one in 23,000
    matches (2,676 of 11,064 x 5,478 when this was written); the bounds leave a factor of two."""
    fs = T.tok_filters()
    pairs = cases = topics_n = near = 0
    for name, (topics, info) in T.tok_batches().items():
        rows = T.expected_rows(name)
        for t, i, row in zip(topics, info, rows):
            if i:
                assert i["own"] in row, (name, t[:60].hex())
                assert R.match(t, i["own"])
                for f in i["not"]:
                    assert f not in row and not R.match(t, f), (name, t[:60].hex(), f[:60].hex())
                near += i["fam"] == "N"
                cases += 1
            pairs += len(row)
        topics_n += len(topics)
    assert near == 220 and cases >= 2500
    assert pairs >= cases  # (a filler or an unfiltered tile topic matches nothing)
    share = pairs / (topics_n * len(fs))
    assert 2e-5 <= share <= 2e-4, (pairs, topics_n, len(fs))


def test_word_token_and_key_hash_literals():
    """Worked out from gm_common.h: short words are their bytes little-endian under the length in
    bits 56..62; FNV-1a("foobar") and fmix64(1) are the published vectors of the two functions the
    hashed token is made of; the hashed tokens and key hashes are the header's own arithmetic
    carried out outside this module."""
    assert P.word_token(b"") == 0
    assert P.word_token(b"abc") == 0x0300000000636261
    assert P.word_token(b"abcdefg") == 0x0767666564636261
    assert P.word_token(b"\xff") == 0x01000000000000ff
    assert P.word_token(b"a\x00") == 0x0200000000000061 and P.word_token(b"a") == 0x0100000000000061
    assert P._fmix64(1) == 0xb456bcfc34c2cb2c
    assert P.word_token(b"abcdefgh") == 0xcdbe4ec528ba88e4
    assert P.word_token(b"abcdefghi") == 0xabb2cae281de7af4
    assert P.word_token(b"seventeen-bytes-w") == 0xf023b7a7e74dc959
    assert all(P.word_token(w) >> 63 == (len(w) > T.TOK_INLINE_MAX)
               for w in (b"", b"1234567", b"12345678"))
    assert P.key_hash(b"") == 0x267e489e3b754e2b
    assert P.key_hash(b"a") == 0x906849801f85960a
    assert P.key_hash(b"abcd") == 0xc0c1caa1d169b683
    assert P.key_hash(b"abcde") == 0xd74a8cafa86726d5
    assert P.key_hash(b"sensor/+/metric/12345") == 0x21f794bde3bb959d
    assert P.key_hash(b"abcde", 2) == 1 and P.key_hash(b"a", 2) == 2
