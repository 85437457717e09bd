"""The checks that the CPU gate (tests/test_acldb_dev_host.py) and the GPU tests
(tests/test_gpu_acldb.py) of the built-in database share: each plays a script of
tests/acldb_cases.py through ``play(script)``, which returns per query (answers, stats, count), and
compares with the script's reference answers.  A helper, not a test."""
import acldb_cases as DC


def check_keys(play, hash_bits):
    s = DC.case("keys", hash_bits)
    st = DC.check(s, play(s))[0]
    assert st["clientid_records"] == st["username_records"] == len(DC.KEYS) and st["all_rules"] == 3
    # keys of 8, 9 and 40 bytes and ${clientid} have hashed tokens: hits are confirmed on the bytes
    assert st["key_checked"] >= 1 and st["candidates"] > st["removed"]
    if hash_bits:
        assert st["key_removed"] >= 1, st  # 11 keys on 16 tokens


def check_order(play, hash_bits):
    s = DC.case("order", hash_bits)
    st = DC.check(s, play(s))[0]
    assert st["clientid_records"] == 2  # the empty record counts


def check_random(play, hash_bits):
    s = DC.case("random", hash_bits)
    st = DC.check(s, play(s))[0]
    assert st["deep"] == 2  # the 40- and the 17-level name
    assert st["rebuilds"] == 0 and st["garbage_words"] == 0


def check_depth(play, hash_bits):
    s = DC.case("depth", hash_bits)
    st = DC.check(s, play(s))[0]
    deep = sum(1 for _, _, n in s.queries()[0][1] if len(n.split(b"/")) > 16)
    assert st["deep"] == deep > 0


def check_runs(play, hash_bits):
    s = DC.case("runs", hash_bits)
    st = DC.check(s, play(s))[0]
    assert st["all_tiles"] == 0 and st["live_words"] > 5 * DC.MAX_RULES


def check_tiling(play, hash_bits):
    s = DC.case("tiling", hash_bits)
    st = DC.check(s, play(s))[0]
    assert st["all_tiles"] == 3 and st["all_rules"] == 105


def check_empty_all(play):
    s = DC.case("empty_all")
    st = DC.check(s, play(s))[0]
    assert st["all_tiles"] == 0 and s.queries()[0][3] == 2


def check_all_edits(play):
    s = DC.case("all_edits")
    st = DC.check(s, play(s))
    # every stream is 11 words: garbage never passes the live words by more than one stream, and
    # rebuilds take it away, so the filter pools do not grow with the number of edits
    assert all(q["live_words"] == 11 and q["garbage_words"] <= 11 for q in st), st
    assert st[-1]["rebuilds"] >= 5 and st[-1]["all_rules"] == 2


def check_shapes(play, hash_bits):
    s = DC.case("shapes", hash_bits)
    ks = DC.chain_keys(hash_bits)
    h = DC.home(ks[0], hash_bits, DC.MIN_SLOTS)
    assert all(DC.home(k, hash_bits, DC.MIN_SLOTS) == h for k in ks) and h + 4 > DC.MIN_SLOTS  # the chain wraps
    st = DC.check(s, play(s))
    for q in st:
        assert q["clientid_slots"] == q["username_slots"] == DC.MIN_SLOTS and q["rebuilds"] == 0, q
        assert q["max_chain"] == 4, q
    assert st[0]["clientid_records"] == 4 and st[0]["clientid_deleted"] == 0
    assert st[1]["clientid_records"] == 3 and st[1]["clientid_deleted"] == st[1]["username_deleted"] == 1
    assert st[2]["clientid_records"] == 4 and st[2]["clientid_deleted"] == 0 and st[2]["username_deleted"] == 1
    if hash_bits:
        # one token for the four keys: every hit but the right one is removed by the byte check
        assert st[0]["key_removed"] >= 1 and st[2]["key_removed"] > st[1]["key_removed"], st


def check_block(play, n):
    s = DC.case("block", 0, n)
    assert len(s.queries()[0][1]) == n
    DC.check(s, play(s))


def check_passes(play):
    s1, s = DC.case("random", 0), DC.case("passes")
    assert -(-len(s.queries()[0][1]) // DC.PASS_NAMES) == 14
    r1, r = play(s1), play(s)
    DC.check(s, r)
    assert r[0] == r1[0]  # answers and counters: each request is counted in one pass


def check_update(play, hash_bits, exact_alloc):
    s = DC.case("update", hash_bits)
    res = play(s)
    st = DC.check(s, res)
    assert st[4]["garbage_words"] > 0 and st[4]["rebuilds"] == 0     # the replaced runs and `all` stream
    assert st[6]["clientid_slots"] > DC.MIN_SLOTS and st[6]["username_slots"] > DC.MIN_SLOTS  # both rehashed
    assert st[6]["rebuilds"] >= 2
    # one commit in which the record pool, the filter bytes and offsets and the key bytes and
    # offsets each outgrow their allocation (a new one and a device-to-device copy), no rebuild
    assert st[8]["growths"] == st[7]["growths"] + 5 and st[8]["rebuilds"] == st[7]["rebuilds"], (st[7], st[8])
    assert st[8]["clientid_slots"] == st[7]["clientid_slots"] and st[8]["clientid_records"] == 64
    assert st[8]["garbage_words"] > 0
    # the forced rebuild: garbage gone, the live words as before, every answer as before
    assert st[9]["rebuilds"] == st[8]["rebuilds"] + 1 and st[9]["garbage_words"] == 0
    assert st[9]["live_words"] == st[8]["live_words"] and res[9][0] == res[8][0]
    assert st[11]["clientid_records"] == 0 and st[11]["username_records"] == 1 and st[11]["live_words"] == 6
    if not exact_alloc:
        # with growth slack a commit of one small record does not grow a pool
        assert st[4]["growths"] == st[2]["growths"]
