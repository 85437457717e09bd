"""The case tables of the admission pass (k_admit, emqx_amd/csrc/gm_admit.inc), shared by the CPU
gate (tests/test_admit_dev_host.py: the kernel's phases under ASan + UBSan) and the device
(tests/test_gpu_admit.py).  A batch is one emqxgm_admit_batch call:

    dict(mode, items, flags (or None), zones (or None), caps (list of zones), base, pass_items)

and its expected records are tests/admit_ref.py's, word for word.  The sizes are the smallest at
which the kernel can go wrong: tile edges (256 items), the 16 alignments of a 16-B chunk, the 8
alignments of a scan word, items around 65535 bytes (which also force the global path of their
tile), one item per class of malformed UTF-8, every parse corner and every caps clause."""
import random

import admit_ref as R

NAME, FILTER = R.NAME, R.FILTER
E_ACUTE, EURO, GRIN = "é".encode(), "€".encode(), "\U0001F600".encode()  # 2, 3, 4 bytes


def batch(mode, items, flags=None, zones=None, caps=None, base=0, pass_items=0):
    return dict(mode=mode, items=list(items), flags=flags, zones=zones, caps=caps or [R.caps()], base=base,
                pass_items=pass_items)


def expected(b):
    out = []
    for i, item in enumerate(b["items"]):
        fl = b["flags"][i] if b["flags"] is not None else 0
        zn = b["zones"][i] if b["zones"] is not None else 0
        out.append(R.record(b["mode"], item, fl, b["caps"][zn]))
    return out


def both_modes(items, **kw):
    return [batch(NAME, items, **kw), batch(FILTER, items, **kw)]


# ---- the seeded sweep ----
PIECES = [b"a", b"/", b"+", b"#", b"$", b"\0", b"$share/", b"$exclusive/", E_ACUTE, EURO, GRIN,
          E_ACUTE[:1], EURO[:1], EURO[:2], GRIN[:1], GRIN[:2], GRIN[:3]]
WEIGHTS = [10, 8, 2, 2, 1, 1, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1]
SWEEP_CAPS = [R.caps(),
              R.caps(max_topic_levels=2, max_qos_allowed=1, retain_available=False, wildcard_subscription=False,
                     shared_subscription=False),
              R.caps(max_topic_levels=0, max_qos_allowed=0, wildcard_subscription=False, shared_subscription=False,
                     exclusive_subscription=True),
              R.caps(max_topic_levels=0, retain_available=False, shared_subscription=False)]


def sweep_items(n=4096, seed=20240607):
    rng = random.Random(seed)
    items = []
    while len(items) < n:
        k = rng.choice((0, 0, 1, 1, 2, 3, 4, 5, 6, 8, 10, 14))
        it = b"".join(rng.choices(PIECES, WEIGHTS, k=k))
        if len(it) <= 40:
            items.append(it)
    return items


def sweep(n=4096, seed=20240607):
    """The same items as names and as filters, random flags, four zones."""
    rng = random.Random(seed + 1)
    items = sweep_items(n, seed)
    flags = [rng.randrange(3) | (R.IN_RETAIN if rng.random() < 0.3 else 0) | (R.IN_HAS_SHARE if rng.random() < 0.15 else 0)
             for _ in items]
    zones = [rng.randrange(len(SWEEP_CAPS)) for _ in items]
    return [batch(m, items, flags, zones, SWEEP_CAPS) for m in (NAME, FILTER)]


# ---- tile edges ----
BATCH_SIZES = (0, 1, 255, 256, 257, 513)


def sizes():
    items = sweep_items(513, seed=7)
    return [b for n in BATCH_SIZES for b in both_modes(items[:n])] + [
        # the same 513 items in passes of 100: pass edges inside tiles
        batch(FILTER, items, pass_items=100)]


# ---- alignments ----
ALIGN_ITEMS = [b"a/b", b"$share/g/t/" + EURO, b"", b"x" + GRIN + b"/#", b"sensor/" + E_ACUTE * 5 + b"/+/v",
               b"#", b"0123456789abcdef/" + EURO[:2], b"+/+/#", b"$exclusive/t", b"a" * 17 + b"#"]


def alignments():
    return [b for base in range(16) for b in both_modes(ALIGN_ITEMS, base=base)]


# ---- item lengths ----
def lengths():
    out = []
    for n in (0, 1, 65535, 65536, 65537):
        long_items = [b"a" * n, (b"a/" * n)[:n], (b"b" * (n - 1) + b"#") if n else b"",
                      (b"$share/g/" + b"c" * n)[:n], (b"$share/g+/" + b"c" * n)[:n],
                      (b"$exclusive/" + EURO * n)[:n - 1] + b"d" if n > 1 else b"e" * n]
        for it in long_items:
            assert len(it) == n
            # small neighbours in the same tile: they take the tile's path
            out += both_modes([b"x/y", it, b"$share/g/t", EURO + b"#", b""])
    return out


# ---- UTF-8 ----
def straddles():
    """A 4-, 3- and 2-byte sequence across a scan-word boundary (8 bytes from the item's start),
    every split, with the batch at each of the 8 byte alignments; the items in front move the
    later ones through the alignments too."""
    items = []
    for seq in (GRIN, EURO, E_ACUTE):
        for word in (1, 2):
            for j in range(1, len(seq)):
                pre = b"x" * (8 * word - j)
                items += [pre + seq + b"y", pre + seq, pre + seq + b"#", pre + seq[:-1] + b"/z", b"/" + pre[1:] + seq]
    return [b for base in range(8) for b in both_modes(items, base=base)]


MALFORMED = {
    "overlong C0": b"\xc0\x80", "overlong C1": b"\xc1\xbf", "overlong E0 80": b"\xe0\x80\x80",
    "overlong E0 9F": b"\xe0\x9f\xbf", "overlong F0 80": b"\xf0\x80\x80\x80", "overlong F0 8F": b"\xf0\x8f\xbf\xbf",
    "surrogate ED A0": b"\xed\xa0\x80", "surrogate ED BF": b"\xed\xbf\xbf", "above F4 90": b"\xf4\x90\x80\x80",
    "above F5": b"\xf5\x80\x80\x80", "above FF": b"\xff", "lone 80": b"\x80", "lone BF": b"\xbf",
    "truncated 2": E_ACUTE[:1], "truncated 3": EURO[:2], "truncated 4": GRIN[:3], "truncated 4 at 1": GRIN[:1],
    "truncated then ascii": EURO[:2] + b"a", "bad second of four": b"\xf0\x9f\x2b\x80",
}


def malformed():
    items = []
    for m in MALFORMED.values():
        items += [m, b"#" + m, m + b"#", b"ab" + m + b"cd#", b"#/" + m, m + b"/#", b"a/#/" + m, m + b"/#/b",
                  b"+" + m, m + b"\0", b"topic/" + m + b"/x", b"abcdefg" + m, b"abcdefgh" + m, b"$share/g/" + m,
                  b"$share/" + m + b"/t"]
    # '/' inside a sequence: the left word keeps a truncated one
    items += [EURO[:2] + b"/" + EURO[2:], GRIN[:2] + b"/" + GRIN[2:], E_ACUTE[:1] + b"/" + E_ACUTE[1:], b"a/" + EURO[:1] + b"/b"]
    # accepted: the edges of the ranges
    items += [chr(c).encode("utf-8", "surrogatepass") for c in (0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFE, 0xFFFF,
                                                                0x10000, 0x10FFFF)]
    items += [b"a/" + chr(0xD7FF).encode() + chr(0xE000).encode() + b"/" + chr(0x10FFFF).encode() + chr(0xFFFF).encode()]
    # '#' not last followed by a malformed word: 'topic_invalid_#' wins
    items += [b"#/\xff", b"a/#/\xc0\x80/b", b"\xff/#/a"]
    return both_modes(items)


# ---- parse ----
PARSE_ITEMS = [b"$share/g/$share/h/t", b"$share/g/$exclusive/t", b"$exclusive/$share/g/t", b"$share//t", b"$share/g/",
               b"$share/t", b"$share/+/t", b"$share/a#/t", b"$exclusive/", b"$share/g/t", b"$shared/x",
               b"$local/$share/g/a", b"$share/", b"$share", b"$exclusive", b"$exclusive/t", b"$exclusive/t/#",
               b"$share/g/$exclusive/", b"$share/g/+/#", b"$share/group-name-longer-than-a-word/t/u",
               b"$share/1234567/t", b"$share/12345678/t", b"$share/123456789/t", b"$share/g#", b"$share/g/#/x",
               b"$share/g/$exclusive/$share/h/t", b"$exclusive/$exclusive/t", b"t", b"", b"$share/" + EURO + b"/t",
               b"$share/\xff/t", b"$SHARE/g/t", b"$share/g\0/t", b"$queue/t"]


def parses():
    none = batch(FILTER, PARSE_ITEMS)
    has = batch(FILTER, PARSE_ITEMS, flags=[R.IN_HAS_SHARE] * len(PARSE_ITEMS))
    excl = batch(FILTER, PARSE_ITEMS, caps=[R.caps(exclusive_subscription=True)])
    return [none, has, excl, batch(NAME, PARSE_ITEMS, flags=[R.IN_HAS_SHARE] * len(PARSE_ITEMS))]


# ---- caps ----
def caps_cases():
    out = []
    # NAME: levels, qos, retain -- each alone, each adjacent pair (the earlier clause wins), all
    names = [b"a/b/c", b"a", b"a/b", b"a/b/c/d"]
    for lv in (0, 1, 2, 3, 4, 65535):
        for mq in (0, 1, 2):
            for ra in (False, True):
                c = [R.caps(max_topic_levels=lv, max_qos_allowed=mq, retain_available=ra)]
                items, flags = [], []
                for nm in names:
                    for q in (0, 1, 2):
                        for rt in (0, R.IN_RETAIN):
                            items.append(nm)
                            flags.append(q | rt)
                out.append(batch(NAME, items, flags, caps=c))
    # FILTER: levels, wildcard, shared, exclusive
    filters = [b"a/b/c", b"a/+/c", b"$share/g/a/b/c", b"$share/g/a/#", b"$exclusive/a/b/c", b"$exclusive/+/b/c",
               b"$share/g/$exclusive/a/b/c", b"$share/g/$exclusive/a/b/#", b"a", b"a/b/c/d", b"$share/g/a/b/c/d"]
    for lv in (0, 2, 3, 4):
        for bits in range(16):
            c = [R.caps(max_topic_levels=lv, wildcard_subscription=bool(bits & 1), shared_subscription=bool(bits & 2),
                        exclusive_subscription=bool(bits & 4), max_qos_allowed=2 if bits & 8 else 0)]
            out.append(batch(FILTER, filters, caps=c))
            out.append(batch(FILTER, filters, flags=[R.IN_HAS_SHARE | 2] * len(filters), caps=c))
    # two zones (and the last of 256) in one batch
    table = [R.caps()] * 256
    table[1] = R.caps(max_topic_levels=1, wildcard_subscription=False)
    table[255] = R.caps(max_qos_allowed=0, retain_available=False, shared_subscription=False)
    items = [b"a/b", b"a/b", b"a/b", b"+", b"+", b"+", b"$share/g/t", b"$share/g/t", b"$share/g/t"]
    zones = [0, 1, 255] * 3
    flags = [1 | R.IN_RETAIN] * 9
    out += [batch(NAME, items, flags, zones, table), batch(FILTER, items, flags, zones, table)]
    return out


TABLES = {"sizes": sizes, "alignments": alignments, "lengths": lengths, "straddles": straddles,
          "malformed": malformed, "parses": parses, "caps": caps_cases, "sweep": sweep}


def check_table(run, name, force_global):
    """run(batch, force_global) -> [(w0, levels, off, share_len)]; compared with admit_ref's."""
    n = 0
    for k, b in enumerate(TABLES[name]()):
        got, want = run(b, force_global), expected(b)
        assert len(got) == len(want), (name, k, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            assert tuple(g) == tuple(w), (name, k, i, b["mode"], b["items"][i][:64], b["flags"] and b["flags"][i],
                                          [hex(x) for x in g], [hex(x) for x in w])
        n += len(want)
    return n
