"""The inputs that the ACL device path is checked on, shared by the header-only program
(tests/test_acl_cpu.py), its CPU gate (tests/test_acl_dev_host.py: the kernel's phases and the
host code under ASan + UBSan) and its GPU tests (tests/test_gpu_acl.py), so that all see exactly
the same cases.  Built on tests/acl_ref.py; expected answers are computed once per process and are
read only.  A helper, not a test.

A case is ``(rules, clients, requests)``: source rules (acl_ref.compile's input), clients as
dicts of clientid / username (bytes or None = undefined) / peerhost (an address tuple or None),
requests as ``(client index, "publish" | "subscribe", name)``.
"""
import functools
import random

import acl_ref as AR
import ruleset_ref as RR

RS_MAX_LEVELS = 16    # emqx_amd/csrc/gm_ruleset_match.h
RS_TILE_WORDS = 1024
ACL_RULE_WORDS = 2    # emqx_amd/csrc/gm_acl_match.h
ACL_FILTER_HDR = 2
HOST_SLOTS = 64
PERM = {"deny": 0, "allow": 1}
ACTION = {"publish": 1, "subscribe": 2, "all": 3}
WHO_ALL, WHO_USERNAME, WHO_CLIENTID, WHO_HOST = 0, 1, 2, 3
NO_CLIENTID, NO_USERNAME = 1, 2
EQ = 1  # EMQXGM_RULE_EQ
BATCH_SIZES = (0, 1, 255, 256, 257, 513)
LIST_SIZES = (63, 64, 65, 130)
PASS_NAMES = 300

PHC, PHU = AR.PH_CLIENTID, AR.PH_USERNAME
ID40A = b"client-id-of-forty-bytes-0123456789abcd1"
ID40B = b"client-id-of-forty-bytes-0123456789abcd2"
assert len(ID40A) == len(ID40B) == 40 and ID40A[:-1] == ID40B[:-1]
# ids and usernames of 1, 7, 8, 9 and 40 bytes, then the values that equal no name word or look
# like something else
VALUES = [b"a", b"sevenby", b"eightbyt", b"ninebytes", ID40A, ID40B, b"", b"+", b"#", b"a/b", PHC, b"$s"]
PEERS = [(127, 0, 0, 1), (192, 168, 1, 10), (10, 0, 0, 5), None]


def client_table():
    """Every value as a client id and as a username, then undefined id, undefined username, both."""
    cs = [{"clientid": v, "username": VALUES[(i + 3) % len(VALUES)], "peerhost": PEERS[i % 4]}
          for i, v in enumerate(VALUES)]
    cs += [{"clientid": None, "username": b"a", "peerhost": PEERS[0]},
           {"clientid": b"sevenby", "username": None, "peerhost": PEERS[1]},
           {"clientid": None, "username": None, "peerhost": None}]
    return cs


CLIENTS = client_table()
# words of the names: the rule-set vocabulary, every client value (a/b as the bytes "a/b": two
# words) and the placeholders themselves
NAME_WORDS = RR.VOCAB + [v for v in VALUES if v not in RR.VOCAB] + [PHU]
HOST_POOL = [("ipaddr", "127.0.0.1"), ("ipaddrs", ["10.0.0.0/8", "192.168.1.0/24"]),
             ("username", ("re", "^se")), ("clientid", ("re", "byt")),
             ("and", [("client", "a"), ("user", "ninebytes")]),
             ("or", [("user", "eightbyt"), ("ipaddr", "10.0.0.5")])]


# ---- the C-ABI's view of a list ----------------------------------------------------------

def _key(w):
    if isinstance(w, tuple):
        return tuple(_key(x) for x in w)
    if isinstance(w, list):
        return ("list",) + tuple(_key(x) for x in w)
    return getattr(w, "pattern", w)


def join(ws) -> bytes:
    return b"/".join(w.encode() if isinstance(w, str) else w for w in ws)


def flatten(compiled):
    """emqxgm_acl_set's arguments for a compiled list, and the compiled principal of each host
    slot: (filters, flags, filter_rule, perm, action, who, slot, who_strings, slot_exprs).
    ValueError when the list has more than 64 distinct host principals."""
    filters, flags, owner, perm, action, who, slot, strings, exprs, slot_of = [], [], [], [], [], [], [], [], [], {}
    for r, (p, w, a, fs) in enumerate(compiled):
        kind, s, string = WHO_ALL, 0, b""
        if w != "all" and w[0] in ("username", "clientid") and w[1][0] == "eq":
            kind, string = (WHO_USERNAME if w[0] == "username" else WHO_CLIENTID), w[1][1]
        elif w != "all":
            if _key(w) not in slot_of:
                if len(exprs) == HOST_SLOTS:
                    raise ValueError("more than 64 host principals")
                slot_of[_key(w)] = len(exprs)
                exprs.append(w)
            kind, s = WHO_HOST, slot_of[_key(w)]
        perm.append(PERM[p])
        action.append(ACTION[a])
        who.append(kind)
        slot.append(s)
        strings.append(string)
        for f in fs:
            eq = isinstance(f, tuple) and f[0] == "eq"
            filters.append(join(f[1] if isinstance(f, tuple) else f))
            flags.append(EQ if eq else 0)
            owner.append(r)
    return filters, flags, owner, perm, action, who, slot, strings, exprs


def table_args(clients, exprs):
    """emqxgm_acl_match's client table: (clientids, usernames, flags, who_bits); None = undefined."""
    ids = [c["clientid"] for c in clients]
    users = [c["username"] for c in clients]
    flags = [(NO_CLIENTID if c["clientid"] is None else 0) | (NO_USERNAME if c["username"] is None else 0)
             for c in clients]
    bits = [sum(1 << k for k, w in enumerate(exprs) if AR.match_who(c, w)) for c in clients]
    return ids, users, flags, bits


def first_rule(client, pubsub, topic, compiled):
    """Index of the rule that decides matches/4, or None."""
    for r, rule in enumerate(compiled):
        if AR.match(client, pubsub, topic, rule) != "nomatch":
            return r
    return None


def answers(case):
    """(compiled rules, first rule per request, matches/4 per request)."""
    rules, clients, reqs = case
    compiled = [AR.compile(r) for r in rules]
    first = [first_rule(clients[c], p, t, compiled) for c, p, t in reqs]
    res = ["nomatch" if r is None else ("matched", compiled[r][0]) for r in first]
    return compiled, first, res


# ---- tokens (gm_common.h word_token in the collision-test mode) and the unconfirmed model -----

M64 = (1 << 64) - 1


def fmix64(k):
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & M64
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & M64
    return k ^ (k >> 33)


def hash_token(w: bytes, bits: int) -> int:
    h = 0xcbf29ce484222325
    for c in w:
        h = (h ^ c) * 0x100000001b3 & M64
    return fmix64(h) & ((1 << bits) - 1)


class Tok:
    """A word known by its masked hash only.  Against an atom ("+", "#", "") it compares by its
    bytes: which words of a name are "#" is known exactly on the device (hash_words)."""

    def __init__(self, b, bits):
        self.b, self.h = bytes(b), hash_token(bytes(b), bits)

    def __eq__(self, o):
        return self.h == o.h if isinstance(o, Tok) else (isinstance(o, str) and self.b == o.encode())

    __hash__ = None


def unconfirmed_first(client, pubsub, topic, compiled, bits=4):
    """first_rule with every word compare done on word_hash_bits = bits tokens and nothing
    confirmed on the bytes (names of more than RS_MAX_LEVELS levels are always matched on the
    bytes, so they keep their answer)."""
    if len(topic.split(b"/")) > RS_MAX_LEVELS:
        return first_rule(client, pubsub, topic, compiled)
    name = [Tok(w, bits) for w in topic.split(b"/")]

    def fed(v, ph):
        if v is None:
            return Tok(ph, bits)
        return Tok(v, bits) if v not in (b"", b"+", b"#") and b"/" not in v else object()

    for r, (perm, who, action, fs) in enumerate(compiled):
        if not AR.match_action(pubsub, action):
            continue
        if who != "all" and who[0] in ("username", "clientid") and who[1][0] == "eq":
            v = client[who[0]]
            if v is None or hash_token(v, bits) != hash_token(who[1][1], bits):
                continue
        elif not AR.match_who(client, who):
            continue
        for f in fs:
            if isinstance(f, tuple) and f[0] == "eq":
                if len(f[1]) <= RS_MAX_LEVELS and name == [Tok(join([w]), bits) for w in f[1]]:
                    return r
                continue
            ws = f[1] if isinstance(f, tuple) else f
            if len(ws) - (ws[-1] == "#") > RS_MAX_LEVELS:
                continue
            g = []
            for i, w in enumerate(ws):
                if w == PHC:
                    g.append(fed(client["clientid"], PHC))
                elif w == PHU:
                    g.append(fed(client["username"], PHU))
                elif w == "+" or (w == "#" and i == len(ws) - 1):
                    g.append(w)
                else:
                    g.append(Tok(join([w]), bits))
            if AR.R.match(name, g):
                return r
    return None


# ---- random lists ------------------------------------------------------------------------

def _word(rng):
    return rng.choice(RR.VOCAB[:3]) if rng.random() < 0.6 else rng.choice(RR.VOCAB)


def rand_filter(rng):
    d = rng.randint(1, 5)
    ws = [_word(rng)]  # a literal first word: a name with a first word of its own matches nothing
    for i in range(1, d):
        r = rng.random()
        if i == d - 1 and r < 0.2:
            ws.append(b"#")
        elif r < 0.3:
            ws.append(b"+")
        elif r < 0.33:
            ws.append(b"#")  # also as a non-final word: a literal
        elif r < 0.5:
            ws.append(PHC if rng.random() < 0.6 else PHU)
        else:
            ws.append(_word(rng))
    f = b"/".join(ws)
    k = rng.random()
    if k < 0.1:
        return ("eq", f)
    return b"eq " + f if k < 0.15 else f


def rand_who(rng):
    k = rng.random()
    if k < 0.5:
        return "all"
    if k < 0.65:
        return (rng.choice(["username", "user"]), rng.choice(VALUES))
    if k < 0.8:
        return (rng.choice(["clientid", "client"]), rng.choice(VALUES))
    return rng.choice(HOST_POOL)


def rand_name(rng) -> bytes:
    ws = [_word(rng) if rng.random() < 0.7 else rng.choice(NAME_WORDS) for _ in range(rng.randint(1, 5))]
    if rng.random() < 0.15:
        ws[0] = b"zz"  # a first word no filter has
    return b"/".join(ws)


# the first rules of a list decide most requests; these seeds give every outcome (allow, deny,
# nomatch) a tenth of the requests or more, which tests/test_acl_ref_cpu.py asserts
SEEDS = {63: 5063, 64: 2064, 65: 2065, 130: 2130}


def random_case(n_rules: int, n_requests: int = 4007):
    """n_rules rules of 0 to 4 filters with all three actions, both permissions and all who kinds
    against n_requests requests whose names end with the rule sets' edge names."""
    rng = random.Random(SEEDS[n_rules])
    rules = [("deny" if rng.random() < 0.6 else "allow", rand_who(rng), rng.choice(["publish", "subscribe", "all"]),
              [rand_filter(rng) for _ in range(rng.randint(0, 4))]) for _ in range(n_rules)]
    names = [rand_name(rng) for _ in range(n_requests - len(RR.EDGE_NAMES))] + RR.EDGE_NAMES
    reqs = [(rng.randrange(len(CLIENTS)), rng.choice(["publish", "subscribe"]), n) for n in names]
    return rules, CLIENTS, reqs


@functools.lru_cache(maxsize=None)
def random_reference(n_rules: int):
    case = random_case(n_rules)
    return (case,) + answers(case)


# ---- the client table: every value as a word of a name ---------------------------------------

def values_case():
    """Filters with each placeholder, alone and after a literal, against names that hold every
    client value as a word, for every client: a wrong atom rule ("+" as a wildcard, "" equal to
    the empty word, "a/b" spliced in as two words) gives a wrong answer."""
    rules = [("deny", "all", "subscribe", ["c/${clientid}", "${clientid}"]),
             ("allow", "all", "all", ["u/${username}/#", "${username}", ("eq", "${clientid}")]),
             ("deny", "all", "all", ["c/${clientid}/${username}", "eq c/${username}"])]
    names = []
    for v in VALUES + [PHU]:
        names += [v, b"c/" + v, b"u/" + v, b"u/" + v + b"/x", b"c/" + v + b"/" + v]
    names += [b"c/${username}", b"c/", b"u//x", b"c/a/b/ninebytes"]
    reqs = [(c, p, n) for c in range(len(CLIENTS)) for n in names for p in ("publish", "subscribe")]
    return rules, CLIENTS, reqs


# ---- first-match order -----------------------------------------------------------------------

def order_case():
    rules = [("deny", "all", "all", ["o/deny/#"]),                          # 0
             ("allow", "all", "all", ["o/#"]),                              # 1: later allow, both match
             ("deny", "all", "subscribe", ["p/#"]),                         # 2: action alone skips it
             ("allow", "all", "publish", ["p/#"]),                          # 3
             ("deny", ("clientid", "sevenby"), "all", ["w/#"]),             # 4: who alone skips it
             ("allow", "all", "all", ["w/#"]),                              # 5
             ("allow", "all", "all", ["s/first", "s/+/second"]),            # 6: the second filter matches
             ("deny", "all", "all", [])]                                    # 7: no filter, never
    names = [b"o/deny/x", b"o/x", b"p/x", b"w/x", b"s/first", b"s/x/second", b"s/x", b"nothing"]
    reqs = [(c, p, n) for c in (0, 1) for p in ("publish", "subscribe") for n in names]
    return rules, CLIENTS, reqs


# ---- who slots -------------------------------------------------------------------------------

def slots_rules(n: int):
    """n rules with n distinct host principals: rule k is for the peers of 10.0.k.0/24."""
    return [("allow" if k % 2 else "deny", ("ipaddr", "10.0.%d.0/24" % k), "all", ["#"]) for k in range(n)]


def slots_case():
    clients = [{"clientid": b"c%d" % k, "username": None, "peerhost": (10, 0, k, 7)} for k in (0, 31, 32, 63, 64)]
    reqs = [(c, "publish", b"t/x") for c in range(len(clients))]
    return slots_rules(64), clients, reqs


# ---- tiling ----------------------------------------------------------------------------------

def record_words(f) -> int:
    """Words of a compiled filter's record (acl_compile_filter): ACL_FILTER_HDR + one per level,
    a final '#' takes none, more than RS_MAX_LEVELS levels: the two header words alone."""
    eq = isinstance(f, tuple) and f[0] == "eq"
    ws = f[1] if isinstance(f, tuple) else f
    n = len(ws) - (1 if not eq and ws[-1] == "#" else 0)
    return ACL_FILTER_HDR if n > RS_MAX_LEVELS else ACL_FILTER_HDR + n


def layout(compiled):
    """([(rule, filter in rule or None for the rule header, tile, word in tile, words)], total
    words of the stream) as rs_append lays the records out: none straddles a tile."""
    at, pos = 0, []

    def put(r, k, w):
        nonlocal at
        if at % RS_TILE_WORDS and at % RS_TILE_WORDS + w > RS_TILE_WORDS:
            at += RS_TILE_WORDS - at % RS_TILE_WORDS
        pos.append((r, k, at // RS_TILE_WORDS, at % RS_TILE_WORDS, w))
        at += w

    for r, rule in enumerate(compiled):
        put(r, None, ACL_RULE_WORDS)
        for k, f in enumerate(rule[3]):
            put(r, k, record_words(f))
    return pos, at


def tiles_of(total_words: int) -> int:
    return (total_words + RS_TILE_WORDS - 1) // RS_TILE_WORDS


def tiling_case():
    """Rules of one 16-level filter take 20 words.  51 of them (1,020 words), then rule 51's
    header (1,022) whose first filter a/# (3 words) opens tile 1; 50 more (tile 1 word 1,003),
    then rule 102: header, a 13-level filter (1,020), b/+ (4 words: the tile is full) and b/# at
    word 0 of tile 2; b/x matches both of them, b only the second.  Rule 103 is a later allow for
    everything, so every request is decided and the earlier rules have to win."""
    def fill(i):
        return ("deny", "all", "all", [b"/".join(b"f%d" % i for _ in range(16))])
    rules = [fill(i) for i in range(51)]
    rules.append(("deny", "all", "all", ["a/#"]))                                           # 51
    rules += [fill(i) for i in range(52, 102)]
    rules.append(("deny", ("clientid", ID40A), "all", [b"/".join([b"g"] * 13), "b/+", "b/#"]))  # 102
    rules.append(("allow", "all", "all", ["#"]))                                             # 103
    names = [b"a/b", b"a", b"b/x", b"b", b"b/x/y", b"/".join([b"f7"] * 16), b"/".join([b"f60"] * 16), b"x"]
    reqs = [(c, "publish", n) for c in (4, 5) for n in names]  # the two 40-byte ids
    return rules, CLIENTS, reqs


# ---- depth -----------------------------------------------------------------------------------

def depth_case():
    def lv(n, last=b"a"):
        return b"/".join([b"a"] * (n - 1) + [last])
    rules = [("deny", "all", "all", [lv(17, PHC)]),           # a pattern whose placeholder is level 17
             ("allow", "all", "publish", [lv(16), lv(17), lv(40)]),
             ("deny", "all", "subscribe", [("eq", lv(17, b"+")), lv(16, PHU), lv(17, b"#")]),
             ("allow", "all", "all", [lv(41, b"#")])]
    names = [lv(16), lv(17), lv(40), lv(15), lv(41), lv(17, b"+"), lv(42)]
    names += [lv(17, v) for v in VALUES if b"/" not in v] + [lv(16, v) for v in VALUES if b"/" not in v]
    names += [lv(17, PHC), lv(16, PHU), lv(16, b"a/b")]
    reqs = [(c, p, n) for c in range(len(CLIENTS)) for n in names for p in ("publish", "subscribe")]
    return rules, CLIENTS, reqs


# ---- sizes -----------------------------------------------------------------------------------

def block_case(n: int):
    """The last n requests (the edge names among them) of the 65-rule random case."""
    (rules, clients, reqs), compiled, first, res = random_reference(65)
    k = len(reqs) - n
    return (rules, clients, reqs[k:]), compiled, first[k:], res[k:]


EMPTY_LISTS = ([], [("allow", "all", "all", []), ("deny", ("user", "a"), "publish", []), ("deny", "all", "all", [])])


def one_client_case():
    rules = [("allow", ("clientid", "only"), "all", ["t/${clientid}"]), ("deny", "all")]
    clients = [{"clientid": b"only", "username": None, "peerhost": None}]
    reqs = [(0, "publish", b"t/only"), (0, "subscribe", b"t/other"), (0, "publish", b"")]
    return rules, clients, reqs


# ---- the built-in database -------------------------------------------------------------------

def builtin_db_case():
    """A few hundred records keyed by client id, by username and `all`, and requests of clients
    with and without records of their own."""
    rng = random.Random(31)
    ids = [b"dev-%03d" % i for i in range(150)] + [ID40A, ID40B, b"a"]
    users = [b"user-%03d" % i for i in range(100)] + [b"ninebytes", b"+"]

    def rs(tag):
        return [(rng.choice(["allow", "deny"]), rng.choice(["publish", "subscribe", "all"]),
                 rng.choice([b"d/${clientid}/#", b"u/${username}/+", b"eq d/" + tag, b"shared/#", b"d/+/state",
                             b"u/+/cmd/#"]))
                for _ in range(rng.randint(1, 3))]
    table = {}
    for c in ids:
        table[("clientid", c)] = rs(c)
    for u in users:
        table[("username", u)] = rs(u)
    table["all"] = [("deny", "subscribe", b"shared/secret"), ("allow", "all", b"shared/#"), ("deny", "all", b"#")]
    clients = [{"clientid": rng.choice(ids + [b"stranger", None]), "username": rng.choice(users + [b"nobody", None]),
                "peerhost": None} for _ in range(300)]
    reqs = []
    for c, cl in enumerate(clients):
        cid, usr = cl["clientid"] or b"x", cl["username"] or b"y"
        for n in (b"d/" + cid + b"/t", b"u/" + usr + b"/cmd", b"d/" + cid, b"shared/secret", b"shared/x",
                  b"d/" + cid + b"/state", b"u/" + usr + b"/cmd/go", b"other"):
            reqs.append((c, rng.choice(["publish", "subscribe"]), n))
    return table, clients, reqs


def builtin_db_records(table):
    """The table as from_builtin_db's records."""
    return [(k, v) for k, v in table.items()]


def builtin_db_rules(table):
    """The global source list: client-id-keyed rules, username-keyed ones, then `all`."""
    out = []
    for want in ("clientid", "username", "all"):
        for k, rs in table.items():
            kind = k if k == "all" else k[0]
            if kind == want:
                out += [(p, "all" if k == "all" else k, a, [t]) for p, a, t in rs]
    return out


# ---- every case the gate and the GPU test run through the C-ABI ------------------------------

@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(case, compiled, first rule per request, matches/4 per request) of a named case."""
    case = {"values": values_case, "order": order_case, "slots": slots_case, "tiling": tiling_case,
            "depth": depth_case, "one_client": one_client_case}[name]()
    return (case,) + answers(case)


# ---- the input file of the host programs (tests/host_harness/acl_input.h) and their output ----

STAT_KEYS = ("records", "tiles", "filters", "rules", "candidates", "removed", "deep", "visited")


def _hex(b) -> str:
    return (b or b"").hex() or "-"


def input_text(compiled, clients, reqs, hash_bits=0, pass_names=0) -> str:
    filters, flags, owner, perm, action, who, slot, strings, exprs = flatten(compiled)
    ids, users, cflags, bits = table_args(clients, exprs)
    lines = [f"{hash_bits} {pass_names}", str(len(compiled))]
    k = 0
    for r in range(len(compiled)):
        nf = owner.count(r)
        lines.append(f"{perm[r]} {action[r]} {who[r]} {slot[r]} {_hex(strings[r])} {nf}")
        lines += [f"{flags[k + j]} {_hex(filters[k + j])}" for j in range(nf)]
        k += nf
    lines.append(str(len(clients)))
    lines += [f"{cflags[c]} {_hex(ids[c])} {_hex(users[c])} {bits[c]}" for c in range(len(clients))]
    lines.append(str(len(reqs)))
    lines += [f"{c} {ACTION[p]} {_hex(n)}" for c, p, n in reqs]
    return "\n".join(lines) + "\n"


def parse_output(stdout: str, n: int):
    """(first rule per request or None, the STATS line as a dict)."""
    out = stdout.split("\n")
    assert out[-1] == "" and out[-2].startswith("STATS "), stdout[-500:]
    assert len(out) == n + 2, (len(out), n)
    rows = [None if line == "-" else int(line) for line in out[:n]]
    return rows, dict(zip(STAT_KEYS, map(int, out[-2].split()[1:])))
