"""The inputs that the built-in authorization database is checked on (DESIGN.md 6b "Built-in
database"), shared by the reference-only test (tests/test_acldb_ref_cpu.py), the CPU gate
(tests/test_acldb_dev_host.py: the kernel's phases and the host code under ASan + UBSan) and the
GPU tests (tests/test_gpu_acldb.py), so that all see exactly the same cases.  Built on
tests/acl_cases.py (its clients, values and name words) and tests/acl_ref.py; expected answers are
computed once per process and are read only.  A helper, not a test.

A case is a ``Script``: mutations of the database (store, store_many, delete, purge, commit, tune)
and queries.  The script keeps the reference table, a dict from ``("clientid", C)``,
``("username", U)`` or ``"all"`` to ``[(permission, action, topic filter)]`` as
``acl_ref.mnesia_authorize`` takes it, applies a mutation to it at the next commit, and records
with every query what the committed table answers: per request ``None`` or ``(permission, source,
position of the deciding rule in its record)``, and ``record_count/0`` with the pending mutations.
"""
import functools
import random

import acl_cases as AC
import acl_ref as AR
import ruleset_ref as RR

CLIENTID, USERNAME, ALL = 0, 1, 2  # EMQXGM_ACLDB_*
KIND = {"clientid": CLIENTID, "username": USERNAME}
MAX_RULES = 65536
MIN_SLOTS = 8                                # gm_acldb_match.h ADB_MIN_SLOTS
HOME_ADD = 0x2545f4914f6cdd1d                # adb_home
TOK_HASHED = 1 << 63
BATCH_SIZES = AC.BATCH_SIZES
PASS_NAMES = AC.PASS_NAMES
STAT_KEYS = ("clientid_records", "clientid_slots", "clientid_deleted", "username_records", "username_slots",
             "username_deleted", "max_chain", "all_rules", "live_words", "garbage_words", "rebuilds", "growths",
             "key_checked", "key_removed", "candidates", "removed", "deep", "all_tiles")

PHC, PHU = AC.PHC, AC.PHU
# keys of 0, 1, 7, 8, 9 and 40 bytes, the two 40-byte ids that differ in the last byte, and keys
# that look like something else
KEYS = [b"", b"a", b"sevenby", b"eightbyt", b"ninebytes", AC.ID40A, AC.ID40B, b"+", b"#", b"a/b", PHC]
assert [len(k) for k in KEYS[:6]] == [0, 1, 7, 8, 9, 40] and all(k in AC.VALUES for k in KEYS)


# ---- the reference -----------------------------------------------------------------------------

def decide(client, pubsub, topic, table):
    """(permission, source, position) of the rule that decides authorize/4, or None: the client-id
    record's rules, then the username record's, then the `all` rules
    (emqx_authz_mnesia.erl:98-120), each compiled and matched by acl_ref (:222-229)."""
    for src, key in ((CLIENTID, ("clientid", client["clientid"])), (USERNAME, ("username", client["username"])),
                     (ALL, "all")):
        if key != "all" and key[1] is None:
            continue
        for pos, (perm, action, tf) in enumerate(table.get(key, [])):
            if AR.match(client, pubsub, topic, AR.compile((perm, "all", action, [tf]))) != "nomatch":
                return (AC.PERM[perm], src, pos)
    return None


def answer(d):
    """decide's result as authorize/4's."""
    return "nomatch" if d is None else ("matched", "allow" if d[0] else "deny")


class Script:
    def __init__(self, clients, hash_bits=0, pass_names=0):
        self.clients, self.hash_bits, self.pass_names = list(clients), hash_bits, pass_names
        self.ops, self.table, self.pending = [], {}, []

    # mutations: pending until commit
    def store(self, key, rules):
        self.ops.append(("store", key, list(rules)))
        self.pending.append((key, list(rules)))

    def store_many(self, records):
        records = [(k, list(r)) for k, r in records]
        self.ops.append(("many", records))
        self.pending += records

    def delete(self, key):
        self.ops.append(("delete", key))
        self.pending.append((key, None))

    def purge(self):
        self.ops.append(("purge",))
        self.pending = [("purge", None)]

    def commit(self):
        self.ops.append(("commit",))
        self.table = self._after()
        self.pending = []

    def tune(self, key, value):
        self.ops.append(("tune", key, value))

    def refused(self):
        """The refused calls (a bad kind, permission, action or offsets, 65,537 rules, a client
        index out of range, a request's action `all`): each returns -EINVAL."""
        self.ops.append(("refused",))

    def _after(self):
        t = dict(self.table)
        for key, rules in self.pending:
            if key == "purge":
                t = {}
            elif rules is None:
                t.pop(key, None)
            else:
                t[key] = rules
        return t

    def query(self, reqs):
        reqs = list(reqs)
        want = [decide(self.clients[c], p, n, self.table) for c, p, n in reqs]
        self.ops.append(("query", reqs, want, len(self._after())))

    def queries(self):
        return [op for op in self.ops if op[0] == "query"]


def load(table, clients, reqs, hash_bits=0, pass_names=0, many=True):
    """The script of a fixed table: one store_many (or one store per record), a commit, a query."""
    s = Script(clients, hash_bits, pass_names)
    if many:
        s.store_many(table.items())
    else:
        for k, r in table.items():
            s.store(k, r)
    s.commit()
    s.query(reqs)
    return s


# ---- tokens and homes (gm_common.h word_token, gm_acl_match.h acl_value_token, adb_home) --------

def key_token(key: bytes, bits: int) -> int:
    if bits:
        return TOK_HASHED | AC.hash_token(key, bits)
    if len(key) <= 7:
        return int.from_bytes(key, "little") | (len(key) << 56)
    h = 0xcbf29ce484222325
    for c in key:
        h = (h ^ c) * 0x100000001b3 & AC.M64
    return TOK_HASHED | (AC.fmix64(h) >> 1)


def home(key: bytes, bits: int, slots: int) -> int:
    return AC.fmix64((key_token(key, bits) + HOME_ADD) & AC.M64) & (slots - 1)


# ---- key lengths, undefined values, filter forms --------------------------------------------------

def keys_table():
    """Every key as a client id and as a username with different rules; placeholder and eq filters
    in all three record kinds."""
    t = {}
    for k, key in enumerate(KEYS):
        t[("clientid", key)] = [("deny", "subscribe", b"t/k%d" % k), ("allow", "publish", b"t/k%d" % k),
                                ("allow", "all", b"c/${clientid}/+"), ("deny", "publish", b"eq e/${username}")]
        t[("username", key)] = [("allow", "subscribe", b"t/k%d" % k), ("deny", "all", b"t/+"),
                                ("deny", "all", b"u/${username}"), ("allow", "all", b"eq c/+/x")]
    t["all"] = [("allow", "subscribe", b"c/${clientid}/#"), ("deny", "publish", b"eq e/${clientid}"),
                ("allow", "publish", b"all/${username}")]
    return t


def keys_case(hash_bits=0):
    names = [b"t/k%d" % k for k in range(len(KEYS))] + [b"t/none", b"e/${username}", b"e/${clientid}", b"c/+/x"]
    for v in AC.VALUES:
        names += [b"c/" + v + b"/x", b"u/" + v, b"all/" + v, b"c/" + v]
    reqs = [(c, p, n) for c in range(len(AC.CLIENTS)) for n in names for p in ("publish", "subscribe")]
    return load(keys_table(), AC.CLIENTS, reqs, hash_bits)


# ---- source order -------------------------------------------------------------------------------

ORDER_CLIENTS = [{"clientid": b"dev", "username": b"bob", "peerhost": None},
                 {"clientid": b"bob", "username": b"dev", "peerhost": None},   # the same bytes, the other kind
                 {"clientid": b"e1", "username": b"bob", "peerhost": None},    # an empty record
                 {"clientid": b"e2", "username": b"bob", "peerhost": None}]    # an absent one


def order_case(hash_bits=0):
    t = {("clientid", b"dev"): [("allow", "publish", b"x/1")],
         ("username", b"bob"): [("deny", "all", b"x/+")],
         ("clientid", b"e1"): [],
         "all": [("allow", "subscribe", b"y/#")]}
    names = [b"x/1", b"y/z", b"q"]
    reqs = [(c, p, n) for c in range(len(ORDER_CLIENTS)) for p in ("publish", "subscribe") for n in names]
    return load(t, ORDER_CLIENTS, reqs, hash_bits, many=False)


# ---- the random case ----------------------------------------------------------------------------

FILTER_POOL = [b"d/${clientid}/#", b"u/${username}/+", b"shared/#", b"d/+/state", b"u/+/cmd/#", b"eq d/x",
               b"eq u/${username}/cmd", b"a/+", b"+/b", b"#"]


def random_case(hash_bits=0, pass_names=0, n_requests=4007):
    """A few hundred records keyed by client id and by username, with the keys of keys_case among
    them, and the `all` record; 4,007 requests whose names end with the rule sets' edge names."""
    rng = random.Random(77)
    ids = [b"dev-%03d" % i for i in range(150)] + KEYS
    users = [b"user-%03d" % i for i in range(100)] + KEYS

    def rs():
        return [(rng.choice(["allow", "deny"]), rng.choice(["publish", "subscribe", "all"]),
                 rng.choice(FILTER_POOL[:-1])) for _ in range(rng.randint(0, 3))]
    t = {}
    for c in ids:
        t[("clientid", c)] = rs()
    for u in users:
        t[("username", u)] = rs()
    t["all"] = [("deny", "subscribe", b"shared/secret"), ("allow", "all", b"shared/#"), ("deny", "publish", b"a/#")]
    clients = [{"clientid": rng.choice(ids + [b"stranger", None]), "username": rng.choice(users + [b"nobody", None]),
                "peerhost": None} for _ in range(300)] + AC.CLIENTS
    reqs = []
    for _ in range(n_requests - len(RR.EDGE_NAMES)):
        c = rng.randrange(len(clients))
        cid, usr = clients[c]["clientid"] or b"x", clients[c]["username"] or b"y"
        n = rng.choice([b"d/" + cid + b"/t", b"u/" + usr + b"/cmd", b"d/" + cid, b"shared/secret", b"shared/x",
                        b"d/" + cid + b"/state", b"u/" + usr + b"/cmd/go", b"other", b"d/x", AC.rand_name(rng)])
        reqs.append((c, rng.choice(["publish", "subscribe"]), n))
    reqs += [(rng.randrange(len(clients)), rng.choice(["publish", "subscribe"]), n) for n in RR.EDGE_NAMES]
    return load(t, clients, reqs, hash_bits, pass_names)


def block_case(n):
    """The last n requests (the edge names among them) of the random case."""
    s = random_case()
    reqs = s.queries()[0][1]
    return load(s.table, s.clients, reqs[len(reqs) - n:])


# ---- depth --------------------------------------------------------------------------------------

def flat_rules(rules):
    """acl_cases rules (permission, "all", action, [filters]) as records' rules, one per filter."""
    out = []
    for perm, who, action, fs in rules:
        assert who == "all"
        out += [(perm, action, b"eq " + AR._bin(f[1]) if isinstance(f, tuple) else AR._bin(f)) for f in fs]
    return out


def depth_case(hash_bits=0):
    """acl_cases.depth_case (names of 15 to 42 levels, filters of 16, 17, 40 and 41) in all three
    record kinds."""
    rules, clients, reqs = AC.depth_case()
    flat = flat_rules(rules)
    t = {("clientid", b"a"): flat[::-1], ("username", b"ninebytes"): flat[2:], "all": flat}
    return load(t, clients, reqs, hash_bits)


# ---- run and tile sizes -------------------------------------------------------------------------

RUN_CLIENTS = [{"clientid": b"one", "username": None, "peerhost": None},
               {"clientid": b"r300", "username": None, "peerhost": None},
               {"clientid": b"big", "username": b"r300", "peerhost": None}]


def runs_case(hash_bits=0):
    """Runs of 1, 300 and 65,536 rules (the limit), each decided by its last rule; no `all`."""
    t = {("clientid", b"one"): [("allow", "all", b"r/last")],
         ("clientid", b"r300"): [("deny", "all", b"r/%d" % i) for i in range(299)] + [("allow", "all", b"r/last")],
         ("username", b"r300"): [("deny", "publish", b"r/%d" % i) for i in range(299)] + [("deny", "all", b"r/+")],
         ("clientid", b"big"): [("deny", "all", b"r/%d" % i) for i in range(MAX_RULES - 1)] + [("allow", "publish", b"r/last")]}
    reqs = [(c, p, n) for c in range(2) for p in ("publish", "subscribe") for n in (b"r/last", b"r/7", b"r/none")]
    reqs += [(2, "publish", b"r/last"), (2, "subscribe", b"r/7"), (2, "subscribe", b"r/none")]
    return load(t, RUN_CLIENTS, reqs, hash_bits)


def tiling_rules():
    """The `all` record over three tiles.  A rule of one 16-level filter takes 20 words: 51 of
    them (1,020), then rule 51 whose 17-level filter is a two-word record that ends at word 1,024
    exactly; rule 52, which decides b/x, starts tile 1; 50 more rules fill tile 1 to word 1,005,
    the next does not fit and opens tile 2; the last rule decides everything left."""
    def fill(i):
        return ("deny", "all", b"/".join(b"f%d" % i for _ in range(16)))
    rules = [fill(i) for i in range(51)]
    rules.append(("deny", "publish", b"/".join([b"a"] * 17)))   # 51
    rules.append(("allow", "all", b"b/#"))                       # 52
    rules += [fill(i) for i in range(53, 104)]
    rules.append(("allow", "all", b"#"))                         # 104
    return rules


def tiling_case(hash_bits=0):
    names = [b"b/x", b"b", b"/".join([b"a"] * 17), b"/".join([b"f7"] * 16), b"/".join([b"f60"] * 16),
             b"/".join([b"f103"] * 16), b"x"]
    reqs = [(c, p, n) for c in (4, 5) for p in ("publish", "subscribe") for n in names]
    return load({"all": tiling_rules()}, AC.CLIENTS, reqs, hash_bits)


def empty_all_case():
    """An `all` record with no rules, against the same table without one."""
    t = {("clientid", b"a"): [("allow", "all", b"t/#")], "all": []}
    reqs = [(c, "publish", n) for c in (0, 1) for n in (b"t/x", b"x")]
    return load(t, AC.CLIENTS, reqs)


# ---- table shapes -------------------------------------------------------------------------------

def chain_keys(hash_bits):
    """Four keys with one home among the last three slots of the smallest table: stored in order
    they take four slots in a row, past the table's end (a chain of four that wraps).  With
    word_hash_bits 4 they are ten bytes long and have one token: only the byte check separates
    them."""
    out, want = [], None
    for i in range(100000):
        k = (b"chain-%04d" % i) if hash_bits else (b"k%d" % i)
        h = home(k, hash_bits, MIN_SLOTS)
        if h < MIN_SLOTS - 3:
            continue
        mine = (h, key_token(k, hash_bits) if hash_bits else 0)
        want = want or mine
        if mine != want:
            continue
        out.append(k)
        if len(out) == 4:
            return out
    raise AssertionError("no chain")


def shapes_case(hash_bits=0):
    """The table at its smallest size: the chain, a delete in its middle, the key stored again."""
    ks = chain_keys(hash_bits)
    clients = [{"clientid": k, "username": k, "peerhost": None} for k in ks]
    reqs = [(c, p, n) for c in range(4) for p in ("publish", "subscribe") for n in (b"s/c", b"s/u", b"s/x")]
    s = Script(clients, hash_bits)
    for i, k in enumerate(ks):
        s.store(("clientid", k), [("allow" if i % 2 else "deny", "all", b"s/c")])
        s.store(("username", k), [("deny" if i % 2 else "allow", "publish", b"s/+")])
    s.commit()
    s.query(reqs)                      # 0: the chain of four, wrapped
    s.delete(("clientid", ks[1]))
    s.delete(("username", ks[1]))
    s.commit()
    s.query(reqs)                      # 1: keys 2 and 3 are found past the deleted slot
    s.store(("clientid", ks[1]), [("allow", "subscribe", b"s/#")])
    s.commit()
    s.query(reqs)                      # 2: stored again, into the deleted slot
    return s


# ---- the update script ----------------------------------------------------------------------------

UPD_CLIENTS = [{"clientid": b"u%d" % i, "username": b"n%d" % (i % 7), "peerhost": None} for i in range(40)]


def update_case(hash_bits=0):
    """store -> match (not visible) -> commit -> replace -> delete -> purge, a query after every
    step; stores enough to grow every pool and rehash both tables; a forced rebuild."""
    reqs = [(c, p, n) for c in range(len(UPD_CLIENTS)) for p in ("publish", "subscribe")
            for n in (b"v/1", b"v/2", b"w/u%d" % c, b"z")]
    s = Script(UPD_CLIENTS, hash_bits)
    s.query(reqs)                                                           # 0: the empty database
    s.store(("clientid", b"u0"), [("allow", "all", b"v/1")])
    s.store(("username", b"n1"), [("deny", "all", b"v/+")])
    s.store("all", [("allow", "subscribe", b"w/${clientid}")])
    s.query(reqs)                                                           # 1: stored, not visible
    s.commit()
    s.query(reqs)                                                           # 2
    s.refused()
    s.query(reqs)                                                           # 3: refused calls change nothing
    s.store(("clientid", b"u0"), [("deny", "publish", b"v/1"), ("allow", "all", b"v/#")])   # replace
    s.store(("clientid", b"u0"), [("deny", "publish", b"v/2"), ("allow", "all", b"v/#")])   # twice before a commit
    s.store("all", [("deny", "subscribe", b"w/${clientid}"), ("allow", "all", b"z")])
    s.commit()
    s.query(reqs)                                                           # 4
    s.delete(("username", b"n1"))
    s.delete(("username", b"absent"))                                       # a no-op
    s.commit()
    s.query(reqs)                                                           # 5
    # one store per commit, then many: the pools grow, the tables pass load 1/2 and are rehashed
    for i in range(1, 6):
        s.store(("clientid", b"u%d" % i), [("allow", "publish", b"v/%d" % (1 + i % 2))])
        s.store(("username", b"n%d" % i), [("deny", "subscribe", b"v/+"), ("allow", "all", b"w/+")])
        s.commit()
    s.query(reqs)                                                           # 6
    s.store_many([(("clientid", b"u%d" % i), [("deny", "all", b"w/${clientid}"), ("allow", "all", b"v/2")] * 20)
                  for i in range(6, 40)])
    s.delete("all")
    s.commit()
    s.query(reqs)                                                           # 7
    # longer runs for the same keys and 24 new keys, which the tables hold without a rehash: every
    # pool outgrows its allocation in this one commit
    s.store_many([(("clientid", b"u%d" % i), [("deny", "all", b"w/${clientid}"), ("allow", "all", b"v/1")] * 30)
                  for i in range(6, 40)] +
                 [(("clientid", b"x-key-%02d-padding" % i), [("allow", "all", b"z")]) for i in range(24)])
    s.commit()
    s.query(reqs)                                                           # 8
    s.tune("rebuild_garbage_pct", 1)
    # u7's record stored again as it is: its old run is garbage, which forces the rebuild, and no
    # answer changes
    s.store(("clientid", b"u7"), [("deny", "all", b"w/${clientid}"), ("allow", "all", b"v/1")] * 30)
    s.commit()
    s.query(reqs)                                                           # 9: equal to 8
    s.tune("rebuild_garbage_pct", 100)
    s.store(("clientid", b"u8"), [("allow", "all", b"eq z")])
    s.purge()                                                               # drops the pending store too
    s.store(("username", b"n2"), [("allow", "all", b"z")])
    s.query(reqs)                                                           # 10: nothing of it visible yet
    s.commit()
    s.query(reqs)                                                           # 11: only n2's record
    return s


def all_edits_case():
    """The `all` record replaced twelve times and nothing else stored: the streams it leaves
    behind are garbage that a rebuild has to take away."""
    s = Script(AC.CLIENTS)
    reqs = [(c, p, n) for c in (0, 1) for p in ("publish", "subscribe") for n in (b"g/1", b"g/12", b"x")]
    for i in range(1, 13):
        s.store("all", [("allow" if i % 2 else "deny", "all", b"g/%d" % i), ("deny", "publish", b"eq x")])
        s.commit()
        s.query(reqs)
    return s


# ---- batches and passes ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(name, hash_bits=0, arg=None):
    """A named script, built once."""
    if name == "block":
        return block_case(arg)
    if name == "passes":
        return random_case(0, PASS_NAMES)
    if name == "empty_all":
        return empty_all_case()
    if name == "all_edits":
        return all_edits_case()
    return {"keys": keys_case, "order": order_case, "random": random_case, "depth": depth_case, "runs": runs_case,
            "tiling": tiling_case, "shapes": shapes_case, "update": update_case}[name](hash_bits)


# ---- the input file of tests/host_harness/acldb_dev_main.cpp and its output ----------------------

def _hex(b) -> str:
    return (b or b"").hex() or "-"


def _key(key):
    return (ALL, b"") if key == "all" else (KIND[key[0]], key[1])


def _rules_text(rules):
    return [f"{AC.PERM[p]} {AC.ACTION[a]} {_hex(f)}" for p, a, f in rules]


def input_text(s: Script) -> str:
    lines = [f"{s.hash_bits} {s.pass_names}", str(len(s.clients))]
    for c in s.clients:
        flags = (AC.NO_CLIENTID if c["clientid"] is None else 0) | (AC.NO_USERNAME if c["username"] is None else 0)
        lines.append(f"{flags} {_hex(c['clientid'])} {_hex(c['username'])}")
    for op in s.ops:
        if op[0] == "store":
            k, key = _key(op[1])
            lines.append(f"S {k} {_hex(key)} {len(op[2])}")
            lines += _rules_text(op[2])
        elif op[0] == "many":
            lines.append(f"M {len(op[1])}")
            for key, rules in op[1]:
                k, key = _key(key)
                lines.append(f"{k} {_hex(key)} {len(rules)}")
                lines += _rules_text(rules)
        elif op[0] == "delete":
            k, key = _key(op[1])
            lines.append(f"D {k} {_hex(key)}")
        elif op[0] == "purge":
            lines.append("P")
        elif op[0] == "commit":
            lines.append("C")
        elif op[0] == "tune":
            lines.append(f"T {op[1]} {op[2]}")
        elif op[0] == "refused":
            lines.append("R")
        else:
            lines.append(f"Q {len(op[1])}")
            lines += [f"{c} {AC.ACTION[p]} {_hex(n)}" for c, p, n in op[1]]
    lines.append("E")
    return "\n".join(lines) + "\n"


def parse_output(stdout: str, s: Script):
    """Per query: (answers: None or (perm, src, pos), the STATS line as a dict, the COUNT line)."""
    out = stdout.split("\n")
    at, res = 0, []
    for op in s.queries():
        n = len(op[1])
        rows = [None if line == "-" else tuple(map(int, line.split())) for line in out[at:at + n]]
        assert out[at + n].startswith("STATS ") and out[at + n + 1].startswith("COUNT "), out[at + n:at + n + 2]
        st = dict(zip(STAT_KEYS, map(int, out[at + n].split()[1:])))
        res.append((rows, st, int(out[at + n + 1].split()[1])))
        at += n + 2
    assert out[at:] == [""], out[at:at + 3]
    return res


def check(s: Script, results):
    """Every query's answers and record count against the reference."""
    qs = s.queries()
    assert len(results) == len(qs)
    for q, ((_, reqs, want, count), (rows, st, got_count)) in enumerate(zip(qs, results)):
        bad = [(q, reqs[i], rows[i], want[i]) for i in range(len(reqs)) if rows[i] != want[i]]
        assert not bad, bad[:5]
        assert got_count == count, (q, got_count, count)
    return [st for _, st, _ in results]
