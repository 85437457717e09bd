"""Reference semantics of ACL rule lists (emqx_amd/csrc/gm_acl_match.h, DESIGN.md 6b "ACL
lists"): emqx_authz_rule (apps/emqx_authz/src/emqx_authz_rule.erl) restated line by line on the
oracle's emqx_topic:words/1 and match/2 (oracle/emqx_ref.py), and emqx_authz_mnesia's list
assembly (apps/emqx_authz/src/emqx_authz_mnesia.erl).  A helper, not a test.

Terms: an atom is a ``str``, a binary is ``bytes`` (the oracle's word representation: the words
``""``, ``"+"`` and ``"#"`` of a topic are atoms, every other word a binary), a tuple a tuple, a
list a list; ``None`` is the atom ``undefined``.  A fed client id or username is put into a word
list as ``bytes``, so it equals no atom: that alone gives the rules for the values ``""``,
``"+"`` and ``"#"``.  Source strings (Erlang strings or binaries) are ``str`` or ``bytes``.
A compiled regex is ``("re_pattern", <compiled re>)``; Python's ``re`` stands in for PCRE.
"""
import ipaddress
import re

from oracle import emqx_ref as R

PH_CLIENTID = b"${clientid}"  # emqx_placeholder.hrl:31
PH_USERNAME = b"${username}"  # emqx_placeholder.hrl:33


def _bin(x) -> bytes:
    """:120-123 bin/1."""
    return x.encode() if isinstance(x, str) else bytes(x)


def _addr(a) -> tuple:
    p = a.packed
    return tuple(p) if len(p) == 4 else tuple(int.from_bytes(p[i:i + 2], "big") for i in range(0, 16, 2))


def cidr_parse(s) -> tuple:
    """esockd_cidr:parse(CIDR, true) -> {Start, End, Len}."""
    net = ipaddress.ip_network(_bin(s).decode(), strict=False)
    return (_addr(net.network_address), _addr(net.broadcast_address), net.prefixlen)


def cidr_match(ip: tuple, cidr: tuple) -> bool:
    """esockd_cidr:match/2."""
    return len(ip) == len(cidr[0]) and cidr[0] <= ip <= cidr[1]


def compile(rule):  # noqa: A001
    """:61-71 compile/1."""
    if len(rule) == 2 and rule[1] == "all":  # :61-64
        assert rule[0] in ("allow", "deny")
        return (rule[0], "all", "all", [compile_topic(b"#")])
    perm, who, action, filters = rule  # :65-71
    assert perm in ("allow", "deny") and action in ("publish", "subscribe", "all") and isinstance(filters, list)
    return (perm, compile_who(who), action, [compile_topic(t) for t in filters])


def compile_who(who):
    """:73-96 compile_who/1."""
    if who == "all":
        return "all"
    k, a = who
    if k == "user":
        return compile_who(("username", a))
    if k == "username" and isinstance(a, tuple) and a[0] == "re":
        return ("username", ("re_pattern", re.compile(_bin(a[1]))))
    if k == "username":
        return ("username", ("eq", _bin(a)))
    if k == "client":
        return compile_who(("clientid", a))
    if k == "clientid" and isinstance(a, tuple) and a[0] == "re":
        return ("clientid", ("re_pattern", re.compile(_bin(a[1]))))
    if k == "clientid":
        return ("clientid", ("eq", _bin(a)))
    if k == "ipaddr":
        return ("ipaddr", cidr_parse(a))
    if k == "ipaddrs":
        return ("ipaddrs", [cidr_parse(c) for c in a])
    if k in ("and", "or") and isinstance(a, list):
        return (k, [compile_who(w) for w in a])
    raise ValueError(who)


def compile_topic(t):
    """:98-107 compile_topic/1."""
    if isinstance(t, tuple) and t[0] == "eq":  # :100-101
        return ("eq", R.words(_bin(t[1])))
    t = _bin(t)
    if t[:3] == b"eq ":  # :98-99
        return ("eq", R.words(t[3:]))
    ws = R.words(t)  # :102-107
    return ("pattern", ws) if pattern(ws) else ws


def pattern(ws) -> bool:
    """:109-110."""
    return PH_USERNAME in ws or PH_CLIENTID in ws


def matches(client, pubsub, topic, rules):
    """:125-133 matches/4."""
    for rule in rules:
        m = match(client, pubsub, topic, rule)
        if m != "nomatch":
            return m
    return "nomatch"


def match(client, pubsub, topic, rule):
    """:135-145 match/4."""
    perm, who, action, filters = rule
    if match_action(pubsub, action) and match_who(client, who) and match_topics(client, topic, filters):
        return ("matched", perm)
    return "nomatch"


def match_action(pubsub, action) -> bool:
    """:147-150."""
    return pubsub == action if action in ("publish", "subscribe") else action == "all"


def match_who(client, who) -> bool:
    """:152-200 match_who/2.  client: dict with clientid, username (bytes or None = undefined)
    and peerhost (an address tuple or None)."""
    if who == "all":  # :152-153
        return True
    k, a = who
    if k == "username":
        if client["username"] is None:  # :154-155
            return False
        if a[0] == "eq":  # :156-157
            return client["username"] == a[1]
        return a[1].search(client["username"]) is not None  # :158-162
    if k == "clientid":
        if a[0] == "eq":  # :163-164 (the atom undefined equals no binary)
            return client["clientid"] is not None and client["clientid"] == a[1]
        # :165-169; re:run(undefined, MP) raises in the reference: taken as no match here
        return client["clientid"] is not None and a[1].search(client["clientid"]) is not None
    if k == "ipaddr":  # :170-173
        return client["peerhost"] is not None and cidr_match(client["peerhost"], a)
    if k == "ipaddrs":  # :174-182
        return client["peerhost"] is not None and any(cidr_match(client["peerhost"], c) for c in a)
    if k == "and":  # :183-190
        return all(match_who(client, w) for w in a)
    if k == "or":  # :191-198
        return any(match_who(client, w) for w in a)
    return False  # :199-200


def match_topics(client, topic, filters) -> bool:
    """:202-210 match_topics/3."""
    for f in filters:
        if isinstance(f, tuple) and f[0] == "pattern":
            f = feed_var(client, f[1])
        if match_topic(R.words(topic), f):
            return True
    return False


def match_topic(topic_words, f) -> bool:
    """:212-215 match_topic/2."""
    if isinstance(f, tuple) and f[0] == "eq":
        return topic_words == f[1]
    return R.match(topic_words, f)


def feed_var(client, ws):
    """:217-230 feed_var/2,3: the fed value is a binary (bytes)."""
    out = []
    for w in ws:
        if w == PH_CLIENTID:
            out.append(PH_CLIENTID if client["clientid"] is None else bytes(client["clientid"]))
        elif w == PH_USERNAME:
            out.append(PH_USERNAME if client["username"] is None else bytes(client["username"]))
        else:
            out.append(w)
    return out


# ---- emqx_authz_mnesia ------------------------------------------------------------------

def mnesia_authorize(client, pubsub, topic, table):
    """emqx_authz_mnesia:authorize/4 (:98-120) with do_authorize/4 (:222-229).  table: dict
    from ("clientid", C), ("username", U) or "all" to [(permission, action, topic_filter)]."""
    rules = (table.get(("clientid", client["clientid"]), []) + table.get(("username", client["username"]), []) +
             table.get("all", []))
    for perm, action, tf in rules:
        m = match(client, pubsub, topic, compile((perm, "all", action, [tf])))
        if m != "nomatch":
            return m
    return "nomatch"


# ---- terms as JSON data (tests/golden/authz_rule_vectors.json) -----------------------------

def term_json(t):
    """A compiled term as JSON data: atom {"a": name}, binary {"b": text}, tuple {"t": [...]},
    list [...], integer; a compiled regex {"re_pattern": true}."""
    if isinstance(t, re.Pattern):
        return {"re_pattern": True}
    if isinstance(t, str):
        return {"a": t}
    if isinstance(t, (bytes, bytearray)):
        return {"b": bytes(t).decode()}
    if isinstance(t, tuple):
        if len(t) == 2 and t[0] == "re_pattern":
            return {"re_pattern": True}
        return {"t": [term_json(x) for x in t]}
    if isinstance(t, list):
        return [term_json(x) for x in t]
    assert isinstance(t, int), t
    return t


def term_from_json(j):
    """Source terms of the golden file: {"a"}, {"b"}, {"s": Erlang string}, {"t"}, lists."""
    if isinstance(j, dict):
        if "a" in j:
            return j["a"]
        if "b" in j:
            return j["b"].encode()
        if "s" in j:
            return j["s"]
        return tuple(term_from_json(x) for x in j["t"])
    if isinstance(j, list):
        return [term_from_json(x) for x in j]
    return j
