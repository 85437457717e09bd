"""ACL rule lists with client placeholders, matched on the device against a resident list
(DESIGN.md 6b "ACL lists"): the host-side mirror of ``emqx_authz_rule``
(apps/emqx_authz/src/emqx_authz_rule.erl) over ``emqx_amd.Acl``.

* ``compile(rule)`` -- ``emqx_authz_rule:compile/1`` (:61-110).  A rule is ``(permission, "all")``
  or ``(permission, who, action, [filter, ...])``; ``who`` is ``"all"``, ``("username", U)``,
  ``("clientid", C)`` (aliases ``"user"``, ``"client"``; ``U`` / ``C`` a string or ``("re", R)``),
  ``("ipaddr", CIDR)``, ``("ipaddrs", [CIDR, ...])``, ``("and", [who, ...])`` or
  ``("or", [who, ...])``; a filter is a string, ``"eq F"`` or ``("eq", F)``.  Strings are ``str`` or
  ``bytes``.  In the compiled term a word is ``bytes`` for a binary and one of the ``str`` atoms
  ``""``, ``"+"``, ``"#"`` (``emqx_topic:word/1``).
* ``AclList(rules).matches(clients, pubsubs, topics)`` -- ``emqx_authz_rule:matches/4``
  (:125-133) for a batch of requests, on the device: ``("matched", "allow" | "deny")`` or
  ``"nomatch"`` each.  It is ``emqx_authz_file:authorize/4`` (emqx_authz_file.erl:64-65).
* ``AclList.from_builtin_db(records)`` -- one list with the answers of
  ``emqx_authz_mnesia:authorize/4`` (emqx_authz_mnesia.erl:98-120, 222-229).

The device decides action, the principals ``all``, ``{username, {eq, U}}`` and
``{clientid, {eq, C}}``, the placeholder feed (``feed_var/2``, :217-230) and the topic match.
Every other principal is evaluated here, once per distinct client, and reaches the device as one
of 64 host slots.  Python's ``re`` stands in for PCRE in this mirror; a NIF caller evaluates the
same slots with ``re:run/2`` (:158-169) and ``esockd_cidr:match/2`` (:172-182).
"""
from __future__ import annotations

import ipaddress
import re
from typing import Dict, List, Optional, Sequence

from . import engine as E

PH_CLIENTID = b"${clientid}"  # emqx_placeholder.hrl:31
PH_USERNAME = b"${username}"  # emqx_placeholder.hrl:33
_ACTIONS = {"publish": E.ACL_PUBLISH, "subscribe": E.ACL_SUBSCRIBE, "all": E.ACL_ALL}
_PERMS = {"deny": E.ACL_DENY, "allow": E.ACL_ALLOW}


def _bin(x) -> bytes:
    """bin/1 (:120-123)."""
    return x.encode() if isinstance(x, str) else bytes(x)


def _atom(x) -> str:
    """atom/1 (:112-118)."""
    return x.decode() if isinstance(x, (bytes, bytearray)) else str(x)


def words(topic: bytes) -> list:
    """emqx_topic:words/1 (apps/emqx/src/emqx_topic.erl:162-169)."""
    return [w.decode() if w in (b"", b"+", b"#") else w for w in topic.split(b"/")]


def _cidr(s):
    """esockd_cidr:parse(CIDR, true): {Start, End, Len} with the addresses as tuples."""
    net = ipaddress.ip_network(_bin(s).decode(), strict=False)

    def tup(a):
        p = a.packed
        return tuple(p) if len(p) == 4 else tuple(int.from_bytes(p[i:i + 2], "big") for i in range(0, 16, 2))
    return (tup(net.network_address), tup(net.broadcast_address), net.prefixlen)


def compile_who(who):
    """compile_who/1 (:73-96)."""
    if who == "all":
        return "all"
    kind, arg = who
    kind = _atom(kind)
    if kind == "user":
        return compile_who(("username", arg))
    if kind == "client":
        return compile_who(("clientid", arg))
    if kind in ("username", "clientid"):
        if isinstance(arg, tuple) and _atom(arg[0]) == "re":
            return (kind, ("re_pattern", re.compile(_bin(arg[1]))))
        return (kind, ("eq", _bin(arg)))
    if kind == "ipaddr":
        return ("ipaddr", _cidr(arg))
    if kind == "ipaddrs":
        return ("ipaddrs", [_cidr(c) for c in arg])
    if kind in ("and", "or"):
        return (kind, [compile_who(w) for w in arg])
    raise ValueError(f"unknown principal {who!r}")


def compile_topic(t):
    """compile_topic/1 (:98-107) with pattern/1 (:109-110)."""
    if isinstance(t, tuple):
        if _atom(t[0]) != "eq":
            raise ValueError(f"unknown topic form {t!r}")
        return ("eq", words(_bin(t[1])))
    t = _bin(t)
    if t.startswith(b"eq "):
        return ("eq", words(t[3:]))
    ws = words(t)
    return ("pattern", ws) if PH_USERNAME in ws or PH_CLIENTID in ws else ws


def compile(rule):  # noqa: A001 -- the reference's name
    """emqx_authz_rule:compile/1 (:61-71)."""
    if len(rule) == 2 and rule[1] == "all" and _atom(rule[0]) in _PERMS:
        return (_atom(rule[0]), "all", "all", [compile_topic(b"#")])
    perm, who, action, filters = rule
    perm, action = _atom(perm), _atom(action)
    if perm not in _PERMS or action not in _ACTIONS or not isinstance(filters, (list, tuple)):
        raise ValueError(f"bad rule {rule!r}")
    return (perm, compile_who(who), action, [compile_topic(t) for t in filters])


def _peer(ip):
    if isinstance(ip, tuple):
        return ip
    p = ipaddress.ip_address(ip).packed
    return tuple(p) if len(p) == 4 else tuple(int.from_bytes(p[i:i + 2], "big") for i in range(0, 16, 2))


def _in_cidr(ip, cidr) -> bool:
    """esockd_cidr:match/2: same family and Start =< Ip =< End."""
    start, end, _ = cidr
    return len(ip) == len(start) and start <= ip <= end


def match_who(client: dict, who) -> bool:
    """match_who/2 (:152-200) on a compiled principal.  client: clientid / username (bytes or
    None = undefined) and peerhost (an address string or tuple, or None)."""
    if who == "all":
        return True
    kind, arg = who
    if kind in ("username", "clientid"):
        v = client.get(kind)
        if kind == "username" and v is None:
            return False  # :154-155
        if arg[0] == "eq":
            return v is not None and _bin(v) == arg[1]
        # re:run(undefined, MP) is a badarg in the reference; an undefined client id matches nothing
        return v is not None and arg[1].search(_bin(v)) is not None
    if kind == "ipaddr":
        ip = client.get("peerhost")
        return ip is not None and _in_cidr(_peer(ip), arg)
    if kind == "ipaddrs":
        ip = client.get("peerhost")
        return ip is not None and any(_in_cidr(_peer(ip), c) for c in arg)
    if kind == "and":
        return all(match_who(client, w) for w in arg)
    if kind == "or":
        return any(match_who(client, w) for w in arg)
    return False


def _who_key(who):
    """A hashable identity of a compiled principal (a compiled regex by its pattern)."""
    if who == "all":
        return who
    kind, arg = who
    if kind in ("and", "or"):
        return (kind, tuple(_who_key(w) for w in arg))
    if kind == "ipaddrs":
        return (kind, tuple(arg))
    if kind in ("username", "clientid") and arg[0] == "re_pattern":
        return (kind, ("re_pattern", arg[1].pattern))
    return (kind, arg)


def _join(ws) -> bytes:
    return b"/".join(w.encode() if isinstance(w, str) else w for w in ws)


class AclList:
    """A compiled rule list resident on the device.  ``rules`` are source rules (``compile`` is
    applied).  Raises ``ValueError`` when the list needs more than 64 host slots."""

    def __init__(self, rules: Sequence = (), device: int = 0, word_hash_bits: int = 0, compiled: bool = False):
        self.rules = [r if compiled else compile(r) for r in rules]
        self.slots: list = []  # slot k -> compiled principal
        self.plan = self._plan()
        self.acl = E.Acl(device=device, word_hash_bits=word_hash_bits)
        self.acl.set(*self.plan)

    def _plan(self):
        """emqxgm_acl_set's arguments for self.rules; assigns the host slots."""
        filters, flags, owner, perm, action, who, slot, strings = [], [], [], [], [], [], [], []
        slot_of: Dict[object, int] = {}
        for r, (p, w, a, fs) in enumerate(self.rules):
            perm.append(_PERMS[p])
            action.append(_ACTIONS[a])
            kind, s, string = E.ACL_WHO_ALL, 0, b""
            if w != "all":
                if w[0] in ("username", "clientid") and w[1][0] == "eq":
                    kind = E.ACL_WHO_USERNAME if w[0] == "username" else E.ACL_WHO_CLIENTID
                    string = w[1][1]
                else:
                    key = _who_key(w)
                    if key not in slot_of:
                        if len(self.slots) >= E.ACL_HOST_SLOTS:
                            raise ValueError(f"the list needs more than {E.ACL_HOST_SLOTS} host principals")
                        slot_of[key] = len(self.slots)
                        self.slots.append(w)
                    kind, s = E.ACL_WHO_HOST, slot_of[key]
            who.append(kind)
            slot.append(s)
            strings.append(string)
            for f in fs:
                eq = isinstance(f, tuple) and f[0] == "eq"
                filters.append(_join(f[1] if isinstance(f, tuple) else f))
                flags.append(E.RULE_EQ if eq else 0)
                owner.append(r)
        return filters, flags, owner, perm, action, who, slot, strings

    def close(self):
        self.acl.close()

    def who_bits(self, client: dict) -> int:
        return sum(1 << k for k, w in enumerate(self.slots) if match_who(client, w))

    def first_rules(self, clients: Sequence[dict], pubsubs: Sequence[str], topics: Sequence[bytes]) -> List[Optional[int]]:
        """The index of the first matching rule per request, or None."""
        table: Dict[tuple, int] = {}
        ids: List[Optional[bytes]] = []
        users: List[Optional[bytes]] = []
        bits: List[int] = []
        idx = []
        for c in clients:
            cid, usr = c.get("clientid"), c.get("username")
            cid = None if cid is None else _bin(cid)
            usr = None if usr is None else _bin(usr)
            key = (cid, usr, c.get("peerhost"))
            if key not in table:
                table[key] = len(ids)
                ids.append(cid)
                users.append(usr)
                bits.append(self.who_bits({"clientid": cid, "username": usr, "peerhost": c.get("peerhost")}))
            idx.append(table[key])
        act = [_ACTIONS[_atom(p)] for p in pubsubs]
        if any(a == E.ACL_ALL for a in act):
            raise ValueError("a request is publish or subscribe")
        out = self.acl.match([_bin(t) for t in topics], idx, act, ids, users, bits)
        return [None if int(r) == E.NONE else int(r) for r in out]

    def matches(self, clients: Sequence[dict], pubsubs: Sequence[str], topics: Sequence[bytes]):
        """emqx_authz_rule:matches/4 (:125-133) per request."""
        return ["nomatch" if r is None else ("matched", self.rules[r][0])
                for r in self.first_rules(clients, pubsubs, topics)]

    @staticmethod
    def builtin_db_rules(records) -> list:
        """The global source list of from_builtin_db: records are ``(key, rules)`` with key
        ``("clientid", C)``, ``("username", U)`` or ``"all"`` and rules
        ``[(permission, action, topic_filter), ...]`` (emqx_authz_mnesia.erl:41-58)."""
        out = []
        for want in ("clientid", "username", "all"):
            for key, rules in records:
                kind = key if key == "all" else _atom(key[0])
                if kind != want:
                    continue
                who = "all" if kind == "all" else (kind, _bin(key[1]))
                out += [(p, who, a, [t]) for p, a, t in rules]
        return out

    @classmethod
    def from_builtin_db(cls, records, **kw) -> "AclList":
        """One list for every client of the built-in database: the client-id-keyed rules (who =
        that client id), then the username-keyed ones, then the ``all`` rules.  Rules keyed to
        other clients never match, so a client's first match is the one of
        emqx_authz_mnesia:authorize/4's ``clientid ++ username ++ all`` order (:98-120), each rule
        compiled as ``{Permission, all, Action, [TopicFilter]}`` (:222-229)."""
        return cls(cls.builtin_db_rules(records), **kw)


class InvalidRule(ValueError):
    """normalize_rules/1's errors (emqx_authz_mnesia.erl:195-214): ``reason`` is one of
    ``invalid_rule``, ``invalid_rule_permission``, ``invalid_rule_action``, ``invalid_rule_topic``."""

    def __init__(self, reason: str, term):
        super().__init__(f"{reason}: {term!r}")
        self.reason, self.term = reason, term


def normalize_rules(rules) -> list:
    """normalize_rules/1 (:195-214): ``[(permission, action, topic)]`` with the atoms as ``str`` and
    the topic a string (``str``) or a binary (``bytes``) -> the same with every topic ``bytes``."""
    out = []
    for rule in rules:
        if not isinstance(rule, tuple) or len(rule) != 3:
            raise InvalidRule("invalid_rule", rule)
        perm, action, topic = rule
        if not isinstance(perm, str) or perm not in _PERMS:
            raise InvalidRule("invalid_rule_permission", perm)
        if not isinstance(action, str) or action not in _ACTIONS:
            raise InvalidRule("invalid_rule_action", action)
        if not isinstance(topic, (str, bytes, bytearray)):
            raise InvalidRule("invalid_rule_topic", topic)
        out.append((perm, action, _bin(topic)))
    return out


class BuiltinDb:
    """The built-in database resident on the device (DESIGN.md 6b "Built-in database"): the mirror
    of ``emqx_authz_mnesia`` (apps/emqx_authz/src/emqx_authz_mnesia.erl) over ``emqx_amd.AclDb``.
    ``who`` is ``("clientid", C)``, ``("username", U)`` or ``"all"`` (:41-58).  Mutations are
    pending until ``commit()``; ``authorize`` answers from the committed records, ``get_rules`` and
    ``record_count`` tell what is stored, pending mutations included."""

    def __init__(self, device: int = 0, word_hash_bits: int = 0):
        self.db = E.AclDb(device=device, word_hash_bits=word_hash_bits)
        self.records: Dict[object, list] = {}

    def close(self):
        self.db.close()

    @staticmethod
    def _who(who):
        if who == "all":
            return "all", E.ACLDB_ALL, b""
        kind, value = who
        kind = _atom(kind)
        if kind not in ("clientid", "username"):
            raise ValueError(f"unknown key {who!r}")
        value = _bin(value)
        return (kind, value), (E.ACLDB_CLIENTID if kind == "clientid" else E.ACLDB_USERNAME), value

    @staticmethod
    def _numbers(rules):
        return [(_PERMS[p], _ACTIONS[a], t) for p, a, t in rules]

    def store_rules(self, who, rules) -> None:
        """store_rules/2 (:132-150): replaces the record."""
        key, kind, value = self._who(who)
        rules = normalize_rules(rules)
        self.db.store(kind, value, self._numbers(rules))
        self.records[key] = rules

    def store_many(self, records) -> None:
        """store_rules/2 for ``[(who, rules)]`` in one call; all or nothing."""
        keyed = [(self._who(w), normalize_rules(r)) for w, r in records]
        self.db.store_many([(kind, value, self._numbers(r)) for (_, kind, value), r in keyed])
        for (key, _, _), r in keyed:
            self.records[key] = r

    def delete_rules(self, who) -> None:
        """delete_rules/1 (:152-164)."""
        key, kind, value = self._who(who)
        self.db.delete(kind, value)
        self.records.pop(key, None)

    def purge_rules(self) -> None:
        """purge_rules/0 (:166-169)."""
        self.db.purge()
        self.records.clear()

    def get_rules(self, who):
        """get_rules/1 (:175-188): ``("ok", rules)`` or ``"not_found"``."""
        key, _, _ = self._who(who)
        return ("ok", list(self.records[key])) if key in self.records else "not_found"

    def record_count(self) -> int:
        """record_count/0 (:171-173)."""
        return self.db.count()

    def commit(self) -> None:
        self.db.commit()

    def _decide(self, clients: Sequence[dict], pubsubs: Sequence[str], topics: Sequence[bytes]):
        """Per request ``None`` or ``(permission 0 | 1, source ACLDB_*, position of the deciding
        rule in its record)``."""
        table: Dict[tuple, int] = {}
        ids: List[Optional[bytes]] = []
        users: List[Optional[bytes]] = []
        idx = []
        for c in clients:
            cid, usr = c.get("clientid"), c.get("username")
            key = (None if cid is None else _bin(cid), None if usr is None else _bin(usr))
            if key not in table:
                table[key] = len(ids)
                ids.append(key[0])
                users.append(key[1])
            idx.append(table[key])
        act = [_ACTIONS[_atom(p)] for p in pubsubs]
        if any(a == E.ACL_ALL for a in act):
            raise ValueError("a request is publish or subscribe")
        perm, src, pos = self.db.match([_bin(t) for t in topics], idx, act, ids, users)
        return [None if int(p) == E.NONE else (int(p), int(s), int(q)) for p, s, q in zip(perm, src, pos)]

    def authorize(self, clients: Sequence[dict], pubsubs: Sequence[str], topics: Sequence[bytes]):
        """authorize/4 (:98-120) per request: ``("matched", "allow" | "deny")`` or ``"nomatch"``;
        emqx_access_control's no_match default stays with the caller."""
        return ["nomatch" if d is None else ("matched", "allow" if d[0] == E.ACL_ALLOW else "deny")
                for d in self._decide(clients, pubsubs, topics)]
