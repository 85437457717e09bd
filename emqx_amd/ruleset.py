"""Rule lists that keep every match, matched on the device against a resident list (DESIGN.md
6b): the loops that run once per publish beside the route match.

* ``get_rules_for_topic(ruleset, topic)`` -- ``emqx_rule_engine:get_rules_for_topic/1``
  (apps/emqx_rule_engine/src/emqx_rule_engine.erl:198-204): the rules one of whose ``from``
  filters matches (``emqx_plugin_libs_rule:can_topic_match_oneof/2``,
  emqx_plugin_libs_rule.erl:340-346), in list order.
* ``get_matched_egress_bridges(ruleset, topic)`` -- ``emqx_bridge:get_matched_egress_bridges/1``
  (emqx_bridge.erl:342-382): the same over the bridges' local topics.
* the exhook and trace topic filters (emqx_exhook_server.erl:361, emqx_trace_handler.erl:138)
  are a ``RuleSet`` with one filter per rule.

A rule is a sequence of filters; a filter is ``bytes`` (``emqx_topic:match/2`` on binaries, the
'$' clauses apply), ``("words", F)`` (match/2 on word lists) or ``("eq", F)`` (word-list
equality).  The list is compiled once (``set``) and stays on the device; ``match`` takes batches
of names.

    rs = RuleSet([[b"t/#", b"u/+"], [("eq", b"t/1")]])
    rs.match([b"t/1", b"x"])        # -> [[0, 1], []]
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import engine as E

STAT_KEYS = ("records", "tiles", "filters", "rules", "candidates", "removed", "deep", "visited")


def _flag_of(f) -> Tuple[int, bytes]:
    if isinstance(f, tuple):
        kind, f = f
        if kind == "eq":
            return E.RULE_EQ, bytes(f)
        if kind == "words":
            return E.RULE_WORDS, bytes(f)
        raise ValueError(f"unknown filter kind {kind!r}")
    return 0, bytes(f)


class RuleSet:
    def __init__(self, rules: Sequence[Sequence] = (), device: int = 0, word_hash_bits: int = 0):
        self._lib = E.lib()
        self._h = None
        h = C.c_void_p()
        rc = self._lib.emqxgm_ruleset_create(device, word_hash_bits, C.byref(h))
        if rc != 0:
            raise E.EngineError(f"emqxgm_ruleset_create failed: {rc}")
        self._h = h
        self.n_rules = 0
        self.set(rules)

    def close(self):
        if self._h:
            self._lib.emqxgm_ruleset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc < 0:
            raise E.EngineError(f"{what} failed: {rc}")
        return rc

    def set(self, rules: Sequence[Sequence]) -> None:
        """Replaces the whole list; rule i is rules[i]."""
        flags, filters, owner = [], [], []
        for r, rule in enumerate(rules):
            for f in rule:
                fg, fb = _flag_of(f)
                flags.append(fg)
                filters.append(fb)
                owner.append(r)
        self.set_raw(filters, flags, owner, len(rules))

    def set_raw(self, filters: Sequence[bytes], flags: Sequence[int], filter_rule: Sequence[int],
                n_rules: int) -> None:
        """emqxgm_ruleset_set as it is: filter i belongs to rule filter_rule[i] (non-decreasing).
        A refused list raises and leaves the one in force unchanged."""
        buf, off = E.pack(list(filters), np.uint32)
        fg = np.asarray(flags, np.uint32)
        fr = np.asarray(filter_rule, np.uint32)
        self._check(self._lib.emqxgm_ruleset_set(self._h, E._ptr(buf), E._ptr(off), E._ptr(fg),
                                                 E._ptr(fr), len(filters), n_rules), "ruleset_set")
        self.n_rules = n_rules

    def match_csr(self, names: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
        """(ptr[n+1] u64, rule u32): name i matches rule[ptr[i]:ptr[i+1]], ascending, each once."""
        names = list(names)
        buf, off = E.pack(names, np.uint32)
        out = E._RulesetOut()
        self._check(self._lib.emqxgm_ruleset_match(self._h, E._ptr(buf), off.ctypes.data_as(C.c_void_p),
                                                   len(names), C.byref(out)), "ruleset_match")
        ptr = np.ctypeslib.as_array(out.ptr, shape=(len(names) + 1,)).copy()
        rule = (np.ctypeslib.as_array(out.rule, shape=(out.n_ids,)).copy() if out.n_ids
                else np.zeros(0, np.uint32))
        return ptr, rule

    def match(self, names: Sequence[bytes]) -> List[List[int]]:
        ptr, rule = self.match_csr(names)
        rule = rule.tolist()
        ptr = ptr.tolist()
        return [rule[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]

    def tune(self, key: str, value: int) -> None:
        self._check(self._lib.emqxgm_ruleset_tune(self._h, key.encode(), int(value)), "ruleset_tune")

    def kernel_times_us(self) -> Tuple[int, int]:
        """(count pass, fill pass) kernel microseconds summed since tune("timing", 1)."""
        return (self._check(self._lib.emqxgm_ruleset_tune(self._h, b"count_us", 0), "ruleset_tune"),
                self._check(self._lib.emqxgm_ruleset_tune(self._h, b"fill_us", 0), "ruleset_tune"))

    def stats(self) -> dict:
        a = (C.c_uint64 * 8)()
        self._check(self._lib.emqxgm_ruleset_stats(self._h, a), "ruleset_stats")
        return dict(zip(STAT_KEYS, (int(x) for x in a)))


def get_rules_for_topic(ruleset: RuleSet, topic: bytes) -> List[int]:
    return ruleset.match([topic])[0]


def get_matched_egress_bridges(ruleset: RuleSet, topic: bytes) -> List[int]:
    return ruleset.match([topic])[0]
