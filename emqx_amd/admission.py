"""Admission of topic names and topic filters on the device (emqxgm_admit_*, DESIGN.md 6b
"Admission"): the steps of the channel in front of the match.

``Admission`` answers, per item of a batch and in the reference's terms,

* ``validate(kind, items)``   emqx_topic:validate/2 (apps/emqx/src/emqx_topic.erl:98-130):
  ``True`` or the error atom's name;
* ``parse(items)``            emqx_topic:parse/1 (:206-233): ``(topic, options)`` or
  ``("invalid_topic_filter", item)``;
* ``check_publish`` / ``check_subscribe``  emqx_packet:check/1, parse and
  emqx_mqtt_caps:check_pub/2 / check_sub/3 in the channel's order: a reason code, 0 = admitted;
* ``check_subscribe_packet``  emqx_packet:check/1 of one SUBSCRIBE packet.

There is no CPU path: every answer comes from k_admit's records (``records``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import engine
from .engine import EngineError, _ptr, pack

NAME, FILTER = 0, 1  # EMQXGM_ADMIT_NAME, EMQXGM_ADMIT_FILTER
VERDICTS = ("ok", "empty_topic", "topic_too_long", "topic_name_error", "topic_invalid_#", "topic_invalid_char",
            "function_clause")  # EMQXGM_ADMIT_V_*
WILDCARD, SHARED, EXCLUSIVE, EXCL_LOOKUP = 1 << 24, 1 << 25, 1 << 26, 1 << 27
IN_RETAIN, IN_HAS_SHARE = 4, 8
RAISES = 0x100  # EMQXGM_ADMIT_RAISES
RC_TOPIC_FILTER_INVALID = 0x8F
STAT_KEYS = ("calls", "items", "bytes", "passes", "growths", "kernel_us")
# emqx_mqtt_caps.erl:61-72
DEFAULT_CAPS = dict(max_topic_levels=65535, max_qos_allowed=2, retain_available=True, wildcard_subscription=True,
                    shared_subscription=True, exclusive_subscription=False)


class _Caps(C.Structure):  # emqxgm_admit_caps
    _fields_ = [("max_topic_levels", C.c_uint32), ("max_qos_allowed", C.c_uint8), ("retain_available", C.c_uint8),
                ("wildcard_subscription", C.c_uint8), ("shared_subscription", C.c_uint8),
                ("exclusive_subscription", C.c_uint8), ("reserved", C.c_uint8 * 3)]


def _caps_table(caps) -> "C.Array":
    rows = [caps] if isinstance(caps, dict) or caps is None else list(caps)
    if not 1 <= len(rows) <= 256:
        raise ValueError("1..256 zones")
    t = (_Caps * len(rows))()
    for r, row in zip(t, rows):
        c = dict(DEFAULT_CAPS)
        c.update(row or {})
        r.max_topic_levels = int(c["max_topic_levels"])
        r.max_qos_allowed = int(c["max_qos_allowed"])
        r.retain_available = bool(c["retain_available"])
        r.wildcard_subscription = bool(c["wildcard_subscription"])
        r.shared_subscription = bool(c["shared_subscription"])
        r.exclusive_subscription = bool(c["exclusive_subscription"])
    return t


class Admission:
    """caps: one zone's caps (a dict over DEFAULT_CAPS) or a list of up to 256 of them, indexed
    by the ``zones`` argument of the checks."""

    def __init__(self, device: int = 0, caps=None):
        self._lib = engine.lib()
        self._h = None
        self._caps = _caps_table(caps)
        h = C.c_void_p()
        rc = self._lib.emqxgm_admit_create(device, C.byref(h))
        if rc != 0:
            raise EngineError(f"emqxgm_admit_create failed: {rc}")
        self._h = h

    def close(self):
        if self._h:
            self._lib.emqxgm_admit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc < 0:
            raise EngineError(f"{what} failed: {rc}")
        return rc

    def set_caps(self, caps) -> None:
        self._caps = _caps_table(caps)

    def tune(self, key: str, value: int) -> None:
        self._check(self._lib.emqxgm_admit_tune(self._h, key.encode(), int(value)), "admit_tune")

    def kernel_time_us(self) -> int:
        """Kernel microseconds summed since tune("timing", 1)."""
        return self._check(self._lib.emqxgm_admit_tune(self._h, b"kernel_us", 0), "admit_tune")

    def stats(self) -> Dict[str, int]:
        a = (C.c_uint64 * 6)()
        self._check(self._lib.emqxgm_admit_stats(self._h, a), "admit_stats")
        return dict(zip(STAT_KEYS, (int(x) for x in a)))

    def records(self, mode: int, items: Sequence[bytes], in_flags=None, zones=None) -> np.ndarray:
        """emqxgm_admit_batch -> u32 [n, 4] (include/emqx_gpumatch.h has the words)."""
        items = list(items)
        n = len(items)
        buf, off = pack(items, np.uint32)
        fl = None if in_flags is None else np.ascontiguousarray(np.asarray(in_flags, np.uint8))
        zn = None if zones is None else np.ascontiguousarray(np.asarray(zones, np.uint8))
        assert fl is None or len(fl) == n
        assert zn is None or len(zn) == n
        out = engine._U32P()
        self._check(self._lib.emqxgm_admit_batch(
            self._h, mode, _ptr(buf), off.ctypes.data_as(C.c_void_p), n, None if fl is None else _ptr(fl),
            None if zn is None else _ptr(zn), C.cast(self._caps, C.c_void_p), len(self._caps), C.byref(out)),
            "admit_batch")
        if n == 0:
            return np.zeros((0, 4), np.uint32)
        return np.ctypeslib.as_array(out, shape=(n * 4,)).reshape(n, 4).copy()

    def reason(self, mode: int, rec) -> int:
        """emqxgm_admit_reason of one record."""
        r = np.ascontiguousarray(np.asarray(rec, np.uint32))
        return int(self._lib.emqxgm_admit_reason(mode, _ptr(r)))

    def validate(self, kind: str, items: Sequence[bytes]) -> List:
        mode = {"name": NAME, "filter": FILTER}[kind]
        return [True if v == 0 else VERDICTS[v] for v in (self.records(mode, items)[:, 0] & 0xFF).tolist()]

    def parse(self, items: Sequence[bytes], has_share: Optional[Sequence[bool]] = None) -> List:
        """has_share[i]: the options passed with item i carry ``share`` already (as ``True``)."""
        items = list(items)
        fl = None if has_share is None else [IN_HAS_SHARE if h else 0 for h in has_share]
        out = []
        for i, (item, r) in enumerate(zip(items, self.records(FILTER, items, fl).tolist())):
            if (r[0] >> 8) & 0xFF:
                out.append(("invalid_topic_filter", item))
                continue
            o: Dict[str, object] = {}
            if r[0] & SHARED:
                o["share"] = item[7:7 + r[3]] if r[3] != engine.NONE else True
            if r[0] & EXCLUSIVE:
                o["is_exclusive"] = True
            out.append((item[r[2]:], o))
        return out

    def check_publish(self, names: Sequence[bytes], qos, retain, zones=None) -> List[int]:
        names = list(names)
        fl = [(int(q) & 3) | (IN_RETAIN if r else 0) for q, r in zip(qos, retain)]
        recs = self.records(NAME, names, fl, zones)
        return [self.reason(NAME, r) for r in recs]

    def check_subscribe(self, filters: Sequence[bytes], has_share=None, zones=None) -> List[int]:
        """Per filter: 0, a reason code, or RAISES where parse/1 raises inside handle_in.  A
        record's EXCL_LOOKUP (``records``) tells where the exclusive table is still to be asked."""
        filters = list(filters)
        fl = None if has_share is None else [IN_HAS_SHARE if h else 0 for h in has_share]
        recs = self.records(FILTER, filters, fl, zones)
        return [self.reason(FILTER, r) for r in recs]

    def check_subscribe_packet(self, filters: Sequence[bytes]) -> int:
        """emqx_packet:check/1 of a SUBSCRIBE (apps/emqx/src/emqx_packet.erl:265-273, 411-420):
        16#8F for an empty list or when validate/1 refuses any filter, else 0."""
        filters = list(filters)
        if not filters:
            return RC_TOPIC_FILTER_INVALID
        return RC_TOPIC_FILTER_INVALID if (self.records(FILTER, filters)[:, 0] & 0xFF).any() else 0
