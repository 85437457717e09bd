"""The retainer's mnesia backend on the device (apps/emqx_retainer/src/emqx_retainer_mnesia.erl),
SURVEY 8f rank 4: retained topics (messages stay with the caller) and the reverse match
``match_messages`` -- a subscription filter to the stored topics it selects -- in batches.

The selected set is ``search_table/3``'s (:300-330) with expiry 0 or > now and no '$' rule:
with index specs configured -- by default the reference's ``[[1,2,3],[1,3],[2,3],[3]]``
(emqx_retainer_schema.erl:24-29) -- the index path of the best-scoring index
(emqx_retainer_index.erl:83-91, 141-200: ``a/+`` also selects ``a/x/y`` under ``[1,2,3]``);
with ``index_specs=[]``, or when no index scores, the full scan of ``condition/1`` (:97-112:
'+' any one word, a last '#' any tail).  See DESIGN.md 6c.

    r = Retainer()
    r.store_retained(b"sensor/1/temp", expiry_ms=0)
    r.match_messages(b"sensor/+/temp", now_ms)   # -> [b"sensor/1/temp"]

The rest of the backend contract (emqx_retainer.erl:75-83): reads in parts through a cursor
(``match_messages_cursor`` / ``match_pages_batch``: match_messages/3 with {Cursor, BatchNum},
:185-202 -- only the window is computed into the output and downloaded), ``clear_expired``
(:154-164), ``page_read`` (:204-238, ordered by the message timestamp ``ts_ms``), the table-full
rule (``set_max_retained``, :141) and the wildcard ``delete_message`` (:171-179) in one call.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import List, Optional, Sequence

import numpy as np

from . import engine as E


def _now_ms() -> int:
    return int(time.time() * 1000)


DEFAULT_INDEX_SPECS = ((1, 2, 3), (1, 3), (2, 3), (3,))  # emqx_retainer_schema.erl:24-29

# cursor phases (include/emqx_gpumatch.h EMQXGM_RC_*); a cursor is (gen, phase, at), None = start
RC_START, RC_BASE, RC_DELTA, RC_DONE, RC_STALE = range(5)
ENOSPC = 28


class StaleCursor(E.EngineError):
    """The base store was rebuilt (or cleaned) under a cursor: restart that filter."""


class _Cursor(C.Structure):
    _fields_ = [("gen", C.c_uint64), ("phase", C.c_uint32), ("at", C.c_uint32)]


class Retainer:
    def __init__(self, device: int = 0, index_specs: Sequence[Sequence[int]] = DEFAULT_INDEX_SPECS):
        self._lib = E.lib()
        h = C.c_void_p()
        rc = self._lib.emqxgm_retain_create(device, C.byref(h))
        if rc != 0:
            raise E.EngineError(f"emqxgm_retain_create failed: {rc}")
        self._h = h
        self._dirty = False
        self.set_index_specs(index_specs)

    def set_index_specs(self, specs: Sequence[Sequence[int]]) -> None:
        """retainer.backend.index_specs (config_indices/0); [] = the full scan only."""
        pos = np.array([p for s in specs for p in s], np.uint32)
        off = np.zeros(len(specs) + 1, np.uint32)
        np.cumsum([len(s) for s in specs], out=off[1:])
        self._check(self._lib.emqxgm_retain_set_indices(self._h, E._ptr(pos), E._ptr(off),
                                                        len(specs)), "retain_set_indices")

    def close(self):
        if self._h:
            self._lib.emqxgm_retain_destroy(self._h)
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

    # ---- emqx_retainer_mnesia API ----
    def store_retained(self, topic: bytes, expiry_ms: int = 0, ts_ms: int = 0) -> Optional[int]:
        """:138-152; None when the table is full and the topic is new (set_max_retained)."""
        i = C.c_uint32()
        rc = self._lib.emqxgm_retain_store_ts(self._h, topic, len(topic), expiry_ms, ts_ms,
                                              C.byref(i))
        if rc == -ENOSPC:
            return None
        self._check(rc, "retain_store")
        self._dirty = True
        return i.value

    def set_max_retained(self, limit: int) -> None:
        """retainer.backend.max_retained_messages (is_table_full/0, :409-411); 0 = no limit."""
        self.tune("max_retained_messages", limit)

    def delete_message(self, topic: bytes) -> None:
        """:166-180: a wildcard deletes every stored topic it selects (Now = 0)."""
        if _wild(topic):
            p, n = E._U32P(), C.c_uint64()
            self._check(self._lib.emqxgm_retain_delete_matching(
                self._h, topic, len(topic), C.byref(p), C.byref(n)), "retain_delete_matching")
            self._dirty = False  # (it commits)
        else:
            self._check(self._lib.emqxgm_retain_delete(self._h, topic, len(topic)),
                        "retain_delete")
            self._dirty = True

    def _id_topics(self, p, n) -> List[bytes]:
        ids = [p[k] for k in range(n.value)]  # valid until the next call: copy first
        return [self.topic(i) for i in ids]

    def clear_expired(self, now_ms: Optional[int] = None) -> List[bytes]:
        """clear_expired/1 (:154-164): the topics with expiry != 0 and < now leave the store;
        returns them (the caller deletes those messages from its own table)."""
        p, n = E._U32P(), C.c_uint64()
        self._check(self._lib.emqxgm_retain_clear_expired(
            self._h, _now_ms() if now_ms is None else now_ms, C.byref(p), C.byref(n)),
            "retain_clear_expired")
        self._dirty = False
        return self._id_topics(p, n)

    def page_read(self, topic: Optional[bytes], page: int, limit: int,
                  now_ms: Optional[int] = None) -> List[bytes]:
        """page_read/4 (:204-238): the selected topics ordered by timestamp, one page of them;
        topic None lists everything."""
        p, n = E._U32P(), C.c_uint64()
        self._check(self._lib.emqxgm_retain_page_read(
            self._h, topic, 0 if topic is None else len(topic), page, limit,
            _now_ms() if now_ms is None else now_ms, C.byref(p), C.byref(n)), "retain_page_read")
        self._dirty = False
        return self._id_topics(p, n)

    def clean(self) -> None:
        self._check(self._lib.emqxgm_retain_clean(self._h), "retain_clean")
        self._dirty = True

    def commit(self) -> None:
        if self._dirty:
            self._check(self._lib.emqxgm_retain_commit(self._h), "retain_commit")
            self._dirty = False

    def tune(self, key: str, value: int) -> None:
        self._check(self._lib.emqxgm_retain_tune(self._h, key.encode(), int(value)), "retain_tune")

    def stats(self) -> dict:
        a = (C.c_uint64 * 4)()
        self._check(self._lib.emqxgm_retain_stats(self._h, a), "retain_stats")
        return {"full_builds": a[0], "delta_commits": a[1], "base_topics": a[2],
                "delta_topics": a[3]}

    def timing(self) -> dict:
        """After tune("timing", 1): HIP-event ms of the last limited read's own launches."""
        a = (C.c_double * 3)()
        self._check(self._lib.emqxgm_retain_timing(self._h, a), "retain_timing")
        return {"count_ms": a[0], "window_ms": a[1], "fill_ms": a[2]}

    def size(self) -> int:
        self.commit()
        n = C.c_uint64()
        self._check(self._lib.emqxgm_retain_size(self._h, C.byref(n)), "retain_size")
        return n.value

    def topic(self, i: int) -> bytes:
        p, n = E._U8P(), C.c_uint32()
        self._check(self._lib.emqxgm_retain_topic(self._h, i, C.byref(p), C.byref(n)),
                    "retain_topic")
        return C.string_at(p, n.value)

    def read_message(self, topic: bytes, now_ms: Optional[int] = None) -> List[bytes]:
        """:182-183 / read_messages/1 :372-382 (expiry 0 or >= now)."""
        self.commit()
        i = C.c_uint32()
        rc = self._check(self._lib.emqxgm_retain_read(
            self._h, topic, len(topic), _now_ms() if now_ms is None else now_ms, C.byref(i)),
            "retain_read")
        return [topic] if rc == 1 else []

    def match_ids(self, filters: Sequence[bytes], now_ms: Optional[int] = None):
        """One device pass: (ptr[n+1] u64, ids u32) -- filter i selects ids[ptr[i]:ptr[i+1]]."""
        self.commit()
        buf, off = E.pack(list(filters), np.uint32)
        out = E._RetOut()
        self._check(self._lib.emqxgm_retain_match(
            self._h, E._ptr(buf), E._ptr(off), len(filters),
            _now_ms() if now_ms is None else now_ms, C.byref(out)), "retain_match")
        n = len(filters)
        ptr = np.ctypeslib.as_array(out.ptr, shape=(n + 1,)).copy()
        ids = (np.ctypeslib.as_array(out.id, shape=(out.n_ids,)).copy() if out.n_ids
               else np.zeros(0, np.uint32))
        return ptr, ids

    def match_messages_batch(self, filters: Sequence[bytes],
                             now_ms: Optional[int] = None) -> List[List[bytes]]:
        ptr, ids = self.match_ids(filters, now_ms)
        return [[self.topic(int(i)) for i in ids[ptr[k]:ptr[k + 1]]] for k in range(len(filters))]

    def match_messages(self, topic: bytes, now_ms: Optional[int] = None) -> List[bytes]:
        """:185-195 (all remaining answers at once)."""
        return self.match_messages_batch([topic], now_ms)[0]

    def match_pages_ids(self, filters: Sequence[bytes], limits: Sequence[int], cursors,
                        now_ms: Optional[int] = None):
        """One device pass of limited reads: (ptr, ids, cursors) -- filter i's next limits[i]
        live ids (0: all) at or after cursors[i] ((gen, phase, at), None = start)."""
        self.commit()
        n = len(filters)
        assert len(limits) == n and len(cursors) == n
        buf, off = E.pack(list(filters), np.uint32)
        lim = np.asarray(limits, np.uint32)
        cur = (_Cursor * max(n, 1))()
        for k, c in enumerate(cursors):
            if c is not None:
                cur[k].gen, cur[k].phase, cur[k].at = c
        out = E._RetOut()
        self._check(self._lib.emqxgm_retain_match_limit(
            self._h, E._ptr(buf), E._ptr(off), n, _now_ms() if now_ms is None else now_ms,
            E._ptr(lim), C.cast(cur, C.c_void_p), C.byref(out)), "retain_match_limit")
        ptr = np.ctypeslib.as_array(out.ptr, shape=(n + 1,)).copy()
        ids = (np.ctypeslib.as_array(out.id, shape=(out.n_ids,)).copy() if out.n_ids
               else np.zeros(0, np.uint32))
        return ptr, ids, [(cur[k].gen, cur[k].phase, cur[k].at) for k in range(n)]

    def match_pages_batch(self, filters: Sequence[bytes], limits: Sequence[int], cursors,
                          now_ms: Optional[int] = None):
        """-> (rows, cursors): a page of each filter and where to go on.  A cursor's phase is
        RC_DONE when nothing remains after its page, RC_STALE when the base store was rebuilt
        under it (the row is empty: restart that filter with None)."""
        ptr, ids, cur = self.match_pages_ids(filters, limits, cursors, now_ms)
        return [[self.topic(int(i)) for i in ids[ptr[k]:ptr[k + 1]]]
                for k in range(len(filters))], cur

    def match_messages_cursor(self, topic: bytes, cursor, batch_read_number: int,
                              now_ms: Optional[int] = None):
        """match_messages/3 with {Cursor, BatchNum} (:185-202): -> (rows, cursor or None).
        None comes with the last rows -- one call earlier than qlc_next_answers/2 closes when
        exactly batch_read_number answers remain; the rows are the same.  StaleCursor when the
        base store was rebuilt under the cursor."""
        rows, cur = self.match_pages_batch([topic], [batch_read_number], [cursor], now_ms)
        if cur[0][1] == RC_STALE:
            raise StaleCursor("the retained store was rebuilt under this cursor")
        return rows[0], (None if cur[0][1] == RC_DONE else cur[0])


def _wild(topic: bytes) -> bool:
    return any(w in (b"+", b"#") for w in topic.split(b"/"))
