"""The reference of the retainer backend's remaining callbacks, on top of the oracle's
emqx_retainer_mnesia restatement (oracle/emqx_ref.py Retainer, untouched): message timestamps,
the table-full rule of store_retained/2 (emqx_retainer_mnesia.erl:141, :409-419),
clear_expired/1 (:154-164), page_read/4 (:204-238) and match_messages/3 with
{Cursor, BatchNum} (:185-202, qlc_next_answers/2 :384-397)."""
from typing import Dict, List, Optional, Sequence, Tuple

from oracle import emqx_ref as R


def wkey(t: bytes):
    """Topic word order (a topic before the topics it prefixes)."""
    return tuple(t.split(b"/"))


class Retainer(R.Retainer):
    def __init__(self, index_specs: Sequence[Sequence[int]] = ()):
        super().__init__(index_specs)
        self.ts: Dict[tuple, int] = {}
        self.max_retained = 0

    def store_retained(self, topic: bytes, expiry: int = 0, ts: int = 0) -> bool:
        """:138-152: refused when is_table_full() andalso is_new_topic(Tokens).  table_size/0
        counts every stored message, expired but uncleared ones included."""
        toks = tuple(R.words(topic))
        if self.max_retained > 0 and len(self.msgs) >= self.max_retained and toks not in self.msgs:
            return False
        super().store_retained(topic, expiry)
        self.ts[toks] = ts
        return True

    def clear_expired(self, now: int) -> List[bytes]:
        """:154-164: ExpiryTime =/= 0 and ExpiryTime < NowMs (strictly)."""
        gone = [t for t, et in self.msgs.items() if et != 0 and et < now]
        for t in gone:
            self._delete(t)
        return [R.join(t) for t in gone]

    def page_read(self, topic: Optional[bytes], page: int, limit: int, now: int) -> List[bytes]:
        """:204-238.  qlc:sort with compare_message/2 (=<, :364-365) is stable over the table's
        own order, which ets does not define: among equal timestamps any order is right."""
        if topic is None:
            ms = R.retainer_condition(R.words(b"#"))  # search_table(undefined, ['#'], Now)
            rows = [R.join(t) for t, et in self.msgs.items()
                    if R.ets_match(ms, list(t)) and (et == 0 or et > now)]
        else:
            rows = self.search_table(R.words(topic), now)
        rows.sort(key=lambda t: self.ts[tuple(R.words(t))])
        skip = (page - 1) * limit
        if skip > 0:
            _, state = _next_answers(rows, 0, skip)
            if state == "closed":
                return []
        return _next_answers(rows, skip, limit)[0]

    def match_messages_cursor(self, topic: bytes, now: int, cursor, batch: int
                              ) -> Tuple[List[bytes], Optional[tuple]]:
        """:185-202 with batch_read_number = batch: cursor None opens a qlc cursor (here: the
        evaluated answers and a position); returns (rows, cursor or None when closed)."""
        if cursor is None:
            cursor = (self.search_table(R.words(topic), now), 0)
        rows, at = cursor
        got, state = _next_answers(rows, at, batch)
        return got, (None if state == "closed" else (rows, at + len(got)))


def _next_answers(rows, at, n):
    """qlc_next_answers/2 (:384-397): closed when fewer than N answers came."""
    got = rows[at:at + n]
    return got, ("closed" if len(got) < n else "more")
