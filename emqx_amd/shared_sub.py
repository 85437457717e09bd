"""``emqx_shared_sub`` on the MI355X engine (apps/emqx/src/emqx_shared_sub.erl), with the
reference's names: ``subscribe/3``, ``unsubscribe/3``, ``subscribers/2``, ``strategy/1`` and, for
``dispatch/3`` over a batch, ``dispatch_batch``.

The membership, the strategies and the pick run in the library (``emqxgm_share_*``, ``k_share``;
DESIGN.md 6b); this class only maps group and subscriber terms to the 32-bit handles and strategy
names to their codes.  ``hc`` and ``ht`` of a request are ``erlang:phash2(ClientId)`` and
``erlang:phash2(SourceTopic)``, computed by the caller; ``draw`` is 32 random bits; ``state`` is
the publisher's ``round_robin`` state for the key or ``None``.  A ``sticky`` group answers
``"host_strategy"``: the stuck member's liveness is the caller's, who picks from
``subscribers/2``.  Redispatch after a nack and the ack protocol stay with the caller.
"""
from __future__ import annotations

from typing import Hashable, List, Optional, Sequence, Tuple

from .engine import NONE, SHARE_STRATEGIES, SharedSub

STATUS = ("picked", "no_subscribers", "host_strategy")


class _Names:
    def __init__(self):
        self.ids, self.names = {}, []

    def id(self, name: Hashable) -> int:
        i = self.ids.get(name)
        if i is None:
            i = self.ids[name] = len(self.names)
            self.names.append(name)
        return i


class SharedSubs:
    def __init__(self, node: str = "node@local", device: int = 0, hash_bits: int = 0, groups=None):
        self.node = node
        self.table = SharedSub(device, hash_bits)
        self._groups = groups if groups is not None else _Names()
        self._subs = _Names()
        self._strategy = {}
        self._default = "round_robin"
        self._dirty = False

    def close(self) -> None:
        self.table.close()

    # ---- membership ----
    def subscribe(self, group: Hashable, topic: bytes, sub: Hashable, node: Optional[str] = None) -> str:
        """subscribe/3; ``node``: where the subscriber lives (default: this node)."""
        self.table.subscribe(self._groups.id(group), topic, self._subs.id(sub), node is None or node == self.node)
        self._dirty = True
        return "ok"

    def unsubscribe(self, group: Hashable, topic: bytes, sub: Hashable) -> str:
        self.table.unsubscribe(self._groups.id(group), topic, self._subs.id(sub))
        self._dirty = True
        return "ok"

    def subscriber_down(self, sub: Hashable) -> None:
        """cleanup_down/1"""
        self.table.subscriber_down(self._subs.id(sub))
        self._dirty = True

    def set_strategy(self, group: Optional[Hashable], strategy: str) -> None:
        """The group's strategy; ``group`` None: broker.shared_subscription_strategy."""
        self.table.set_strategy(None if group is None else self._groups.id(group), strategy)
        if group is None:
            self._default = strategy
        else:
            self._strategy[group] = strategy
        self._dirty = True

    def commit(self) -> None:
        if self._dirty:
            self.table.commit()
            self._dirty = False

    # ---- reads ----
    def strategy(self, group: Hashable) -> str:
        """strategy/1, as set (visible to picks after the commit)."""
        return self._strategy.get(group, self._default)

    def subscribers(self, group: Hashable, topic: bytes) -> List[Hashable]:
        """subscribers/2: the committed members in subscribe order."""
        self.commit()
        return [self._subs.names[h] for h, _ in self.table.members(self._groups.id(group), topic)]

    def dispatch_batch(self, requests: Sequence[Tuple]) -> List[Tuple]:
        """requests: (group, topic, hc, ht, draw, state | None) ->
        [(status, member | None, state out | None, Count)] with status in STATUS."""
        self.commit()
        requests = list(requests)
        out = self.table.pick([self._groups.id(r[0]) for r in requests], [r[1] for r in requests],
                              [r[2] for r in requests], [r[3] for r in requests], [r[4] for r in requests],
                              [NONE if r[5] is None else r[5] for r in requests])
        return [(STATUS[int(st)], None if int(m) == NONE else self._subs.names[int(m)],
                 None if int(state) == NONE else int(state), int(count)) for m, st, state, count in out]


__all__ = ["SharedSubs", "STATUS", "SHARE_STRATEGIES"]
