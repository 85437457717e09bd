"""emqx_shared_sub restated on plain Python (apps/emqx/src/emqx_shared_sub.erl): the membership
bag, the per-group strategy, the round_robin_per_group counters and pick/6 for a first dispatch
(FailedSubs = #{}).  The reference of tests/test_share_ref_cpu.py, tests/test_share_dev_host.py and
tests/test_gpu_share.py; it shares no code with the library.

Where the reference draws (rand:uniform(Count)) the request's ``draw`` names the member,
``1 + draw rem Count``: any member is a valid outcome there, this one can be pinned.  ``hc`` and
``ht`` stand for erlang:phash2(ClientId) and erlang:phash2(SourceTopic), which the caller computes.
An answer is the four words of emqxgm_share_pick: (member | NONE, status, state out, Count)."""

NONE = 0xFFFFFFFF
STRATEGIES = ("random", "round_robin", "round_robin_per_group", "sticky", "local", "hash_clientid", "hash_topic")
RANDOM, ROUND_ROBIN, RR_PER_GROUP, STICKY, LOCAL, HASH_CLIENTID, HASH_TOPIC = range(7)
PICKED, NO_SUBSCRIBERS, HOST_STRATEGY = 0, 1, 2
DEVICE_DECIDED = (RANDOM, ROUND_ROBIN, LOCAL, HASH_CLIENTID, HASH_TOPIC)


def do_pick_subscriber(strategy, hc, ht, draw, state, counters, key, count):
    """do_pick_subscriber/6 (:359-379) -> (Nth, state out)."""
    if strategy == RANDOM:  # :359-360
        return 1 + draw % count, state
    if strategy == HASH_CLIENTID:  # :361-362
        return 1 + hc % count, state
    if strategy == HASH_TOPIC:  # :363-364
        return 1 + ht % count, state
    if strategy == ROUND_ROBIN:  # :365-372
        rem = draw % count if state == NONE else (state + 1) % count
        return rem + 1, rem
    if strategy == RR_PER_GROUP:  # :373-379: ets:update_counter(Key, {2, 1, Count, 1}, {Key, 0})
        c = counters.get(key, 0) + 1
        if c > count:
            c = 1
        counters[key] = c
        return c, state
    raise ValueError(strategy)


def pick_subscriber(strategy, hc, ht, draw, state, counters, key, subs):
    """pick_subscriber/6 (:346-357) over subs = [(sub, local)] -> (sub, state out)."""
    if len(subs) == 1:  # :346-347, before any strategy
        return subs[0][0], state
    if strategy == LOCAL:  # :348-354
        local = [s for s in subs if s[1]]
        return pick_subscriber(RANDOM, hc, ht, draw, state, counters, key, local or subs)
    nth, state = do_pick_subscriber(strategy, hc, ht, draw, state, counters, key, len(subs))
    return subs[nth - 1][0], state  # lists:nth(Nth, Subs)


class SharedSubRef:
    def __init__(self):
        self.bag = {}  # (group, topic) -> [(sub, local)] in insertion order; absent when empty
        self.group_strategy = {}
        self.default = ROUND_ROBIN  # emqx_schema.erl: shared_subscription_strategy
        self.counters = {}  # ?SHARED_SUBS_ROUND_ROBIN_COUNTER
        self.pending = []

    # -- mutations: pending, in call order, until commit ------------------------------------
    def subscribe(self, group, topic, sub, local):
        self.pending.append(("S", group, bytes(topic), sub, bool(local)))

    def unsubscribe(self, group, topic, sub):
        self.pending.append(("U", group, bytes(topic), sub))

    def subscriber_down(self, sub):
        self.pending.append(("D", sub))

    def set_strategy(self, group, strategy):
        self.pending.append(("G", group, strategy))

    def strategy(self, group):
        """strategy/1 (:159-164)"""
        return self.group_strategy.get(group, self.default)

    def _remove(self, key, sub):
        subs = self.bag.get(key, [])
        left = [s for s in subs if s[0] != sub]
        if left:
            self.bag[key] = left
        else:
            self.bag.pop(key, None)
        # maybe_delete_round_robin_count/1 (:489-494)
        if self.strategy(key[0]) == RR_PER_GROUP and key not in self.bag:
            self.counters.pop(key, None)

    def commit(self):
        for op in self.pending:
            if op[0] == "S":  # handle_call({subscribe, ..}) (:416-425); the table is a bag
                key = (op[1], op[2])
                subs = self.bag.setdefault(key, [])
                if all(s[0] != op[3] for s in subs):
                    subs.append((op[3], op[4]))
                if self.strategy(op[1]) == RR_PER_GROUP:  # maybe_insert_round_robin_count/1 (:484-487)
                    self.counters[key] = 0
            elif op[0] == "U":  # handle_call({unsubscribe, ..}) (:426-431)
                self._remove((op[1], op[2]), op[3])
            elif op[0] == "D":  # cleanup_down/1 (:509-519)
                for key in [k for k, subs in self.bag.items() if any(s[0] == op[1] for s in subs)]:
                    self._remove(key, op[1])
            else:
                if op[1] is None:
                    self.default = op[2]
                else:
                    self.group_strategy[op[1]] = op[2]
        self.pending = []

    # -- reads --------------------------------------------------------------------------------
    def subscribers(self, group, topic):
        """subscribers/2 (:391-392)"""
        return list(self.bag.get((group, bytes(topic)), []))

    def counter(self, group, topic):
        return self.counters.get((group, bytes(topic)))

    def pick(self, group, topic, hc, ht, draw, state):
        """pick/6 (:309-344) with FailedSubs = #{} -> (member | NONE, status, state out, Count)."""
        key = (group, bytes(topic))
        subs = self.bag.get(key, [])
        if not subs:  # do_pick([], ..) -> false (:334-335)
            return (NONE, NO_SUBSCRIBERS, state, 0)
        strategy = self.strategy(group)
        if strategy == STICKY:  # :309-329: is_active_sub/3 is the caller's to answer
            return (NONE, HOST_STRATEGY, state, len(subs))
        sub, state = pick_subscriber(strategy, hc, ht, draw, state, self.counters, key, subs)
        return (sub, PICKED, state, len(subs))

    def dispatch_batch(self, requests):
        return [self.pick(*r) for r in requests]
