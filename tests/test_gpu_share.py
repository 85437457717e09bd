"""GPU parity of shared subscriptions (emqx_amd.SharedSub over emqxgm_share_*, k_share, the mirror
emqx_amd.SharedSubs and Broker.publish_shared_batch; DESIGN.md 6b "Shared subscriptions") against
the reference semantics of tests/share_ref.py, on the scripts of tests/share_cases.py -- the same
ones the CPU gate (tests/test_share_dev_host.py) runs the kernel's phases and the host code on
under ASan + UBSan: member, status, round_robin state and Count per request."""
import random

import pytest

import share_cases as SC
import share_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _refused(emqx):
    """The refused calls: each raises (-EINVAL) and leaves the table and what is pending alone."""
    E = emqx.EngineError
    big = 1 << 31

    def run(s):
        for call in (lambda: s.subscribe(1, b"r/t", big, True), lambda: s.subscribe(big, b"r/t", 1, True),
                     lambda: s.unsubscribe(1, b"r/t", big), lambda: s.subscriber_down(SC.NONE),
                     lambda: s.set_strategy(1, 7), lambda: s.set_strategy(big, 1),
                     lambda: s.pick([big], [b"r/t"], [0], [0], [0], [0]),
                     lambda: s.tune("no_such_key", 1), lambda: s.tune("rebuild_load_pct", 51),
                     lambda: s.tune("rebuild_garbage_pct", 0), lambda: s.tune("pass_names", 0)):
            with pytest.raises(E):
                call()
        pending = s.stats()["pending"]
        g = 0x7FFFFFF0
        s.subscribe(g, b"r/t", 5, True)
        with pytest.raises(E):
            s.subscribe(g, b"r/t", 5, False)  # the other local flag
        s.subscribe(g, b"r/t", 5, True)
        s.unsubscribe(g, b"r/t", 5)
        s.subscribe(g, b"r/t", 5, False)
        s.unsubscribe(g, b"r/t", 5)
        assert s.stats()["pending"] == pending + 5
        with pytest.raises(E):
            emqx.SharedSub(0, 17)
    return run


@pytest.fixture
def play(emqx):
    def run(script, hash_bits=0, pass_names=0):
        return SC.run_lib(emqx.SharedSub, _refused(emqx), script, hash_bits, pass_names)
    return run


def test_strategies_sizes_and_edges(play):
    SC.check_strategies(play)


@pytest.mark.parametrize("stage", [False, True])
@pytest.mark.parametrize("hash_bits", [0, 4])
def test_topic_lengths_and_key_identity(play, hash_bits, stage):
    SC.check_topics(play, hash_bits, stage)


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_mutations(play, hash_bits):
    SC.check_mutations(play, hash_bits)


@pytest.mark.parametrize("split", [False, True])
def test_round_robin_per_group_golden(play, split):
    SC.check_golden_rr(play, split)


def test_round_robin_per_group_counters(play):
    SC.check_counters(play)


@pytest.mark.parametrize("n", SC.BATCH_SIZES)
def test_block_edges(play, n):
    SC.check_block(play, n)


@pytest.mark.parametrize("stage", [False, True])
@pytest.mark.parametrize("hash_bits", [0, 4])
def test_random_case(play, hash_bits, stage):
    SC.check_random(play, hash_bits, stage=stage)


def test_fourteen_passes_against_one(play):
    assert SC.check_random(play, 0, 287) == SC.check_random(play, 0)


def test_growth_and_garbage_rebuild(play):
    SC.check_big(play)


def test_refused_calls(play):
    SC.check_refused(play)


def test_mirror_names(emqx):
    """emqx_amd.SharedSubs: the reference's names over terms."""
    s = emqx.SharedSubs(node="n1")
    try:
        assert s.strategy(b"g") == "round_robin"
        s.set_strategy(b"g", "hash_clientid")
        s.set_strategy(b"st", "sticky")
        for sub, node in (("c1", None), ("c2", "n2"), ("c3", "n1")):
            assert s.subscribe(b"g", b"t/1", sub, node) == "ok"
        s.subscribe(b"st", b"t/1", "c9")
        assert s.subscribers(b"g", b"t/1") == ["c1", "c2", "c3"] and s.strategy(b"g") == "hash_clientid"
        got = s.dispatch_batch([(b"g", b"t/1", 4, 0, 0, None), (b"g", b"t/2", 4, 0, 0, 7),
                                (b"st", b"t/1", 0, 0, 0, None)])
        assert got == [("picked", "c2", None, 3), ("no_subscribers", None, 7, 0), ("host_strategy", None, None, 1)]
        s.unsubscribe(b"g", b"t/1", "c1")
        s.subscribe(b"g", b"t/1", "c1")
        s.subscriber_down("c3")
        assert s.subscribers(b"g", b"t/1") == ["c2", "c1"]
        s.set_strategy(b"g", "local")
        assert s.dispatch_batch([(b"g", b"t/1", 0, 0, 0, None)]) == [("picked", "c1", None, 2)]
    finally:
        s.close()


def test_publish_shared_batch(emqx):
    """Broker.publish_shared_batch against oracle.emqx_ref.publish plus share_ref: a small route
    table with three groups, one strategy each."""
    from oracle import emqx_ref as R
    rng = random.Random(5)
    b = emqx.Broker(node="n1")
    rt, ref = R.Router(), SR.SharedSubRef()
    groups = {b"ga": SR.HASH_CLIENTID, b"gb": SR.ROUND_ROBIN, b"gc": SR.RR_PER_GROUP}
    gid = {g: i for i, g in enumerate(groups)}
    filters = [b"s/+/x", b"s/#", b"s/1/x", b"other"]
    subs = {}
    for g, strat in groups.items():
        b.shared.set_strategy(g, emqx.shared_sub.SHARE_STRATEGIES[strat])
        ref.set_strategy(gid[g], strat)
    sub = 0
    for f in filters:
        b.subscribe(f, "plain-%s" % f.decode())
        rt.add_route(f, "n1")
        subs[f] = ["plain-%s" % f.decode()]
        for g in groups:
            if rng.random() < 0.8:
                b.add_route(f, (g, "n1"))
                rt.add_route(f, (g, "n1"))
                for _ in range(rng.randrange(1, 4)):
                    sub += 1
                    b.shared.subscribe(g, f, "m%d" % sub, None if sub % 2 else "n2")
                    ref.subscribe(gid[g], f, "m%d" % sub, sub % 2 == 1)
    ref.commit()
    topics = [b"s/1/x", b"s/2/x", b"s/1/y", b"other", b"none"] * 3
    msgs = [(rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32), {(b"gb", b"s/#"): 0}) for _ in topics]
    got = b.publish_shared_batch(topics, msgs)
    n_group_entries = 0
    for t, (hc, ht, draw, states), g in zip(topics, msgs, got):
        entries, _ = R.publish(rt, t, "n1", subs)
        want = []
        for to, dest in entries:
            if dest in groups:
                st = states.get((dest, to))
                m, status, so, count = ref.pick(gid[dest], to, hc, ht, draw, SR.NONE if st is None else st)
                want.append((to, dest, (emqx.shared_sub.STATUS[status], None if m == SR.NONE else m,
                                        None if so == SR.NONE else so, count)))
        # the reference's entries are a set (route/2); requests of one call on one key keep their order
        assert sorted(g) == sorted(want), (t, g, want)
        n_group_entries += len(want)
    assert n_group_entries > 20
    assert b.publish_batch(topics)[0][0]  # publish_batch itself answers as before
