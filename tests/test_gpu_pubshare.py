"""GPU parity of the pick inside the publish (emqxgm_publish_shared_batch, k_pubshare; DESIGN.md 6b
"The pick inside the publish") through emqx_amd.Engine.publish_shared and
Broker.publish_shared_batch, on the scripts of tests/pubshare_cases.py -- the same ones the CPU
gate (tests/test_pubshare_dev_host.py) runs the kernel's phases on under ASan + UBSan.  Every
entry's (To, dest, member, status, round_robin state, Count) is compared exactly with
oracle.emqx_ref.publish's entries picked by tests/share_ref.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import pubshare_cases as PC
import share_cases as SC
import share_ref as SR

pytestmark = pytest.mark.gpu
NODES = {"n1": 0, "n2": 1}
NODE_NAMES = {v: k for k, v in NODES.items()}


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def _states_for(eng, msgs):
    """The call's state lists in the C-ABI's terms; None when no message carries one."""
    if all(m[3] is None for m in msgs):
        return None
    out = []
    for m in msgs:
        row = []
        for (g, to), v in m[3] or ():
            f = eng.lookup_id(to)
            if f is not None:  # a To that is no filter is dropped
                row.append((g, f, v))
        out.append(row)
    return out


@pytest.fixture
def play(emqx):
    """The script on emqx_amd.Engine and emqx_amd.SharedSub, the C-ABI as it is."""
    def run(script, hash_bits=0, batch_max=0, also_plain=False):
        eng, share, out = emqx.Engine(batch_max=batch_max), emqx.SharedSub(0, hash_bits), []
        eng.set_local_node(NODES[PC.LOCAL_NODE])
        try:
            for op in script:
                k = op[0]
                if k == "G":
                    share.set_strategy(op[1], op[2])
                elif k == "S":
                    share.subscribe(*op[1:])
                elif k == "U":
                    share.unsubscribe(*op[1:])
                elif k == "C":
                    share.commit()
                elif k in ("RA", "RD"):
                    node, group = (NODES[op[2]], emqx.NONE) if isinstance(op[2], str) else (NODES[PC.LOCAL_NODE], op[2])
                    (eng.route_add if k == "RA" else eng.route_delete)(op[1], node, group)
                elif k == "RC":
                    eng.commit()
                elif k == "P":
                    topics, msgs = op[1], op[2]
                    res = eng.publish_shared(topics, share, [m[0] for m in msgs], [m[1] for m in msgs],
                                             [m[2] for m in msgs], _states_for(eng, msgs))
                    if also_plain:  # pub of the new entry is emqxgm_publish_batch's answer
                        plain = eng.publish(topics)
                        for name in ("route_ptr", "route_filter", "route_dest", "deliver_ptr", "deliver_filter", "deliver_sub"):
                            assert np.array_equal(getattr(res, name), getattr(plain, name)), name
                        assert res.share.shape == (len(plain.route_filter), 4)
                    rows = []
                    for i in range(len(topics)):
                        rows.append([(eng.filter_bytes(f), d & 0x7FFFFFFF if d & emqx.engine.DEST_GROUP else NODE_NAMES[d], q)
                                     for (f, d), q in zip(res.routes(i), res.shares(i))])
                    out.append(rows)
        finally:
            share.close()
            eng.close()
        return out
    return run


def play_broker(emqx, script, fused=True):
    """The script on emqx_amd.Broker and its SharedSubs: the group entries only, as
    publish_shared_batch answers them, turned back into the reference's terms."""
    b, out = emqx.Broker(node=PC.LOCAL_NODE), []
    status = {s: i for i, s in enumerate(emqx.shared_sub.STATUS)}
    try:
        for op in script:
            k = op[0]
            if k == "G":
                b.shared.set_strategy(op[1], SR.STRATEGIES[op[2]])
            elif k == "S":
                b.shared.subscribe(op[1], op[2], op[3], None if op[4] else "n2")
            elif k == "U":
                b.shared.unsubscribe(*op[1:])
            elif k == "C":
                b.shared.commit()
            elif k in ("RA", "RD"):
                dest = op[2] if isinstance(op[2], str) else (op[2], PC.LOCAL_NODE)
                (b.add_route if k == "RA" else b.delete_route)(op[1], dest)
            elif k == "RC":
                b.commit()
            elif k == "P":
                msgs = []
                for hc, ht, draw, states in op[2]:
                    d = {}
                    for key, v in states or ():
                        d.setdefault(key, None if v == PC.NONE else v)  # the first pair wins
                    msgs.append((hc, ht, draw, d if states is not None else None))
                got = b.publish_shared_batch(op[1], msgs, fused=fused)
                out.append([[(to, g, (PC.NONE if m is None else m, status[st], PC.NONE if so is None else so, count))
                             for to, g, (st, m, so, count) in row] for row in got])
    finally:
        b.shared.close()
        b.engine.close()
    return out


def group_entries(result):
    return [[e for e in row if not isinstance(e[1], str)] for row in result]


@pytest.mark.parametrize("n", SC.BATCH_SIZES)
@pytest.mark.parametrize("layout", ["spread", "one", "gaps"])
def test_entry_counts(play, n, layout):
    PC.same_as_ref(play, PC.count_script(n, layout))


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_to_lengths_and_key_identity(play, hash_bits):
    PC.same_as_ref(play, PC.to_length_script(), hash_bits=hash_bits)


def test_strategies_sizes_and_edges(play):
    PC.same_as_ref(play, PC.strategy_script())


def test_state_lists(play):
    PC.same_as_ref(play, PC.state_script())


def test_round_robin_per_group_three_chunks_against_one(play):
    one, _ = PC.same_as_ref(play, PC.rr_group_script())
    three, _ = PC.same_as_ref(play, PC.rr_group_script(), batch_max=171)
    assert three == one


def test_mutations(play):
    PC.same_as_ref(play, PC.mutation_script())


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_random_case_and_pub_of_the_plain_entry(play, hash_bits):
    PC.same_as_ref(play, PC.random_script(), hash_bits=hash_bits, also_plain=True)


def test_random_case_in_chunks(play):
    PC.same_as_ref(play, PC.random_script(), batch_max=97, also_plain=True)


@pytest.mark.parametrize("name", ["random", "states", "rr_group", "strategies"])
def test_broker_fused(emqx, name):
    script = PC.ALL_SCRIPTS[name]()
    got, ref = play_broker(emqx, script), [group_entries(r) for r in PC.run_ref(script)]
    assert [PC.canon(g) for g in got] == [PC.canon(r) for r in ref]


def test_broker_fused_against_two_calls(emqx):
    script = PC.random_script()
    fused, two = play_broker(emqx, script, fused=True), play_broker(emqx, script, fused=False)
    assert [PC.canon(g) for g in fused] == [PC.canon(g) for g in two]
    assert sum(len(row) for row in fused[0]) > 1000


def test_refused_calls(emqx):
    """-EINVAL before anything is launched; both handles answer afterwards as before."""
    import torch
    script = PC.to_length_script()
    topics, msgs = script[-1][1], script[-1][2]
    eng, share = emqx.Engine(), emqx.SharedSub(0, 0)
    eng.set_local_node(0)
    try:
        for op in script[:-1]:
            if op[0] == "G":
                share.set_strategy(op[1], op[2])
            elif op[0] == "S":
                share.subscribe(*op[1:])
            elif op[0] == "RA":
                eng.route_add(op[1], 0, op[2])
        share.commit()
        eng.commit()
        args = ([m[0] for m in msgs], [m[1] for m in msgs], [m[2] for m in msgs])
        f0 = eng.lookup_id(topics[0])
        states = [[(1, f0, 0)] for _ in topics]
        before = eng.publish_shared(topics, share, *args, states)
        picks_before = share.pick([1], [topics[0]], [0], [0], [0], [PC.NONE])

        lib = emqx.engine.lib()
        buf, off = emqx.engine.pack(list(topics), np.uint32)
        n = len(topics)
        z = np.zeros(n, np.uint32)
        sp = np.arange(n + 1, dtype=np.uint32)
        sg, sf, sv = np.ones(n, np.uint32), np.full(n, f0, np.uint32), np.zeros(n, np.uint32)
        out = emqx.engine._PubSharedOut()

        def call(h=eng._h, s=share._h, off=off, sp=sp, sg=sg):
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            return lib.emqxgm_publish_shared_batch(h, s, p(buf), p(off), n, p(z), p(z), p(z), p(sp), p(sg), p(sf), p(sv),
                                                   C.byref(out))
        assert call() == 0
        assert call(h=None) == -errno.EINVAL and call(s=None) == -errno.EINVAL
        bad_off = off.copy()
        bad_off[3], bad_off[4] = off[4], off[3]
        assert call(off=bad_off) == -errno.EINVAL
        bad_sp = sp.copy()
        bad_sp[5] = 3
        assert call(sp=bad_sp) == -errno.EINVAL
        bad_sg = sg.copy()
        bad_sg[n - 1] = 1 << 31
        assert call(sg=bad_sg) == -errno.EINVAL
        if torch.cuda.device_count() > 1:  # handles on different devices
            other = emqx.SharedSub(1, 0)
            try:
                assert call(s=other._h) == -errno.EINVAL
            finally:
                other.close()

        after = eng.publish_shared(topics, share, *args, states)
        assert np.array_equal(after.share, before.share) and np.array_equal(after.route_dest, before.route_dest)
        assert len(before.share) > 40 and (before.share[:, 1] == SR.PICKED).all()
        assert np.array_equal(share.pick([1], [topics[0]], [0], [0], [0], [PC.NONE]), picks_before)
        assert eng.publish(topics).routes(0) == before.routes(0)
    finally:
        share.close()
        eng.close()
