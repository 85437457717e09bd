"""The pick inside the publish (emqxgm_publish_shared_batch, k_pubshare; DESIGN.md 6b "The pick
inside the publish") against the two-call sequence it replaces, on one index and one batch: a
cfg3-shaped index of --filters filters, every one with a route to another node and --group-share of
them also with a route of one of 8 groups (1..8 members per key, the device-decided strategies and
round_robin_per_group), --topics cfg3 topics.

  fused     emqxgm_publish_shared_batch: best-of---reps wall time of the C-ABI call, the kernel time
            of k_pubshare per call by HIP events, the entries and the bytes copied back for them
  two_call  emqxgm_publish_batch, the requests packed on the host (numpy gathers over the filter
            bytes by id, fetched once before the clock starts), emqxgm_share_pick: best-of---reps
            wall time of the sequence and of its three parts

--tree PATH runs the two-call sequence on the library of another checkout (the parent commit's,
built there), for the A/B of MEASUREMENTS.md r18.  One JSON line.

  python tools/pubshare_bench.py [--filters 200000] [--topics 1000000] [--group-share 0.25]
                                 [--reps 3] [--mode both|fused|two_call] [--tree PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

STRATS = ("random", "round_robin", "local", "hash_clientid", "hash_topic", "random", "round_robin",
          "round_robin_per_group")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=200_000)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--group-share", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", default="both", choices=("both", "fused", "two_call"))
    ap.add_argument("--tree", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import workloads
    from emqx_amd import Engine, SharedSub
    from emqx_amd.engine import DEST_GROUP, NONE, _PubOut, _ptr, lib
    L = lib()
    rng = np.random.default_rng(18)
    w = workloads.generate(3, args.filters, args.topics)
    eng, share = Engine(), SharedSub()
    eng.set_local_node(0)
    for g, s in enumerate(STRATS):
        share.set_strategy(g, s)
    grouped = rng.random(w.nf) < args.group_share
    sub = members = 0
    for i in range(w.nf):
        f = w.filter(i)
        L.emqxgm_route_add(eng._h, f, len(f), 1, NONE)
        if grouped[i]:
            g = i % len(STRATS)
            L.emqxgm_route_add(eng._h, f, len(f), 0, g)
            for _ in range(1 + i % 8):
                L.emqxgm_share_subscribe(share._h, g, f, len(f), sub & 0x7FFFFFFF, sub & 1)
                sub += 1
                members += 1
    eng.commit()
    share.commit()
    n = w.nt
    tb, to = np.ascontiguousarray(w.tbytes), np.ascontiguousarray(w.toff, dtype=np.uint32)
    hc, ht, dr = (rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    res = {"filters": int(w.nf), "group_routed_filters": int(grouped.sum()), "members": members, "topics": int(n),
           "tree": root}

    if args.mode in ("both", "fused"):
        from emqx_amd.engine import _PubSharedOut
        o = _PubSharedOut()

        def fused():
            rc = L.emqxgm_publish_shared_batch(eng._h, share._h, p(tb), p(to), n, p(hc), p(ht), p(dr), None, None, None,
                                               None, C.byref(o))
            assert rc == 0, rc
        fused()
        share.tune("timing", 1)
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fused()
            walls.append(time.perf_counter() - t0)
        nr = int(o.pub.n_routes)
        q = np.ctypeslib.as_array(o.share, shape=(nr, 4))
        res["fused"] = {"wall_ms": [round(t * 1e3, 2) for t in walls], "best_ms": round(min(walls) * 1e3, 2),
                        "k_pubshare_ms_per_call": round(share.kernel_time_us() / 1000 / args.reps, 4),
                        "entries": nr, "group_entries": int((q[:, 1] != 5).sum()),
                        "picked": int((q[:, 1] == 0).sum()), "share_bytes_copied_back": nr * 16,
                        "bytes_per_entry": 16}
        share.tune("timing", 0)

    if args.mode in ("both", "two_call"):
        # the filter bytes by id, as a caller's own table of its filters would have them
        ids = np.array([eng.lookup_id(w.filter(i)) for i in range(w.nf)], np.int64)
        flen = np.zeros(int(ids.max()) + 1, np.int64)
        fsrc = np.zeros(int(ids.max()) + 1, np.int64)
        flen[ids] = (w.foff[1:] - w.foff[:-1]).astype(np.int64)
        fsrc[ids] = w.foff[:-1].astype(np.int64)
        o = _PubOut()
        parts = []

        def two_call():
            t0 = time.perf_counter()
            rc = L.emqxgm_publish_batch(eng._h, p(tb), p(to), n, C.byref(o))
            assert rc == 0, rc
            t1 = time.perf_counter()
            nr = int(o.n_routes)
            rp = np.ctypeslib.as_array(o.route_ptr, shape=(n + 1,))
            rf = np.ctypeslib.as_array(o.route_filter, shape=(nr,))
            rd = np.ctypeslib.as_array(o.route_dest, shape=(nr,))
            sel = np.nonzero(rd & DEST_GROUP)[0]
            owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp).astype(np.int64))[sel]
            f = rf[sel].astype(np.int64)
            groups = (rd[sel] & 0x7FFFFFFF).astype(np.uint32)
            ko = np.zeros(len(sel) + 1, np.uint32)
            np.cumsum(flen[f], out=ko[1:])
            kb = w.fbytes[np.repeat(fsrc[f] - ko[:-1].astype(np.int64), flen[f]) + np.arange(int(ko[-1]), dtype=np.int64)]
            rhc, rht, rdr = hc[owner], ht[owner], dr[owner]
            state = np.full(len(sel), NONE, np.uint32)
            out = np.empty((len(sel), 4), np.uint32)
            t2 = time.perf_counter()
            rc = L.emqxgm_share_pick(share._h, len(sel), p(groups), p(kb), p(ko), p(rhc), p(rht), p(rdr), p(state), p(out))
            assert rc == 0, rc
            t3 = time.perf_counter()
            parts.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0, len(sel), int((out[:, 1] == 0).sum())))
        two_call()
        parts.clear()
        share.tune("timing", 1)
        for _ in range(args.reps):
            two_call()
        best = min(parts, key=lambda r: r[3])
        res["two_call"] = {"wall_ms": [round(r[3] * 1e3, 2) for r in parts], "best_ms": round(best[3] * 1e3, 2),
                           "best_publish_ms": round(best[0] * 1e3, 2), "best_host_pack_ms": round(best[1] * 1e3, 2),
                           "best_share_pick_ms": round(best[2] * 1e3, 2),
                           "k_share_ms_per_call": round(share.kernel_time_us() / 1000 / args.reps, 4),
                           "group_entries": best[4], "picked": best[5]}
    print(json.dumps(res), flush=True)
    share.close()
    eng.close()


if __name__ == "__main__":
    main()
