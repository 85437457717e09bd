"""Shared subscriptions on the device (emqxgm_share_pick, k_share; DESIGN.md 6b "Shared
subscriptions"): --requests requests spread over --keys keys of 1..64 members, once per
device-decided strategy, with the block's topics hashed from global memory and staged through LDS
("stage_lds").  Per run: the kernel time per pass by HIP events and the end-to-end rate of
SharedSub.pick (packing in Python included), best of --reps.  One JSON line.

  python tools/share_bench.py [--requests 1000000] [--keys 16384,1000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEVICE_DECIDED = ("random", "round_robin", "local", "hash_clientid", "hash_topic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1_000_000)
    ap.add_argument("--keys", default="16384,1000000")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import ctypes as C

    import numpy as np
    from emqx_amd import SharedSub
    from emqx_amd.engine import NONE, SHARE_STRATEGIES, _ptr, lib, pack
    rng = np.random.default_rng(16)
    n = args.requests
    res = {"requests": n}
    for nk in [int(k) for k in args.keys.split(",") if k]:
        s = SharedSub()
        topics = [b"site/%d/device/%d/shared" % (k % 997, k) for k in range(nk)]
        sizes = rng.integers(1, 65, nk)
        t0 = time.perf_counter()
        L = lib()
        sub = 0
        for k in range(nk):
            t = topics[k]
            for _ in range(int(sizes[k])):
                L.emqxgm_share_subscribe(s._h, 1, t, len(t), sub & 0x7FFFFFFF, sub & 1)
                sub += 1
        s.commit()
        load = time.perf_counter() - t0
        pick = rng.integers(0, nk, n)
        req = [topics[i] for i in pick]
        buf, off = pack(req, np.uint32)
        arrs = [np.ones(n, np.uint32)] + [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(3)]
        state = np.where(rng.random(n) < 0.5, NONE, rng.integers(0, 64, n)).astype(np.uint32)
        out = np.zeros((n, 4), np.uint32)
        passes = -(-n // (1 << 20))

        def call():
            rc = L.emqxgm_share_pick(s._h, n, _ptr(arrs[0]), _ptr(buf), off.ctypes.data_as(C.c_void_p), _ptr(arrs[1]),
                                     _ptr(arrs[2]), _ptr(arrs[3]), _ptr(state), _ptr(out))
            assert rc == 0, rc
        r = {"members": int(sizes.sum()), "load_s": round(load, 2), "stats": s.stats()}
        for strat in DEVICE_DECIDED:
            s.set_strategy(1, strat)
            s.commit()
            for stage in (0, 1):
                s.tune("stage_lds", stage)
                call()
                s.tune("timing", 1)
                best = 1e9
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    call()
                    best = min(best, time.perf_counter() - t0)
                assert (out[:, 1] == 0).all() and (out[:, 3] == sizes[pick]).all()
                r["%s_%s" % (strat, "lds" if stage else "global")] = {
                    "kernel_ms_per_pass": round(s.kernel_time_us() / 1000 / args.reps / passes, 4),
                    "abi_call_ms": round(best * 1e3, 2), "requests_per_s": round(n / best)}
            t0 = time.perf_counter()
            s.pick(arrs[0][:100000], req[:100000], arrs[1][:100000], arrs[2][:100000], arrs[3][:100000], state[:100000])
            r["%s_python_100k_ms" % strat] = round((time.perf_counter() - t0) * 1e3, 1)
        res["keys_%d" % nk] = r
        s.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
