"""The built-in authorization database on the device (emqxgm_acldb_match, k_acldb; DESIGN.md 6b
"Built-in database") on the requests of tools/acl_bench.py: 1M cfg3 topic names, each a publish
or a subscribe of one of 10k clients whose id is the device word of some name.

  (a) the nearest earlier path: AclList.from_builtin_db at the largest table it accepts with the
      four `all` rules, 16,383 client-id keys x 4 rules (emqxgm_acl_match, k_acl);
  (b) emqxgm_acldb_match on that same table;
  (c) emqxgm_acldb_match at --keys keys x 4 rules (default 100,000 and 1,000,000), with the same
      requests and the same `all` rules;
  (d) one changed record committed at the largest table, against a full reload.

For (a) to (c): the kernel time per pass by HIP events and the end-to-end time, best of --reps.
One JSON line.

  python tools/acldb_bench.py [--names 1000000] [--clients 10000] [--keys 100000,1000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL_RULES = [("deny", "subscribe", b"site/+/device/+/secret/#"), ("allow", "subscribe", b"site/+/status"),
             ("allow", "all", b"shared/#"), ("deny", "all", b"#")]

LIST_KEYS = (65536 - len(ALL_RULES)) // 4  # emqxgm_acl_set takes 65,536 rules


def key_rules(cid: bytes):
    """A client may use the topics under its own device id."""
    return [("allow", "publish", b"site/+/device/${clientid}/m1/#"), ("allow", "subscribe", b"site/+/device/${clientid}/#"),
            ("deny", "publish", b"eq site/0/device/" + cid + b"/reset"), ("allow", "all", b"site/+/device/${clientid}")]


def _best(fn, reps):
    best, out = 1e9, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return best, out


def table(ids, n_keys):
    """n_keys client-id records: the clients' own ids first, then ids no request carries."""
    keys = list(ids[:n_keys]) + [b"pad-%07d" % i for i in range(max(0, n_keys - len(ids)))]
    return [(("clientid", k), key_rules(k)) for k in keys] + [("all", ALL_RULES)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=1_000_000)
    ap.add_argument("--clients", type=int, default=10_000)
    ap.add_argument("--keys", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import workloads
    from emqx_amd import NONE, AclList, BuiltinDb
    w = workloads.generate(3, 1000, args.names)
    names = [w.topic(i) for i in range(w.nt)]
    n = len(names)
    ids, seen = [], set()
    for t in names:
        ws = t.split(b"/")
        if len(ws) > 3 and ws[3] not in seen:
            seen.add(ws[3])
            ids.append(ws[3])
            if len(ids) == args.clients:
                break
    rng = np.random.default_rng(13)
    own = np.array([i % len(ids) for i in range(n)], np.uint32)
    client = np.where(rng.random(n) < 0.5, own, rng.integers(0, len(ids), n, dtype=np.uint32)).astype(np.uint32)
    action = rng.integers(1, 3, n, dtype=np.uint32)
    users = [b"user-" + c for c in ids]
    passes = -(-n // (1 << 20))
    res = {"names": n, "clients": len(ids), "passes": passes}

    # (a) the flattened list at its limit
    recs = table(ids, LIST_KEYS)
    al = AclList.from_builtin_db(recs)
    bits = [0] * len(ids)
    al.acl.match(names[:1000], client[:1000], action[:1000], ids, users, bits)
    al.acl.tune("timing", 1)
    best, out_a = _best(lambda: al.acl.match(names, client, action, ids, users, bits), args.reps)
    perm_a = np.array([NONE if r == NONE else (1 if al.rules[r][0] == "allow" else 0) for r in out_a.tolist()], np.uint32)
    res["a_acl_list_%dx4" % LIST_KEYS] = {"rules": len(al.rules), "end_to_end_ms": round(best * 1e3, 2),
                                 "kernel_ms_per_pass": round(al.acl.kernel_time_us() / 1000 / args.reps / passes, 3)}
    al.close()

    def timed_db(records):
        db = BuiltinDb()
        t0 = time.perf_counter()
        db.store_many(records)
        db.commit()
        load = time.perf_counter() - t0
        db.db.match(names[:1000], client[:1000], action[:1000], ids, users)
        db.db.tune("timing", 1)
        best, out = _best(lambda: db.db.match(names, client, action, ids, users), args.reps)
        r = {"records": db.record_count(), "load_s": round(load, 2), "end_to_end_ms": round(best * 1e3, 2),
             "kernel_ms_per_pass": round(db.db.kernel_time_us() / 1000 / args.reps / passes, 3)}
        return db, out, r

    # (b) the keyed store on the same table: the same permissions
    db, out_b, r = timed_db(recs)
    assert (out_b[0] == perm_a).all(), "k_acldb and k_acl disagree"
    res["b_acldb_%dx4" % LIST_KEYS] = r
    db.close()
    # (c) more keys, the same requests
    for nk in [int(k) for k in args.keys.split(",") if k]:
        db, out_c, r = timed_db(table(ids, nk))
        assert (out_c[0] == perm_a).all() or nk < LIST_KEYS, "the answers changed with the number of keys"
        res["c_acldb_%dx4" % nk] = r
        # (d) one changed record against the full reload above
        t0 = time.perf_counter()
        db.store_rules(("clientid", ids[0]), key_rules(ids[0])[::-1])
        db.commit()
        r["one_record_commit_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        r["stats"] = {k: v for k, v in db.db.stats().items() if k in ("rebuilds", "growths", "clientid_slots", "live_words")}
        db.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
