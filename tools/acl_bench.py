"""Throughput of ACL rule lists matched on the device (emqxgm_acl_match, k_acl; DESIGN.md 6b
"ACL lists"): 1M cfg3 topic names (the generator of tools/rules_bench.py), each a publish or a
subscribe of one of 10k clients (a client's id is the device word of some name; half of the
requests take client i mod 10k, half a random one, so few requests come from the client whose
id the name carries and the closing deny decides nearly all), against 64 rules of which a quarter
are ${clientid} patterns; end to end (host requests in, host answers out) with the kernel time
per pass by HIP events.  Beside it, on the same names:

  * emqxgm_match_rules (k_rules) with the same 64 filters, placeholders left literal -- the
    nearest path the library had before: no client, no action, no who;
  * the host loop it replaces: tests/acl_ref.py's matches/4 (emqx_authz_rule restated in Python)
    over a sample of the requests on one core.

  python tools/acl_bench.py [--names 1000000] [--rules 64] [--clients 10000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _best(fn, reps):
    best, out = 1e9, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return best, out


def rule_list(n_rules):
    """Three quarters plain filters that match no name, then the patterns (a client may use the
    topics under its own device id), then a closing deny."""
    n_pat = n_rules // 4
    plain = [("deny", "all", "all", [f"site/{s}/device/+/m{s % 32}/#"])
             for s in range(10_000, 10_000 + n_rules - n_pat - 1)]
    pats = [("allow", "all", "publish" if k % 2 else "all", [f"site/+/device/${{clientid}}/m{k}/#"])
            for k in range(n_pat - 1)] + [("allow", "all", "subscribe", ["site/+/device/${clientid}/#"])]
    return plain + pats + [("deny", "all")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=1_000_000)
    ap.add_argument("--rules", type=int, default=64)
    ap.add_argument("--clients", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=2000)
    args = ap.parse_args()
    import numpy as np
    import workloads
    from emqx_amd import NONE, AclList, Engine
    from emqx_amd import engine as E
    w = workloads.generate(3, 1000, args.names)
    names = [w.topic(i) for i in range(w.nt)]
    n = len(names)
    # a client's id is the device word of some name, so its pattern rules can match
    ids = []
    seen = set()
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
    rules = rule_list(args.rules)
    al = AclList(rules)
    users = [b"user-" + c for c in ids]
    bits = [0] * len(ids)
    al.acl.match(names[:1000], client[:1000] % len(ids), action[:1000], ids, users, bits)
    al.acl.tune("timing", 1)
    best, out = _best(lambda: al.acl.match(names, client, action, ids, users, bits), args.reps)
    passes = -(-n // (1 << 20))
    res = {"names": n, "rules": len(rules), "pattern_rules": sum(1 for r in al.rules if r[3] and r[3][0][0] == "pattern"),
           "clients": len(ids), "names_per_s_end_to_end": round(n / best),
           "kernel_ms_per_pass": round(al.acl.kernel_time_us() / 1000 / args.reps / passes, 3), "passes": passes,
           "allow": int(sum(1 for r in out.tolist() if r != NONE and al.rules[r][0] == "allow")),
           "deny": int(sum(1 for r in out.tolist() if r != NONE and al.rules[r][0] == "deny"))}
    # the nearest earlier path: first matching filter, placeholders literal
    filters, flags = al.plan[0], [E.RULE_EQ if f else E.RULE_WORDS for f in al.plan[1]]
    eng = Engine()
    eng.match_rules(names[:1000], filters, flags)
    b2, _ = _best(lambda: eng.match_rules(names, filters, flags), args.reps)
    res["match_rules_names_per_s_end_to_end"] = round(n / b2)
    # the host loop on one core
    import acl_ref as AR
    compiled = [AR.compile(r) for r in rules]
    k = min(args.host_sample, n)
    cl = [{"clientid": ids[int(client[i])], "username": users[int(client[i])], "peerhost": None} for i in range(k)]
    t0 = time.perf_counter()
    want = [AR.matches(cl[i], "publish" if action[i] == 1 else "subscribe", names[i], compiled) for i in range(k)]
    res["host_loop_names_per_s_one_core"] = round(k / (time.perf_counter() - t0))
    got = ["nomatch" if r == NONE else ("matched", al.rules[r][0]) for r in out[:k].tolist()]
    assert got == want, "the device and the host loop disagree"
    al.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
