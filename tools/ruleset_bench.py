"""Throughput of rule sets that return every matching rule per name (emqxgm_ruleset_match,
k_ruleset): 1M cfg3 topic names (the generator of tools/rules_bench.py) against 64
single-filter rules, end to end (host names in, host rows out), with the count-pass and
fill-pass kernel times by HIP events.

  list (i)   64 rules none of which matches any name: the first-match path (emqxgm_match_rules,
             k_rules) then evaluates all 64 per name too, the same work -- measured beside it;
  list (ii)  the 64 rules of tools/rules_bench.py (the last two match).

  python tools/ruleset_bench.py [--names 1000000] [--rules 64] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _best(fn, reps):
    best, out = 1e9, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=1_000_000)
    ap.add_argument("--rules", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import workloads
    from emqx_amd import NONE, Engine, RuleSet
    w = workloads.generate(3, 1000, args.names)
    names = [w.topic(i) for i in range(w.nt)]
    miss = [f"site/{s}/device/+/m{s % 32}/#".encode() for s in range(10_000, 10_000 + args.rules)]
    lists = {"i_no_match": miss,
             "ii_rules_bench": miss[:args.rules - 2] + [b"site/+/device/+/m7/#", b"site/#"]}
    out = {"names": len(names), "rules": args.rules}
    eng = Engine()
    for key, filters in lists.items():
        rs = RuleSet([[f] for f in filters])
        rs.match(names[:1000])
        rs.tune("timing", 1)
        best, (ptr, rule) = _best(lambda: rs.match_csr(names), args.reps)
        count_us, fill_us = rs.kernel_times_us()
        res = {"names_per_s_end_to_end": round(len(names) / best),
               "count_kernel_ms": round(count_us / 1000 / args.reps, 3),
               "fill_kernel_ms": round(fill_us / 1000 / args.reps, 3),
               "row_entries": int(ptr[-1])}
        if key == "i_no_match":
            fl = [0] * len(filters)
            eng.match_rules(names[:1000], filters, fl)
            b2, r = _best(lambda: eng.match_rules(names, filters, fl), args.reps)
            assert int((r != NONE).sum()) == 0 and int(ptr[-1]) == 0
            res["match_rules_names_per_s_end_to_end"] = round(len(names) / b2)
        out[key] = res
        rs.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
