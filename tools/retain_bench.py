"""Reverse-match throughput of the retained-topic store: N cfg3 topics
retained, a batch of cfg3-shaped subscription filters matched against them (emqxgm_retain_match,
end to end: host filters in, host CSR of topic ids out).

  python tools/retain_bench.py [--topics 2000000] [--filters 100000]
  python tools/retain_bench.py --pages [--topics 2000000] [--page 1000] [--out FILE]

--pages: limited reads (emqxgm_retain_match_limit) over the same store -- '#' and 1,000 cfg3
subscription filters read in pages of --page ids: time per page and per full traversal, the
HIP-event times of the limited read's own launches, and the unlimited emqxgm_retain_match of the
same store and filters (three runs, for an A/B against another build: a tree without the
limited read reports that part alone).  One JSON line, appended to --out when given.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topics", type=int, default=2_000_000)
    ap.add_argument("--filters", type=int, default=100_000)
    ap.add_argument("--pages", action="store_true")
    ap.add_argument("--page", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import workloads
    from emqx_amd import Retainer
    if args.pages:
        return pages(args, workloads, Retainer)
    w = workloads.generate(3, args.filters, args.topics)
    r = Retainer()
    t0 = time.perf_counter()
    to = w.toff.astype(np.int64)
    for i in range(w.nt):
        r.store_retained(bytes(w.tbytes[to[i]:to[i + 1]]))
    t1 = time.perf_counter()
    r.commit()
    t2 = time.perf_counter()
    filters = [w.filter(i) for i in range(w.nf)]
    r.match_ids(filters[:1000], 1)
    best, n_ids = 1e9, 0
    for _ in range(3):
        t3 = time.perf_counter()
        ptr, ids = r.match_ids(filters, 1)
        best = min(best, time.perf_counter() - t3)
        n_ids = len(ids)
    # delta commits: 10k new retained topics, then 10k deletions of base topics
    extra = [b"x/" + w.topic(i) for i in range(10_000)]
    t4 = time.perf_counter()
    for t in extra:
        r.store_retained(t)
    t5 = time.perf_counter()
    r.commit()
    t6 = time.perf_counter()
    for i in range(10_000):
        r.delete_message(w.topic(i))
    r.commit()
    t7 = time.perf_counter()
    ptr2, ids2 = r.match_ids(filters, 1)
    st = r.stats()
    print(json.dumps({
        "delta_store_10k_commit_s": round(t6 - t5, 4), "delta_store_10k_registry_s": round(t5 - t4, 4),
        "delete_10k_base_topics_incl_registry_s": round(t7 - t6, 4), "stats": st,
        "ids_after_churn": int(len(ids2))}), flush=True)
    print(json.dumps({
        "retained_topics": r.size(), "filters": len(filters), "ids_selected": n_ids,
        "store_registry_s": round(t1 - t0, 3), "commit_build_s": round(t2 - t1, 3),
        "match_s": round(best, 4), "filters_per_s": round(len(filters) / best),
        "ids_per_s": round(n_ids / best)}), flush=True)


def pages(args, workloads, Retainer):
    w = workloads.generate(3, 1000, args.topics)
    r = Retainer()
    to = w.toff.astype(np.int64)
    for i in range(w.nt):
        r.store_retained(bytes(w.tbytes[to[i]:to[i + 1]]))
    r.commit()
    subs = [w.filter(i) for i in range(w.nf)]
    res = {"leg": "pages", "retained_topics": r.size(), "filters": len(subs), "page": args.page}
    # the unlimited match: '#' alone, and the 1,000 filters
    for name, fs in (("hash", [b"#"]), ("subs", subs)):
        r.match_ids(fs, 1)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            _, ids = r.match_ids(fs, 1)
            ts.append(round(time.perf_counter() - t0, 5))
        res["unlimited_%s_s" % name] = ts
        res["unlimited_%s_ids" % name] = int(len(ids))
    if hasattr(r, "match_pages_ids"):
        r.tune("timing", 1)
        for name, fs in (("hash", [b"#"]), ("subs", subs)):
            lim = [args.page] * len(fs)
            cur = [None] * len(fs)
            per_page, ev, n_ids, most = [], [], 0, 0
            t0 = time.perf_counter()
            while True:
                t1 = time.perf_counter()
                _, ids, cur = r.match_pages_ids(fs, lim, cur, 1)
                per_page.append(time.perf_counter() - t1)
                ev.append(r.timing())
                n_ids += len(ids)
                most = max(most, len(ids))
                if all(c[1] == 3 for c in cur):
                    break
            total = time.perf_counter() - t0
            per_page.sort()
            res["paged_" + name] = {
                "calls": len(per_page), "traversal_s": round(total, 4), "ids": n_ids,
                "max_ids_per_call": most,
                "page_ms_median": round(1e3 * per_page[len(per_page) // 2], 4),
                "page_ms_max": round(1e3 * per_page[-1], 4),
                "event_ms_median": {k: round(sorted(e[k] for e in ev)[len(ev) // 2], 4)
                                    for k in ev[0]}}
            assert n_ids == res["unlimited_%s_ids" % name]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
