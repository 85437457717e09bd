"""k_admit's time (emqxgm_admit_batch, DESIGN.md 6b "Admission") from HIP events, warm, for two
inputs, each beside its yardstick:

  names    1M cfg3-shaped topic names, NAME mode; the yardstick is k_tok on the same batch (the
           engine's profiling counters: it reads the same bytes and writes 44-72 B per topic where
           k_admit writes 16), so k_admit slower than k_tok is a finding to explain;
  filters  1M filters, 10% of them "$share/<group>/..." and 1% with multi-byte words, FILTER mode;
           the yardstick is gm_admit_match.h compiled for the host (tools/admit_host_bench.cpp),
           on one core and on --threads cores.

Each figure is the median of --reps warm runs after --warmup; with the LDS tile and with
force_global.

  python tools/admit_bench.py [--items 1000000] [--reps 10] [--warmup 3] [--threads 16]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _kernel_ms(adm, mode, items, reps, warmup):
    for _ in range(warmup):
        adm.records(mode, items)
    ms = []
    for _ in range(reps):
        adm.tune("timing", 1)  # resets the sum
        adm.records(mode, items)
        ms.append(adm.kernel_time_us() / 1000.0)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _host_ms(items, mode, threads, reps):
    exe = os.path.join(tempfile.gettempdir(), "admit_host_bench_%d" % os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "admit_host_bench.cpp"), "-o", exe],
                   check=True)
    from emqx_amd.engine import pack
    buf, off = pack(items, np.uint32)
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(np.uint32(len(items)).tobytes())
        f.write(off.tobytes())
        f.write(buf.tobytes() + b"\0" * 8)
        path = f.name
    try:
        return {str(t): float(subprocess.run([exe, path, str(mode), str(t), str(reps)], check=True,
                                             stdout=subprocess.PIPE, text=True).stdout.split()[0])
                for t in (1, threads)}
    finally:
        os.unlink(path)
        os.unlink(exe)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import workloads
    from emqx_amd import Admission, Engine
    from emqx_amd.admission import FILTER, NAME
    w = workloads.generate(3, 1000, args.items)
    names = [w.topic(i) for i in range(w.nt)]
    rng = random.Random(5)
    filters = []
    for i, nm in enumerate(names):
        parts = nm.split(b"/")
        if rng.random() < 0.3:
            parts[rng.randrange(len(parts))] = b"+"
        if rng.random() < 0.2:
            parts[-1] = b"#"
        if i % 100 == 0:
            parts[0] = "wärme-€-\U0001F600".encode()
        f = b"/".join(parts)
        filters.append(b"$share/g%d/" % (i % 8) + f if i % 10 == 0 else f)
    out = {"items": len(names), "name_bytes": sum(map(len, names)), "filter_bytes": sum(map(len, filters))}
    adm = Admission()
    for key, mode, items in (("names", NAME, names), ("filters", FILTER, filters)):
        res = {}
        for fg in (0, 1):
            adm.tune("force_global", fg)
            res["k_admit_global" if fg else "k_admit_lds"] = _kernel_ms(adm, mode, items, args.reps, args.warmup)
        recs = adm.records(mode, items)
        res["not_ok"] = int(((recs[:, 0] & 0xFFFF) != 0).sum())
        out[key] = res
    adm.close()
    # k_tok on the names, through the engine's profiling counters
    eng = Engine()
    eng.trie_insert(b"site/+/device/+/m7/#")
    eng.commit()
    for _ in range(args.warmup):
        eng.match(names)
    eng.set_profiling(True)
    tok = []
    for _ in range(args.reps):
        s0 = eng.stats()
        eng.match(names)
        s1 = eng.stats()
        tok.append((s1["tok_ms"] - s0["tok_ms"]) / max(1, s1["tok_launches"] - s0["tok_launches"]))
    out["names"]["k_tok"] = {"median_ms": round(statistics.median(tok), 4), "min_ms": round(min(tok), 4),
                             "max_ms": round(max(tok), 4)}
    out["filters"]["host_ms_by_threads"] = _host_ms(filters, FILTER, args.threads, 5)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
