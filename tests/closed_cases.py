"""The miniature cfg3 that the closed-bucket tests share (tests/test_closed_host.py on the CPU,
tests/test_gpu_closed.py on the device), and the census figures both must reproduce on it.

The miniature is tests/test_gpu_keyed_share.py's (8 sites x 24 devices, the five filter patterns of
workloads/gen.cpp gen_cfg3, 2,000 topics and 12 special ones, seed 31), so that the figures with the
rule off are the ones MEASUREMENTS r09 records for the parent on it: 5,310 bucket loads and 3,161
lane iterations for the census walk with root_plus_half and keyed_share on."""
import random

SITES, DEVS = 8, 24
SEED = 31


def dev(s, j):
    return s * DEVS + j  # global device ids: a token D has the two parents site/s/device, site/+/device


def cfg3_filters(rng):
    fs = set()
    for s in range(SITES):
        for j in range(DEVS):
            d = dev(s, j)
            r = rng.random()
            if r < 0.7:
                fs.add(f"site/{s}/device/{d}/#")
            if r > 0.4:
                fs.add(f"site/+/device/{d}/#")
            if rng.random() < 0.3:
                for k in range(16):
                    if rng.random() < 0.25:
                        fs.add(f"site/{s}/device/{d}/+/{k}")
        for m in range(8):
            if rng.random() < 0.5:
                fs.add(f"site/{s}/device/+/m{m}")
            if rng.random() < 0.3:
                fs.add(f"site/{s}/+/+/m{m}")
    return sorted(fs)


def cfg3_topics(rng, n):
    ts = []
    for _ in range(n):
        s = rng.randrange(SITES + 1)  # (site 8: no such site)
        d = dev(s, rng.randrange(DEVS + 2)) if rng.random() < 0.9 else rng.randrange(400)
        ts.append(f"site/{s}/device/{d}/m{rng.randrange(9)}/{rng.randrange(16)}")
    ts += ["site", "site/1", "site/1/device", "site/1/device/24", "site/1/device/24/m1/3",
           "site/1/device/24/m1/3/a/b", "site/1/device/24/" + "/".join("l%d" % i for i in range(13)),
           "$site/1/device/24/m1/3", "$site", "$SYS/x", "site/+/device/24/m1/3", "other/1/device/24/m1/3"]
    return ts


def miniature():
    """(filters in registration order, topics)"""
    rng = random.Random(SEED)
    filters = cfg3_filters(rng)
    topics = cfg3_topics(rng, 2000)
    return sorted(set(filters)), topics


# Census of the miniature, {closed_buckets: (bucket loads, lane iterations)}: 0 = the parent's
# figures (MEASUREMENTS r09), 1 = the CPU restatement's count with the rule
# (tests/host_harness/closed_harness.cpp --count), which the device must equal.
CENSUS = {0: (5310, 3161), 1: (4742, 2654)}
