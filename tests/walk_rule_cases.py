"""What the device tests of the walk's rules share (tests/test_gpu_psig.py, test_gpu_keyed_share.py,
test_gpu_closed.py): an engine loaded beside the Python restatement of emqx_trie
(oracle/emqx_ref.py), the row check through a matrix of tune switches, and the census call."""
import itertools

import numpy as np

from oracle import emqx_ref as R


def _bytes(xs):
    return [x if isinstance(x, bytes) else x.encode() for x in xs]


def load(emqx, filters, bits=0, keyed=2, fat=None, dedup_sorted=False):
    """An engine that patches whenever possible and the oracle, with the filters inserted in the
    order given -- insertion order decides filter ids -- or, dedup_sorted, as sorted(set(filters)).
    fat: tune "fat_buckets", None to leave the default."""
    eng = emqx.Engine(word_hash_bits=bits)
    eng.tune("keyed", keyed)
    if fat is not None:
        eng.tune("fat_buckets", fat)
    eng.tune("delta_commit", 2)  # patch whenever possible
    py = R.Trie()
    for f in _bytes(sorted(set(filters)) if dedup_sorted else filters):
        eng.trie_insert(f)
        py.insert(f)
    eng.commit()
    return eng, py


def check(eng, py, topics, what, switches, pairs=(0, 1, 2)):
    """Rows equal the oracle's, compared by filter name, for every tune "walk_pair" of pairs (0 one
    lane per topic: the kernels with the rules, 1 the default choice, 2 every batch through the
    pair walk) x every 1/0 combination of the named switches, the first named outermost.  All
    of them are 1 again afterwards.  Returns the oracle's rows."""
    topics = _bytes(topics)
    want = [sorted(py.match(t)) for t in topics]  # (once per state, shared by the matrix)
    names = {}

    def name(f):
        if f not in names:
            names[f] = eng.filter_bytes(f)
        return names[f]

    for pair in pairs:
        eng.tune("walk_pair", pair)
        for values in itertools.product((1, 0), repeat=len(switches)):
            for k, v in zip(switches, values):
                eng.tune(k, v)
            res = eng.match(topics)
            for i, t in enumerate(topics):
                got = sorted(name(int(f)) for f in res.row(i))
                assert got == want[i], (what, pair) + values + (t,)
    for k in ("walk_pair",) + tuple(switches):
        eng.tune(k, 1)
    return want


def census(eng, topics):
    """One census pass (a one-lane walk) over the topics."""
    import torch
    from emqx_amd.engine import pack
    tb, to = pack(_bytes(topics), np.uint32)
    db = torch.from_numpy(tb).cuda()
    do = torch.from_numpy(to.view(np.int32)).cuda()
    torch.cuda.synchronize()
    return eng.walk_census(db.data_ptr(), do.data_ptr(), len(topics), int(to[-1]))
