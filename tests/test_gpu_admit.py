"""GPU parity of the admission pass (emqx_amd.Admission over emqxgm_admit_*, k_admit; DESIGN.md 6b
"Admission") against the reference semantics of tests/admit_ref.py, on the case tables of
tests/admit_cases.py -- the same ones the CPU gate (tests/test_admit_dev_host.py) runs the kernel's
phases and the host code on under ASan + UBSan: every record word for word, with the LDS tile
(force_global off) and from global memory (on)."""
import pytest

import admit_cases as AC
import admit_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


@pytest.fixture(scope="module")
def adm(emqx):
    a = emqx.Admission(0)
    yield a
    a.close()


def _run(adm):
    def run(b, force_global):
        adm.set_caps(b["caps"])
        adm.tune("force_global", int(force_global))
        adm.tune("byte_base", b["base"])
        adm.tune("pass_items", b["pass_items"] or (1 << 22))
        recs = adm.records(b["mode"], b["items"], b["flags"], b["zones"])
        for r in recs[:64]:
            assert adm.reason(b["mode"], r) == R.reason(b["mode"], r.tolist())
        return [tuple(r) for r in recs.tolist()]
    return run


@pytest.mark.parametrize("force_global", [False, True])
@pytest.mark.parametrize("table", sorted(AC.TABLES))
def test_table(adm, table, force_global):
    assert AC.check_table(_run(adm), table, force_global) > 0


def test_in_the_oracles_terms(emqx):
    """validate, parse and the checks of emqx_amd.Admission, as the reference returns them."""
    a = emqx.Admission(0, caps=[R.caps(), R.caps(max_topic_levels=2, max_qos_allowed=1, retain_available=False,
                                               wildcard_subscription=False, shared_subscription=False)])
    items = AC.PARSE_ITEMS + AC.ALIGN_ITEMS + list(AC.MALFORMED.values())
    for kind in ("name", "filter"):
        assert a.validate(kind, items) == [R.validate(kind, it) for it in items]
    for has in (False, True):
        got = a.parse(items, [has] * len(items))
        for it, g in zip(items, got):
            want = R.parse(it, {"share": True} if has else {})
            assert g == (("invalid_topic_filter", it) if want is None else want), (it, has)
    assert a.parse([b"$share/g/$exclusive/t"]) == [(b"t", {"share": b"g", "is_exclusive": True})]
    names = [b"a", b"a/b/c", b"a/+", b"a", b"a", b"\xff"]
    assert a.check_publish(names, [0, 0, 0, 2, 1, 0], [False, False, False, False, True, False], [1] * 6) == \
        [0, 0x90, 0x90, 0x9B, 0x9A, 0x90]
    assert a.check_publish(names, [0, 0, 0, 2, 1, 0], [False] * 6) == [0, 0, 0x90, 0, 0, 0x90]
    filters = [b"t", b"a/b/c", b"+/#", b"$share/g/t", b"$share/t", b"a/#/b", b"$exclusive/t", b"t"]
    assert a.check_subscribe(filters, zones=[1] * 8) == [0, 0x8F, 0xA2, 0x9E, emqx.admission.RAISES, 0x8F, 0x8F, 0]
    assert a.check_subscribe([b"t"], has_share=[True], zones=[1]) == [0x9E]
    assert a.check_subscribe_packet([]) == 0x8F
    assert a.check_subscribe_packet([b"a/b", b"$share/g/+"]) == 0
    assert a.check_subscribe_packet([b"a/b", b"a/#/b"]) == 0x8F
    assert a.check_subscribe_packet([b"a/b", b"\xc0\x80"]) == 0x8F
    st = a.stats()
    assert st["calls"] > 0 and st["items"] > 0 and st["passes"] > 0
    a.close()


def test_refused_calls(emqx, adm):
    E = emqx.EngineError
    adm.set_caps(None)
    for call in (lambda: adm.tune("no_such_key", 1), lambda: adm.tune("byte_base", 16), lambda: adm.tune("pass_items", 0),
                 lambda: adm.records(2, [b"a"]), lambda: adm.records(R.NAME, [b"a"], zones=[200])):
        with pytest.raises(E):
            call()
    with pytest.raises(ValueError):
        emqx.Admission(0, caps=[])
    adm.set_caps(None)
    assert adm.records(R.NAME, [b"a/b"]).tolist() == [[0, 2, 0, R.NONE]]
