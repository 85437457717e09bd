"""The retainer's limited reads (emqxgm_retain_match_limit: match_messages/3 with
{Cursor, BatchNum}, emqx_retainer_mnesia.erl:185-202) and the host side of the backend contract
(clear_expired/1, page_read/4, the table-full rule, the wildcard delete) on the device, on the
inputs and checks of tests/retain_cases.py -- the ones tests/test_retain_dev_host.py runs on the
CPU gate -- against tests/retain_ref.py."""
import pytest

import retain_cases as RC
import retain_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emqx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import emqx_amd
    return emqx_amd


def einval_of(emqx):
    return lambda: pytest.raises(emqx.EngineError, match="-22")


@pytest.fixture(scope="module", params=[RC.DEFAULT, []], ids=["index", "scan"])
def built(request, emqx):
    """One built store per index setting, shared by the read-only page tests."""
    dev, ref = emqx.Retainer(index_specs=request.param), RR.Retainer(request.param)
    RC.build(dev, ref, request.param)
    yield dev, ref
    dev.close()


@pytest.mark.parametrize("limit", RC.LIMITS)
def test_page_identity(built, limit):
    dev, ref = built
    RC.check_page_identity(dev, ref, RC.FILTERS, [limit] * len(RC.FILTERS))


@pytest.mark.parametrize("n", RC.BATCHES)
def test_page_identity_mixed_batches(built, n):
    dev, ref = built
    fs, ls = RC.mixed_batch(n)
    RC.check_page_identity(dev, ref, fs, ls)


def test_only_the_windows_are_downloaded(built):
    """n_ids of a call is the sum of its windows, not of the selected sets."""
    dev, _ = built
    fs = [b"#", b"dead/#", b"nope/#", b"p1/#"]
    ptr, ids, cur = dev.match_pages_ids(fs, [7, 0, 3, 5], [None] * 4, RC.NOW)
    assert list(ptr) == [0, 7, 7 + 195, 7 + 195, 7 + 195 + 1] and len(ids) == 203
    assert [c[1] for c in cur] == [RC.RC_BASE, RC.RC_DONE, RC.RC_DONE, RC.RC_DONE]
    ptr, ids, cur = dev.match_pages_ids(fs, [7, 0, 3, 5], cur, RC.NOW)
    assert list(ptr) == [0, 7, 7, 7, 7] and len(ids) == 7


def test_forged_cursors(built, emqx):
    RC.check_forged(built[0], einval_of(emqx))


def test_cursor_api_and_stale(emqx):
    dev, ref = emqx.Retainer(), RR.Retainer(RC.DEFAULT)
    RC.build(dev, ref, RC.DEFAULT)
    rows, cur, reads = [], None, 0
    while True:
        got, cur = dev.match_messages_cursor(b"pd/#", cur, 3, RC.NOW)
        rows += got
        reads += 1
        if cur is None:
            break
    assert rows == dev.match_messages(b"pd/#", RC.NOW) and len(rows) == 68 and reads == 23
    _, cur = dev.match_messages_cursor(b"pd/#", None, 3, RC.NOW)
    dev.clean()
    with pytest.raises(emqx.retainer.StaleCursor):
        dev.match_messages_cursor(b"pd/#", cur, 3, RC.NOW)
    dev.close()


def test_cursors_under_change(emqx):
    dev, ref = emqx.Retainer(), RR.Retainer(RC.DEFAULT)
    RC.build(dev, ref, RC.DEFAULT)
    RC.check_cursors_under_change(dev, ref)
    dev.close()


def test_clear_expired(emqx):
    dev = emqx.Retainer()
    RC.check_clear_expired(dev, RR.Retainer(RC.DEFAULT))
    dev.close()


@pytest.mark.parametrize("limit", [1, 3])
def test_table_full(emqx, limit):
    dev = emqx.Retainer()
    RC.check_table_full(dev, RR.Retainer(RC.DEFAULT), limit)
    dev.close()


@pytest.mark.parametrize("specs", [RC.DEFAULT, []], ids=["index", "scan"])
def test_page_read(emqx, specs):
    dev = emqx.Retainer(index_specs=specs)
    RC.check_page_read(dev, RR.Retainer(specs))
    RC.check_page_read_invalid(dev, einval_of(emqx))
    dev.close()


@pytest.mark.parametrize("specs", [RC.DEFAULT, []], ids=["index", "scan"])
def test_delete_matching(emqx, specs):
    dev = emqx.Retainer(index_specs=specs)
    RC.check_delete_matching(dev, RR.Retainer(specs), specs)
    dev.close()


@pytest.mark.parametrize("name", sorted(RC.golden()))
def test_suite_vectors(emqx, name):
    dev = emqx.Retainer()
    RC.run_golden(dev, RC.golden()[name])
    dev.close()
