"""The NIF (c_src/emqx_trie_gpu_nif.c) over the engine on the device: the driver of
tests/host_harness/nif_driver.c on the fake erl_nif runtime (tests/nif_stub), built without a
sanitizer and linked against the engine library (emqx_amd.build.build_nif_driver).

Each scenario is one driver process with its own time limit.  A to D are the scenarios of
tests/nif_cases.py that the CPU gate (tests/test_nif_host.py) runs over the mock engine; E and F
(tests/nif_family_cases.py) are the retainer and the other families.  What a result or a message
must be comes from the Python references alone.  A driver that ends by a signal or at its limit
fails its test and the module's remaining scenarios are skipped: nothing is run again on a device
that may be in trouble."""
import subprocess

import pytest

import nif_cases as C
import nif_family_cases as F

pytestmark = pytest.mark.gpu
LIMIT_S = 120
_broken = []  # set by a driver run that died: the remaining scenarios do not start
_runs = {}    # scenario -> (its run, its check): each scenario runs once per session


def _snapshot(tmp):
    return str(tmp.mktemp("nif") / "snapshot").encode()


SCENARIOS = {
    "A-match_async": lambda s, tmp: C.case_match(s),
    "B-publish_async": lambda s, tmp: C.case_publish(s, mock=False),
    "C-cancel": lambda s, tmp: C.case_cancel(s),
    "D-resync": lambda s, tmp: C.case_resync(s, _snapshot(tmp), mock=False),
    "E-retainer": lambda s, tmp: F.case_retainer(s),
}
SCENARIOS.update({"F-" + k: (lambda s, tmp, fn=fn: fn(s)) for k, fn in F.FAMILIES.items()})


@pytest.fixture(scope="module")
def driver():
    import torch
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from emqx_amd import build
    return build.build_nif_driver()


def scenario(driver, tmp, name):
    if name in _runs:
        return _runs[name]
    if _broken:
        pytest.skip("an earlier driver run died (%s)" % _broken[0])
    s = C.Script()
    check = SCENARIOS[name](s, tmp)
    try:
        r = C.run(driver, s, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        _broken.append(name + ": time limit")
        pytest.fail("the driver ran into its %d s limit" % LIMIT_S)
    if r.returncode < 0:
        _broken.append("%s: signal %d" % (name, -r.returncode))
        pytest.fail(r.tail())
    _runs[name] = (r, check)
    return r, check


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario(driver, tmp_path_factory, name):
    r, check = scenario(driver, tmp_path_factory, name)
    assert r.clean() and r.mailbox == 0, r.tail()
    check(r)


def test_every_entry_ran_on_the_device(driver, tmp_path_factory):
    """The union of the function tables that A to F print: every name/arity of the NIF was called
    on the device (test_scenario asserts that the calls were accepted and answered rightly)."""
    total = {}
    for name in sorted(SCENARIOS):
        r, _ = scenario(driver, tmp_path_factory, name)
        assert r.returncode == 0, r.tail()
        for k, n in r.table.items():
            total[k] = total.get(k, 0) + n
    assert len(total) >= 61, sorted(total)
    assert not [k for k, n in total.items() if n == 0], sorted(k for k, n in total.items() if n == 0)
