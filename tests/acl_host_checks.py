"""The checks that the two ACL host programs share (tests/test_acl_cpu.py: gm_acl_match.h alone;
tests/test_acl_dev_host.py: the kernel's phases and the C-ABI's host code), each on the inputs of
tests/acl_cases.py against tests/acl_ref.py.  ``run(compiled, clients, reqs, hash_bits,
pass_names)`` runs the program and returns (first rule per request, stats).  A helper, not a
test."""
import subprocess

import acl_cases as AC
import host_build


def runner(exe, tmp_path):
    def run(compiled, clients, reqs, hash_bits=0, pass_names=0):
        path = tmp_path / "acl_in.txt"
        path.write_text(AC.input_text(compiled, clients, reqs, hash_bits, pass_names))
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           env=host_build.ENV, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:]
        return AC.parse_output(r.stdout, len(reqs))
    return run


def same(reqs, rows, want):
    bad = [(reqs[i], rows[i], want[i]) for i in range(len(reqs)) if rows[i] != want[i]]
    assert not bad, bad[:5]


def check_random(run, n_rules, hash_bits):
    (rules, clients, reqs), compiled, first, res = AC.random_reference(n_rules)
    rows, st = run(compiled, clients, reqs, hash_bits)
    same(reqs, rows, first)
    assert st["rules"] == n_rules and st["filters"] == st["records"] == sum(len(r[3]) for r in compiled)
    assert st["deep"] == 2  # the 40- and the 17-level name; the 16-level one is tokenised
    assert st["candidates"] > st["removed"]
    if hash_bits:
        # 4 bits of hash: different words share tokens; the byte check tells them apart
        assert st["removed"] >= 1, st


def check_named(run, name, hash_bits):
    (rules, clients, reqs), compiled, first, res = AC.reference(name)
    rows, st = run(compiled, clients, reqs, hash_bits)
    same(reqs, rows, first)
    return st


def check_values(run, hash_bits):
    st = check_named(run, "values", hash_bits)
    # 40-byte ids, the literal placeholder of an undefined value: hashed tokens, confirmed on the
    # bytes; the two 40-byte ids differ in hash_bits 0 already, so nothing need be removed there
    assert st["candidates"] >= 1, st


def check_tiling(run, hash_bits):
    st = check_named(run, "tiling", hash_bits)
    assert st["tiles"] == 3, st
    assert st["candidates"] >= 1  # rule 102's who string is a 40-byte id: compared on the bytes


def check_depth(run, hash_bits):
    (rules, clients, reqs), compiled, first, res = AC.reference("depth")
    st = check_named(run, "depth", hash_bits)
    deep = sum(1 for _, _, n in reqs if len(n.split(b"/")) > AC.RS_MAX_LEVELS)
    assert st["deep"] == deep > 0 and st["candidates"] >= deep


def check_block(run, n):
    (rules, clients, reqs), compiled, first, res = AC.block_case(n)
    assert len(reqs) == n
    rows, _ = run(compiled, clients, reqs)
    same(reqs, rows, first)


def check_passes(run):
    (rules, clients, reqs), compiled, first, res = AC.random_reference(65)
    assert -(-len(reqs) // AC.PASS_NAMES) == 14
    rows1, st1 = run(compiled, clients, reqs)
    rows, st = run(compiled, clients, reqs, pass_names=AC.PASS_NAMES)
    assert rows == rows1
    same(reqs, rows, first)
    assert st == st1  # each request is counted in one pass


def check_empty(run, rules):
    import acl_ref as AR
    compiled = [AR.compile(r) for r in rules]
    reqs = [(c % len(AC.CLIENTS), "publish", n) for c, n in enumerate(AC.RR.EDGE_NAMES)]
    rows, st = run(compiled, AC.CLIENTS, reqs)
    assert rows == [None] * len(reqs)
    assert st["records"] == 0 and st["rules"] == len(rules) and st["tiles"] == (1 if rules else 0)


def check_clients(run):
    st = check_named(run, "one_client", 0)
    assert st["rules"] == 2
    (rules, clients, reqs), compiled, first, res = AC.reference("one_client")
    rows, _ = run(compiled, [], [])  # no client, no request
    assert rows == []
