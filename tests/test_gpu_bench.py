"""bench.py end to end on a small cfg1 index: a plain run reports the headline alone and
--dump-outputs writes what its last timed step returned (checked against the oracle); --full
adds the figures measured beside it.  The benchmark runs as its own process, as the driver
starts it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.cref import RefIndex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF, NT = 5000, 20000
SIZE = ["--cfg", "1", "--filters", str(NF), "--topics", str(NT), "--settle-s", "0"]
EXTRAS = ("roofline", "cpu_baseline", "crossover", "end_to_end", "nif_windows", "nif_concurrent",
          "subscribe")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SIZE, *args],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == 1, out
    return json.loads(out[0])


def test_plain_run_reports_the_headline_and_dumps_its_last_step(tmp_path):
    import workloads
    steps, warmup = 4, 2
    line = _bench("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path))
    assert line["metric"] == "published topics matched/sec (cfg1)"
    assert line["unit"] == "topics/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(NT / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert all(line[k] is None for k in EXTRAS)
    assert line["config"]["one_pass_at_a_time"] is None and "pairs_per_batch" not in line["config"]

    # the last timed step's batch: the rotation starts with the warm-up steps
    seeds = line["config"]["topic_seeds"]
    seed = seeds[(warmup + steps - 1) % len(seeds)]
    w = workloads.generate(1, NF, NT)
    t = workloads.generate(1, NF, NT, seed_t=seed, topics_only=True)
    ref = RefIndex(True)
    ref.add_many(w.fbytes, w.foff, 2 + w.fwild)
    row, ids, ex = ref.match(t.tbytes, t.toff, threads=8)
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert sorted(got) == ["exact_id", "filter_id", "n_pairs", "n_words", "row_len", "topics"]
    assert np.array_equal(got["topics"], np.arange(NT))
    assert got["n_pairs"].tolist() == [float(len(ids))] and len(ids) > 0
    assert np.array_equal(got["row_len"], np.diff(row.astype(np.int64)))
    assert np.array_equal(got["filter_id"], ids.astype(np.float64))  # the oracle's rows ascend
    assert np.array_equal(got["exact_id"], ex.astype(np.float64))
    levels = np.array([t.topic(i).count(b"/") + 1 for i in range(NT)])
    assert np.array_equal(got["n_words"], levels)


def test_full_run_adds_the_figures_beside_the_headline():
    """(the legs that take seconds each -- CPU baseline, host pipes, subscribe, concurrent entry --
    switched off by their own options, as the A/B scripts run it)"""
    line = _bench("--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-e2e",
                  "--no-subscribe", "--nif=")
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    cfg, roof = line["config"], line["roofline"]
    assert cfg["pairs_per_batch"] > 0 and cfg["trie_states_per_batch"] > 0
    assert cfg["one_pass_at_a_time"]["ms_per_step"] > 0
    assert set(roof["kernels_ms"]) == {"k_tok", "k_exact", "k_walk", "verify+scan+scatter", "pass"}
    assert roof["kernels_ms"]["pass"] > 0
