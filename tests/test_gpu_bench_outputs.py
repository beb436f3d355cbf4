"""bench.py's plain run and --dump-outputs: the plain line holds the headline and nothing that takes runs of its own, --steps is the
number of timed steps, and the dumped outputs are the timed path's results -- the same from run to run and from one rank to two,
and bit-equal to the oracle on the first samples' block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pair_i", "pair_j", "d", "nn", "p_direct", "expected_k")


def _bench(args, env_extra=None, timeout=600):
    env = dict(os.environ, **(env_extra or {}))
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                         timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    got = {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in NAMES)
    assert all(a.dtype == np.float64 and a.ndim == 1 and len(a) == len(got["d"]) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    return got


def test_plain_line_and_dump_outputs(tmp_path):
    n, L = 700, 200000
    size = ["--samples", str(n), "--sites", str(L)]
    j = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")] + size)
    assert j["metric"].startswith("sample-pairs/sec") and j["unit"] == "pairs/s" and j["higher_is_better"] is True and j["dtype"] == "u32"
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0
    assert abs(j["value"] - n * (n - 1) / 2 / (j["ms_per_step"] / 1e3)) < 1e-6 * j["value"]
    # nothing that takes runs of its own (those are --full's)
    assert not {"value_steady_state", "single_pass", "roofline", "roofline_per_pack", "sensitivity", "filter", "roofline_general",
                "dm_frontend", "cpu_baseline"} & set(j)
    a = _load(tmp_path / "a")
    iu = np.triu_indices(n, 1)                                  # fewer pairs than the sample: every pair, row-major
    assert np.array_equal(a["pair_i"], iu[0]) and np.array_equal(a["pair_j"], iu[1])
    assert a["d"].sum() == j["config"]["checksum_d"]
    assert np.all((a["p_direct"] >= 0) & (a["p_direct"] <= 1)) and np.all(np.isfinite(a["expected_k"]))
    # the first samples' block against the oracle, bit-equal
    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle as O
    from tracs_amd import synth
    m = 48
    seqs = synth.first_samples_host(n, L, 20241022 + 2, m, **bench.synth_kw(0.0, "sparse"))
    r, c, d, nn = O.pairsnp_planes(O.pack(seqs), L)
    sel = (a["pair_i"] < m) & (a["pair_j"] < m)
    assert np.array_equal(a["pair_i"][sel], r.astype(np.float64)) and np.array_equal(a["pair_j"][sel], c.astype(np.float64))
    assert np.array_equal(a["d"][sel], d.astype(np.float64)) and np.array_equal(a["nn"][sel], nn.astype(np.float64))
    # another run with another number of steps: the same inputs, the same outputs
    j2 = _bench(["--gpus", "1", "--steps", "3", "--warmup", "0", "--dump-outputs", str(tmp_path / "b")] + size)
    assert j2["steps"] == 3 and j2["warmup"] == 0
    b = _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)


def test_dump_outputs_of_two_site_shards_equal_one_rank(tmp_path):
    """--gpus 2 (two gloo ranks sharing the GPU, site partition: every rank owns some rows of the results) dumps what one rank does."""
    size = ["--samples", "1501", "--sites", "100000", "--steps", "2", "--warmup", "1"]
    one = _bench(["--gpus", "1", "--dump-outputs", str(tmp_path / "one")] + size)
    two = _bench(["--gpus", "2", "--partition", "sites", "--dump-outputs", str(tmp_path / "two")] + size, {"TRACS_BENCH_BACKEND": "gloo"})
    assert two["n_gpus"] == 2 and two["config"]["checksum_d"] == one["config"]["checksum_d"]
    a, b = _load(tmp_path / "one"), _load(tmp_path / "two")
    i, j = a["pair_i"], a["pair_j"]                             # more pairs than the sample: a seeded sample of them, row-major
    assert len(i) == 1 << 20 and np.all(i < j) and j.max() < 1501
    assert np.all(np.diff(i * 1501 + j) > 0)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
