"""The committed bench lines and the PMC profiles they may quote (profiles/r03_*, profiles/r05_*): the driver's contract
keys, a roofline fraction that is a fraction, and the rule that HBM traffic measured by rocprofv3 is
only ever attached to a build whose kernel sources hash to the profile's."""
import json
import os
import re

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the round whose final collection is tied to the committed kernel sources (earlier rounds' files are history)
LATEST = "r06" if os.path.exists(os.path.join(ROOT, "profiles", "r06_pmc_plane_down.json")) else None
ROUNDS = ["r03", "r05"] + (["r06"] if LATEST else [])


def _load(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        return json.loads(f.read().strip().splitlines()[-1]) if name.endswith("bench.json") else json.load(f)


@pytest.mark.parametrize("rnd", ROUNDS)
def test_committed_bench_line_keeps_the_contract(rnd):
    d = _load(rnd + "_bench.json")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "V-cycles/s" and d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-3          # value = steps / time of exactly those steps
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert 0.0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(r["achieved"] - r["bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) / r["achieved"] < 1e-2
    assert r["csr_equiv_bytes"] > r["bytes_per_launch"]                          # the CSR-byte rate is reported, never used for frac
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["unit"] == "V-cycles/s" and c["value"] > 0 and c["sample"]
    assert d["csr_path"]["residual"]["frac"] <= 1.0 and d["csr_path"]["fine_grid_spmv"]["frac"] <= 1.0
    assert all(d["config"]["plane_levels"]) and d["set_schedule"]["vcycles_per_s"] < d["value"]
    for k in ("plane_down", "plane_up"):
        assert 0.0 < r["level0_kernels"][k]["frac"] <= 1.0 and r["level0_kernels"][k]["launches_per_cycle"] == 1.0
    assert d["reference_smoother"]["vcycles_per_s"] > 0 and all(d["reference_smoother"]["wavefront_levels"])
    assert re.fullmatch(r"[0-9a-f]{16}", d["config"]["kernel_src_sha"]) and re.fullmatch(r"[0-9a-f]{40}", d["config"]["git_head"])
    if rnd >= "r05":
        # round 5's legs: the matrix-free fine-grid SpMV over the line VERDICT r4 drew, BASELINE configs[0] and [4] (the latter
        # with its own roofline and the coefficient update), which kind of allocation the finest level's vectors got
        assert 0.70 <= d["fine_grid_spmv"]["frac"] <= 1.0
        assert d["config0"]["vcycles_per_s"] > 1500 and d["config0"]["grids"] == 3
        c4 = d["config4"]
        assert c4["stencil27_kernels"] and 0.0 < c4["roofline"]["frac"] <= 1.0 and c4["dtype"] == "f32"
        assert c4["update_fine_device_ms"] is not None and c4["update_fine_device_ms"] < c4["update_fine_device_plus_cycle_ms"] < 20.0
        assert d["config"]["process_population"]["which"] in ("fast", "slow")
        assert d["default_cycle"]["plane"] and d["default_cycle"]["vcycles_per_s"] > 0


@pytest.mark.parametrize("rnd", ROUNDS)
def test_pmc_traffic_is_tied_to_the_kernel_sources_it_was_measured_on(rnd):
    p = _load(rnd + "_pmc_plane_down.json")
    assert re.fullmatch(r"[0-9a-f]{16}", p["kernel_src_sha"]) and re.fullmatch(r"[0-9a-f]{40}", p["git_head_at_collection"])
    assert p["traffic_bytes"] == p["read_bytes"] + p["write_bytes"]
    assert abs(p["read_bytes"] - 2 * p["fetch_size_KiB"] * 1024) < 1024          # gfx950: reads = 2 x FETCH_SIZE
    assert p["traffic_bytes"] >= p["bytes_per_launch"]                           # over-fetch, never under
    h = bench.kernel_source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", h) and h == bench.kernel_source_hash()
    if rnd == LATEST:
        # the round's final collection was made on the sources as they are committed: the profiles are this build's
        assert h == p["kernel_src_sha"], "openmg_amd/csrc changed after the round's profiles were collected"
        q = _load(rnd + "_pmc_s27_sweep.json")
        assert q["kernel_src_sha"] == h and q["traffic_bytes"] == q["read_bytes"] + q["write_bytes"]
    d = _load(rnd + "_bench.json")
    if d["roofline"]["traffic"] is not None:                                     # only a run of the profiled build may carry it
        # (the line quotes the PMC passes that were committed when it ran; the profile next to it may be a
        # later collection on the same sources: FETCH_SIZE varies by a few hundred bytes from pass to pass)
        assert d["config"]["kernel_src_sha"] == p["kernel_src_sha"]
        assert abs(d["roofline"]["traffic"] - p["traffic_bytes"]) <= 1e-3 * p["traffic_bytes"]
        assert "NOT measured in this run" in d["roofline"]["traffic_source"]


def test_dump_outputs_are_float_arrays_within_the_budget_and_the_same_sample_every_run(tmp_path):
    """--dump-outputs: x.npy and residual_norm.npy in float32 / float64, 64 MB at most in all; an iterate above the budget
    as the entries at one fixed, sorted set of positions (two runs: the same file), a small one whole."""
    import numpy as np
    x = np.arange(3 * bench.DUMP_BYTES // 8 + 5, dtype=np.float64)           # entry i holds i: the positions written
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), x, 0.25)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["residual_norm.npy", "x.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= 64e6
    got = np.load(str(tmp_path / "a" / "x.npy"))
    assert got.dtype == np.float64 and got.size == bench.DUMP_BYTES // 8
    assert np.all(np.diff(got) > 0) and got[0] >= 0 and got[-1] < x.size
    assert np.array_equal(got, np.load(str(tmp_path / "b" / "x.npy")))
    assert np.load(str(tmp_path / "a" / "residual_norm.npy")).tolist() == [0.25]
    small = np.random.default_rng(3).random(1000).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "c"), small, 1.5)
    got = np.load(str(tmp_path / "c" / "x.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, small)


@pytest.mark.gpu
def test_dump_outputs_hold_the_iterate_and_norm_of_the_last_timed_cycle(tmp_path):
    """`bench.py --dump-outputs DIR` at 32^3: x.npy and residual_norm.npy have the bits of the same warm-up and timed cycles
    run here on a hierarchy of bench.py's problem; the line counts exactly --steps cycles per timed region."""
    import subprocess
    import sys
    import numpy as np
    from openmg_amd import _hip, operators
    size, grids, steps, warmup, repeats = 32, 3, 3, 2, 2
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(size), "--grids", str(grids),
                        "--steps", str(steps), "--warmup", str(warmup), "--repeats", str(repeats), "--no-cpu", "--no-plain",
                        "--no-sets", "--no-lex", "--no-dropin", "--no-config4", "--no-config1", "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and len(d["config"]["ms_per_step_all"]) == repeats
    shape = (size,) * 3
    A0 = operators.stencil_poisson(shape)
    b = A0 @ np.random.default_rng(12345).random(A0.shape[0])
    R = operators.restrictionList(shape, grids - 2, 8)
    with _hip.Hierarchy(operators.coeffecientList(A0, R), R, smoother="colour") as h:
        h.resident_load(b)
        h.resident_cycles(1, 1, warmup)
        for _ in range(repeats):
            norms = h.resident_cycles(1, 1, steps)
        x = h.resident_fetch()
    got = np.load(str(tmp_path / "x.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, x), int(np.sum(got != x))
    assert np.load(str(tmp_path / "residual_norm.npy")).tolist() == [norms[-1]]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_full_adds_the_legs():
    """A plain run at 32^3 measures nothing after its timed regions: the legs, the roofline and the CPU baseline are null.
    The same run with --full (configs[1] / [4] left out, the CPU baseline at 32^3) fills them in."""
    import subprocess
    import sys
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "32", "--grids", "3", "--steps", "3",
            "--warmup", "2", "--repeats", "3"]
    legs = ("roofline", "fine_grid_spmv", "dropin", "csr_path", "reference_smoother", "cpu_baseline")
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-config4", "--no-config1", "--cpu-size", "32", "--cpu-cycles", "1"])):
        p = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, (mode, p.stderr[-3000:])
        lines[mode] = d = json.loads(p.stdout.strip().splitlines()[-1])
        assert d["unit"] == "V-cycles/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 3
        assert abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-3 and len(d["config"]["ms_per_step_all"]) == 3
        assert d["config"]["full"] is (mode == "full")
    plain, full = lines["plain"], lines["full"]
    assert all(plain[k] is None for k in legs + ("set_schedule", "default_cycle", "config0", "config1", "config4", "var7"))
    assert plain["config"]["final_residual_norm"] is None and plain["config"]["setup_device_s"] is None
    assert all(isinstance(full[k], dict) for k in legs), [k for k in legs if not isinstance(full[k], dict)]
    assert full["roofline"]["level0_kernels"] and full["cpu_baseline"]["value"] > 0 and full["config"]["final_residual_norm"] > 0
