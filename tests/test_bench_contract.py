"""bench.py's output contract: exactly one JSON line on stdout with the agreed keys, the headline ones in a plain run and
all of them with --full (GPU, smallest config)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config", "full")
FULL_ONLY_KEYS = ("roofline", "value_without_row_classes", "value_with_odd_rows", "v22_cycles_per_s", "residual_l2_after",
                  "rhs_l2", "cpu_baseline")


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_line_only():
    """Without --full: one JSON line with the headline keys saying what they say in a --full run, and none of the
    figures that take runs of their own."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--steps", "3",
                          "--warmup", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[:2000]
    d = json.loads(lines[0])
    for key in HEADLINE_KEYS:
        assert key in d, key
    for key in FULL_ONLY_KEYS:
        assert key not in d, key
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["unit"] == "V-cycles/s" and d["dtype"] == "f64"
    assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 1000.0) < 1e-6 * 1000.0
    assert "workload" in d["config"] and d["setup_s"] > 0 and d["device_memory_GB_per_gpu"] > 0


class _RecordingHierarchy:
    """Stands in for the device hierarchy: records every call, and knows only the calls a plain run may make."""

    def __init__(self):
        self.calls = []

    def sync(self):
        self.calls.append(("sync",))

    def zero_vector(self, level, name):
        self.calls.append(("zero_vector", level, name))

    def vcycle(self, level, n):
        self.calls.append(("vcycle", level, n))

    def memory_bytes(self):
        self.calls.append(("memory_bytes",))
        return 1 << 20

    def device_info(self):
        self.calls.append(("device_info",))
        return "stub"

    def close(self):
        self.calls.append(("close",))


def test_plain_bench_run_does_only_what_the_headline_needs(monkeypatch, capfd):
    """Without --full the hierarchy sees set-up, the warm-up and the timed cycles, each followed by a wait, and the two
    cheap queries of the result line -- no kernel timing, no tuning switch, no further cycle (CPU: a recording stand-in
    that has no other method); the oracle's CPU cycles do not run either."""
    import bench

    h = _RecordingHierarchy()
    monkeypatch.setattr(bench, "build_hierarchy", lambda args, rv: h)
    monkeypatch.setattr(bench, "cpu_baseline", lambda args: pytest.fail("a plain run timed the CPU baseline"))
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert bench.parse().full is False
    bench.main()
    assert h.calls == [("sync",), ("zero_vector", 7, "v"), ("vcycle", 7, 2), ("sync",), ("vcycle", 7, 4), ("sync",),
                       ("memory_bytes",), ("device_info",), ("close",)]
    lines = [l for l in capfd.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in HEADLINE_KEYS:
        assert key in d, key
    for key in FULL_ONLY_KEYS:
        assert key not in d, key
    assert d["full"] is False and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 1000.0) < 1e-6 * 1000.0


def test_full_bench_run_hands_the_hierarchy_on_after_the_timed_cycles(monkeypatch, capfd):
    """--full: the same set-up, warm-up and timed cycles, then everything else the script measures on the same
    hierarchy, its keys in the one result line (CPU: stand-ins for the hierarchy and for both further legs)."""
    import bench

    h = _RecordingHierarchy()
    monkeypatch.setattr(bench, "build_hierarchy", lambda args, rv: h)
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    seen = []
    monkeypatch.setattr(bench, "full_measurements", lambda args, rv, hh: (seen.append(hh) or {"roofline": {}}, 1 << 20, "stub"))
    monkeypatch.setattr(bench, "cpu_baseline", lambda args: {"value": 1.0})
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", "--full"])
    assert bench.parse().full is True
    bench.main()
    assert seen == [h]
    assert h.calls == [("sync",), ("zero_vector", 7, "v"), ("vcycle", 7, 2), ("sync",), ("vcycle", 7, 4), ("sync",)]
    lines = [l for l in capfd.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is True and d["roofline"] == {} and d["cpu_baseline"] == {"value": 1.0}
    assert d["steps"] == 4 and d["warmup"] == 2 and abs(d["ms_per_step"] * d["value"] - 1000.0) < 1e-6 * 1000.0


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    """--full: the headline keys and everything else the script measures, in one JSON line."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1", "--steps", "3", "--warmup", "1", "--full"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[:2000]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 1000.0) < 1e-6 * 1000.0
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    # the fraction is priced on the bytes the shipped format must stream: it cannot exceed the roofline, and it is
    # reproducible from the line itself
    assert 0.0 < r["frac"] <= 1.0
    assert abs(r["achieved"] - r["format_bytes_per_row"] * r["rows_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["traffic"] is None or r["traffic"] >= r["algorithmic_bytes_per_launch"] * 0.9
    assert "speedup_vs_csr_model" in r and "value_without_row_classes" in d
    assert "value_with_odd_rows" in d and d["value_with_odd_rows"] is None         # (measured on the headline configuration only)
    c = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0


def test_bench_starts_its_own_ranks_when_not_under_a_launcher(monkeypatch, capsys):
    """`python bench.py --gpus N` with WORLD_SIZE unset: the parent never touches a GPU, it starts
    `python -m torch.distributed.run ... bench.py <same arguments>` as a child process, relays rank 0's JSON line and
    returns the child's exit code (CPU: the child is replaced by a stub)."""
    import io
    import bench

    seen = {}

    class FakeProc:
        def __init__(self, cmd, stdout=None, env=None):
            seen["cmd"], seen["env"] = cmd, env
            self.stdout = io.BytesIO(b"NCCL version banner\n" + b'{"metric": "m", "value": 1.0, "n_gpus": 4}\n')

        def wait(self):
            return seen.get("rc", 0)

    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2", "--warmup", "1"])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-7:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    assert [l for l in out.out.splitlines() if l.strip()] == ['{"metric": "m", "value": 1.0, "n_gpus": 4}']
    assert "NCCL version banner" in out.err
    # a failing child: its exit code comes back, and a child that printed no line is a failure too
    seen["rc"] = 3
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 3


@pytest.mark.gpu
def test_bench_with_two_ranks_starts_itself():
    """`python bench.py --gpus 2` without a launcher, two ranks sharing the one GPU through the host-staged gloo
    transport (the RCCL transport needs one GPU per rank): one JSON line, n_gpus 2, strong scaling."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c3", "--transport", "gloo",
                          "--mu", "2", "--steps", "2", "--warmup", "1", "--kernel-reps", "2", "--full"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[:2000]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["parallelism"].startswith("slab2")
    assert d["residual_l2_after"] < d["rhs_l2"]


def test_dump_sample_is_fixed_and_within_the_budget():
    """--dump-outputs writes small outputs whole and a fixed seeded sample of large ones: sorted distinct indices, the
    same from run to run, values and float64 indices together within 64 MB."""
    import numpy as np
    import bench

    assert bench.output_sample(4225) is None
    assert bench.output_sample(bench.DUMP_BYTES // 8) is None
    n = 1025 ** 3
    idx = bench.output_sample(n)
    assert np.array_equal(idx, bench.output_sample(n))
    assert idx.dtype == np.int64 and idx[0] >= 0 and idx[-1] < n and np.all(np.diff(idx) > 0)
    assert 16 * idx.size <= bench.DUMP_BYTES and idx.size > bench.DUMP_BYTES // 40
    assert np.array_equal(idx.astype(np.float64).astype(np.int64), idx)


@pytest.mark.gpu
def test_bench_dumps_what_the_timed_cycles_computed(tmp_path):
    """--dump-outputs DIR: the finest level's iterate after the warm-up and the timed V-cycles, float64, equal to the
    same cycles run through the library directly; the JSON line is unchanged."""
    import numpy as np
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1", "--steps", "2", "--warmup", "1",
                          "--kernel-reps", "2", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and json.loads(lines[0])["steps"] == 2
    assert sorted(os.listdir(tmp_path / "dump")) == ["v.npy"]
    got = np.load(tmp_path / "dump" / "v.npy")
    assert got.dtype == np.float64 and got.shape == (65 * 65,) and np.all(np.isfinite(got))
    with DeviceHierarchy.synthetic(2, 1, 3, c=8, mu1=50, mu2=50, omega=2.0 / 3.0, prune_zeros=True) as h:
        h.zero_vector(3, "v")
        h.vcycle(3, 1)
        h.vcycle(3, 2)
        want = h.get_vector(3, "v").ravel()
    assert np.linalg.norm(want) > 0
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
