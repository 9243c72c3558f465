"""bench.py's JSON line (the driver's contract, BASELINE.json's metric) and
its algorithmic figures.  The CPU tests pin the closed forms of SURVEY.md 8d;
the GPU test runs one short bench and checks every field the driver and the
judge read (a subprocess, as the driver runs it)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_algorithmic_bytes_match_the_survey():
    # in 8 (28N + 25), out 8 (18N + 13) + 4
    for N, total in ((10, 3988), (20, 7668), (60, 22388)):
        assert bench.algorithmic_bytes(N) == 8 * (28 * N + 25) + 8 * (18 * N + 13) + 4 == total


def test_workload_labels_name_the_baseline_configs():
    class A:   # bench.parse() defaults, then per config
        variant, N, straight, mu_sweep, precision, refine, batch, global_batch = '3f', 10, False, False, 'f64', 5, 65536, 0
    a = A()
    assert bench.workload_label(a, 1).startswith('configs[2]')
    a.precision = 'f32'
    assert bench.workload_label(a, 1).startswith('configs[4]')
    a.precision, a.variant, a.straight, a.batch = 'f64', '2f', True, 4096
    assert bench.workload_label(a, 1).startswith('configs[1]')
    a.variant, a.N, a.mu_sweep, a.global_batch = '3f', 20, True, 262144
    assert bench.workload_label(a, 8).startswith('configs[3]') and 'strong' in bench.workload_label(a, 8)


@pytest.mark.gpu
def test_bench_line_contract():
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--prewarm-ms', '100',
           '--full', '--cpu-seconds', '1', '--batch', '4096']
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'prewarm_ms', 'prewarm_steps'):
        assert k in d, k
    assert d['metric'] == bench.METRIC and d['unit'] == 'QP solves/s' and d['value'] > 0
    assert (d['n_gpus'], d['steps'], d['warmup']) == (1, 3, 1)
    assert d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert d['dtype'] == 'f64' and d['config']['workload'].startswith('configs[2]')
    assert abs(d['value'] - 4096 / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
    r = d['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in r, k
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-12
    c = d['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in c, k
    assert c['kind'] == 'port' and c['value'] > 0
    assert d['prewarm_ms'] >= 100 and d['prewarm_steps'] > 0
    p = d['parity_sample']
    assert p['instances'] > 0 and p['max_abs_du_vs_port'] <= 1e-6 and p['status_mismatch_total'] == 0


@pytest.mark.gpu
def test_plain_run_skips_the_baseline_and_dumps_its_outputs(tmp_path):
    """Without --full: no CPU baseline, no parity sample.  --dump-outputs writes the last
    step's outputs as float64 .npy, the same from run to run of one build (seeded inputs)."""
    import numpy as np
    B, N = 1024, 10
    dumps = []
    for name in ('a', 'b'):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
               '--prewarm-ms', '0', '--batch', str(B), '--dump-outputs', str(tmp_path / name)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1, out.stdout
        d = json.loads(lines[0])
        assert d['cpu_baseline'] is None and d['parity_sample'] is None
        assert d['steps'] == 2 and d['metric'] == bench.METRIC and d['dtype'] == 'f64'
        assert abs(d['value'] - B / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
        dumps.append({f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    a, b = dumps
    shapes = {'u': (B, N, 6), 'x': (B, N + 1, 12), 'obj': (B,), 'status': (B,), 'iters': (B,), 'active': (B,),
              'index': (B,)}
    assert {k: v.shape for k, v in a.items()} == shapes
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a['index'], np.arange(B)) and (a['status'] == 0).mean() > 0.9
    for k in shapes:
        assert np.array_equal(a[k], b[k]), k


def test_dump_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    """A batch above the byte budget is dumped as a seeded sample of instances (CPU tensors here)."""
    import numpy as np
    torch = pytest.importorskip('torch')
    assert bench.DUMP_BYTES + 7 * 128 <= 64_000_000   # the budget, plus the .npy headers
    monkeypatch.setattr(bench, 'DUMP_BYTES', 100_000)
    B = 1000   # 62 doubles each: 496 kB, five times the budget
    out = dict(u=torch.arange(B * 60, dtype=torch.float64).reshape(B, 10, 6), obj=torch.arange(B, dtype=torch.float64))
    for name in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / name), out, 0, 1)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['index.npy', 'obj.npy', 'u.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) - 128 for f in files) <= 100_000
    idx = np.load(tmp_path / 'a' / 'index.npy').astype(np.int64)
    assert len(idx) == 100_000 // (8 * 62) and (np.diff(idx) > 0).all() and idx[-1] < B
    assert np.array_equal(np.load(tmp_path / 'a' / 'obj.npy'), idx.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / 'a' / 'u.npy')[:, 0, 0], 60.0 * idx)
    for f in files:
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)), f
