"""CPU: the LAUNCH path of bench.py.  `python bench.py --gpus N` is the driver's command shape; without a launcher in the
environment it must start its N ranks itself (it died on an assert).  Run here as a real subprocess with
--dry-run 1 (CPU tensors, the type-checking stub of the C ABI, gloo): self-launch -> torch.distributed.run -> process group ->
reducer -> rank 0 prints exactly one JSON line.  The numbers in that line are meaningless by construction."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--dry-run', '1', '--steps', '2', '--warmup', '1'] + extra      # a later --steps wins
    return subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def test_bench_gpus_2_launches_its_own_ranks_and_prints_one_line():
    r = _run(['--gpus', '2'])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['config']['parallelism'] == 'dp2' and out['config']['global_batch'] == 2 * out['config']['per_gpu_batch']
    dp = out['data_parallel']
    assert dp['rccl_ranks_seen'] == 2 and dp['backend'] == 'gloo' and dp['buckets'] >= 2
    assert dp['gemm_cu_reserved'] == 16                 # the persistent GEMM grids leave CUs to the collective while buckets fly
    assert 'DRY RUN' in out['data']
    assert 'without a launcher' in r.stderr


def test_bench_single_rank_dry_run_line_keeps_the_contract():
    r = _run(['--gpus', '1'])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data',
              'config', 'roofline', 'cpu_baseline'):
        assert k in out, k
    assert out['n_gpus'] == 1 and 'data_parallel' not in out


def test_bench_refuses_a_launcher_environment_that_disagrees_with_gpus():
    r = _run(['--gpus', '2'], env_extra=dict(WORLD_SIZE='1', RANK='0', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='29541'), timeout=300)
    assert r.returncode != 0 and 'must agree' in r.stderr


def test_bench_dump_outputs_writes_the_last_step_as_float_arrays(tmp_path):
    """--dump-outputs DIR: the last timed step's losses, masks, predictions and updated parameters as float32 / float64 .npy
    files, 64 MiB at most in all; the line's `steps` / `ms_per_step` are those of the timed loop."""
    import numpy as np
    out_dir = tmp_path / 'dump'
    r = _run(['--gpus', '1', '--steps', '3', '--dump-outputs', str(out_dir)])
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert out['steps'] == 3 and out['ms_per_step'] > 0
    names = sorted(p.name for p in out_dir.iterdir())
    doms, tasks = ['depth', 'rgb', 'semseg'], ['depth', 'norm_rgb', 'rgb', 'semseg']
    assert names == sorted(['loss_total.npy', 'params.npy'] + [f'loss_{t}.npy' for t in tasks] + [f'mask_{d}.npy' for d in doms]
                           + [f'pred_{t}.npy' for t in tasks]), names
    total = 0
    for n in names:
        a = np.load(out_dir / n)
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        total += a.nbytes
    assert np.load(out_dir / 'mask_rgb.npy').shape == (2, 196)
    assert total <= 64 << 20, total


def _main_with_recorded_runs(monkeypatch, argv):
    """bench.main() on `argv` with run_once replaced by a recorder: the arguments of every measured configuration, and the line."""
    import copy
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    runs = []

    def run_once(a):
        runs.append(copy.copy(a))
        return {k: a.config for k in ('metric', 'value', 'unit', 'ms_per_step', 'steps', 'warmup', 'dtype', 'config', 'final_loss', 'roofline')}
    monkeypatch.setattr(bench, 'run_once', run_once)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    bench.main()
    return runs


def test_bench_plain_run_measures_the_timed_steps_alone(monkeypatch, capsys):
    """Without --full: one measured configuration, no kernel timing pass, no CPU baseline, no secondary lines."""
    runs = _main_with_recorded_runs(monkeypatch, ['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert len(runs) == 1
    a = runs[0]
    assert (a.config, a.precision, a.steps, a.warmup) == ('cfg3', 'bf16', 20, 5)
    assert a.no_kernel_timing and a.no_cpu_baseline and a.no_secondary
    out = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][0])
    assert not any(k.startswith('secondary') for k in out)


def test_bench_full_run_keeps_every_extra_measurement(monkeypatch, capsys):
    """--full: the primary line with the kernel timing pass and the CPU baseline, then the cfg5 MX-fp8, x3-adapter and cfg2 lines."""
    runs = _main_with_recorded_runs(monkeypatch, ['--gpus', '1', '--steps', '20', '--warmup', '5', '--full'])
    assert [(a.config, a.steps, a.warmup) for a in runs] == [('cfg3', 20, 5), ('cfg5', 5, 2), ('cfg3', 10, 3), ('cfg2', 10, 3)]
    assert not runs[0].no_kernel_timing and not runs[0].no_cpu_baseline
    assert runs[1].precision == 'mxfp8' and not runs[1].no_kernel_timing and runs[2].fp32_adapter_gemm == 'x3'
    out = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][0])
    assert out['secondary']['config'] == 'cfg5' and out['secondary_x3_adapter']['config'] == 'cfg3' and out['secondary_cfg2']['config'] == 'cfg2'
    # the opt-outs keep working under --full
    runs = _main_with_recorded_runs(monkeypatch, ['--full', '--no-cpu-baseline', '--no-secondary'])
    assert len(runs) == 1 and runs[0].no_cpu_baseline and not runs[0].no_kernel_timing


def test_bench_refuses_zero_steps():
    r = _run(['--gpus', '1', '--steps', '0'], timeout=300)
    assert r.returncode != 0 and '--steps' in r.stderr
