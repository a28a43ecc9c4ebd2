"""`python bench.py --gpus N` starts its own rank processes (bench.py launch_ranks; SURVEY.md section 8e: one process per GPU, the
reference itself selects a single device, cli/util.py:56-64).

CPU: the launcher is driven with `--dry-run` workers (gloo, world size 2): rank 0's single line is forwarded and nothing else, a
failing rank's exit code comes back and the surviving rank is ended, RANK in the environment bypasses the launcher.
GPU: `bench.py --gpus 1 --spawn` forces the child path on the one GPU of the box: a parseable line from a fresh rank process under
an RCCL group, `value` within 5 % of the in-process run of the same command, both with the hardware queues bench.py asks for."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'LOCAL_WORLD_SIZE')}
    env['MASTER_ADDR'] = '127.0.0.1'
    return env


def _run(args, timeout=240, env=None):
    return subprocess.run([sys.executable, BENCH] + args, env=env or _env(), capture_output=True, text=True, timeout=timeout)


@pytest.mark.timeout(300)
def test_launcher_forwards_rank0_line_only():
    r = _run(['--gpus', '2', '--dry-run'])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout                       # rank 1's stdout text went to stderr, gloo's banner too
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['dry_run'] is True and out['value'] is None
    assert out['config']['ranks_seen'] == 2                # the all-reduce of ones over the group the launcher's environment set up
    assert 'must not reach' in r.stderr


@pytest.mark.timeout(300)
def test_launcher_propagates_a_failing_rank():
    r = _run(['--gpus', '2', '--dry-run', '--dry-run-fail-rank', '1'])
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == ''                          # no line for a job that did not complete on every rank
    assert 'rank 1 exited with code 3' in r.stderr
    r = _run(['--gpus', '2', '--dry-run', '--dry-run-fail-rank', '0'])
    assert r.returncode == 3 and r.stdout.strip() == ''


@pytest.mark.timeout(300)
def test_spawn_at_world_one_and_launcher_bypass_under_a_launcher():
    r = _run(['--gpus', '1', '--spawn', '--dry-run'])
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout)['config']['ranks_seen'] == 1
    # RANK set by an outer launcher (torch.distributed.run): this process IS a rank; a world-size mismatch is refused, not relaunched
    env = dict(_env(), RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_PORT='29533')
    r = _run(['--gpus', '2', '--dry-run'], env=env)
    assert r.returncode == 2 and r.stdout.strip() == ''


@pytest.mark.timeout(300)
def test_launcher_times_out_on_a_stuck_rank():
    """A rank that never reaches the rendezvous (what a rank stuck in RCCL init looks like): after --launch-timeout the launcher names
    the ranks that are still running, ends them by PID and returns 124 -- no line, no endless wait."""
    import time
    t0 = time.time()
    r = _run(['--gpus', '2', '--dry-run', '--dry-run-hang-rank', '1', '--launch-timeout', '8'], timeout=120)
    assert r.returncode == 124, (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == ''
    assert 'still running after 8 s' in r.stderr and '[0, 1]' in r.stderr      # rank 0 waits for rank 1 in the rendezvous: both are named
    assert time.time() - t0 < 90


@pytest.mark.timeout(300)
def test_launcher_drains_a_long_rank0_line():
    """Rank 0's line may be longer than a pipe buffer (64 KiB): the launcher reads it while the ranks run."""
    env = dict(_env(), COCR_BENCH_DRYRUN_PAD='200000')
    r = _run(['--gpus', '2', '--dry-run'], env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) > 200000
    assert json.loads(lines[0])['config']['ranks_seen'] == 2


@pytest.mark.timeout(120)
def test_launcher_refuses_more_gpus_than_visible():
    import torch
    n = torch.cuda.device_count() + 1
    r = _run(['--gpus', str(max(n, 2)), '--steps', '1', '--warmup', '0'])
    assert r.returncode == 2 and r.stdout.strip() == ''
    assert 'GPU(s) are visible' in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_forced_spawn_on_the_gpu_matches_the_in_process_run():
    # bench.py sets GPU_MAX_HW_QUEUES=8 (one hardware queue per batch in flight) only where the caller has not set it.  With a
    # caller's 4 the two launch paths measured 34.6 k (in-process) against 43.5 k lines/s (rank process under RCCL), and 43.7 k
    # in-process with 8: the comparison is of the launch paths, so both runs get the setting bench.py asks for.
    env = dict(_env(), GPU_MAX_HW_QUEUES='8')
    args = ['--gpus', '1', '--steps', '100', '--warmup', '10', '--full', '--no-cpu-baseline', '--no-extra-legs', '--profile-steps', '0']
    a = _run(args, timeout=420, env=env)
    assert a.returncode == 0, a.stderr[-3000:]
    b = _run(args + ['--spawn'], timeout=420, env=env)
    assert b.returncode == 0, b.stderr[-3000:]
    la, lb = [ln for ln in a.stdout.splitlines() if ln.strip()], [ln for ln in b.stdout.splitlines() if ln.strip()]
    assert len(la) == 1 and len(lb) == 1
    ja, jb = json.loads(la[0]), json.loads(lb[0])
    assert jb['n_gpus'] == 1 and jb['config']['rccl_ranks_seen'] == 1 and jb['config']['launched_by'] == 'bench.py launch_ranks'
    assert ja['config']['launched_by'] == 'in-process'
    assert ja['config']['gpu_max_hw_queues'] == jb['config']['gpu_max_hw_queues'] == '8'
    assert jb['cer_vs_reference'] == 0.0 and ja['cer_vs_reference'] == 0.0
    print('in-process', ja['value'], 'spawned', jb['value'])
    assert abs(jb['value'] - ja['value']) <= 0.05 * ja['value'], (ja['value'], jb['value'])


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location('cocr_bench', BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_and_samples_large_logits(tmp_path, monkeypatch):
    import numpy as np
    import torch
    bench = _bench_module()
    logits = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    recs = [[(5, 0, 1, 0.5)], [(7, 1, 2, 0.25), (9, 2, 2, 0.75)]]
    bench.dump_outputs(str(tmp_path / 'a'), logits, np.array([3, 2], dtype=np.int32), recs)
    a = {f.stem: np.load(f) for f in (tmp_path / 'a').iterdir()}
    assert sorted(a) == ['logits', 'out_lens', 'records']
    assert a['logits'].dtype == np.float32 and np.array_equal(a['logits'], logits.numpy())
    assert a['out_lens'].dtype == np.float64 and a['out_lens'].tolist() == [3.0, 2.0]
    assert a['records'].dtype == np.float64 and a['records'].tolist() == [[0, 5, 0, 1, 0.5], [1, 7, 1, 2, 0.25], [1, 9, 2, 2, 0.75]]
    # logits above the budget: the same seeded sample on every call
    monkeypatch.setattr(bench, 'DUMP_LOGITS_MAX_BYTES', 48)
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), logits, np.array([3, 2], dtype=np.int32), [[], []])
    b = {f.stem: np.load(f) for f in (tmp_path / 'b').iterdir()}
    c = {f.stem: np.load(f) for f in (tmp_path / 'c').iterdir()}
    assert sorted(b) == ['logits_sample', 'logits_sample_index', 'out_lens', 'records']
    assert b['logits_sample'].dtype == np.float32 and b['logits_sample_index'].dtype == np.float64 and len(b['logits_sample']) == 4
    assert np.array_equal(b['logits_sample'], logits.numpy().reshape(-1)[b['logits_sample_index'].astype(np.int64)])
    assert all(np.array_equal(b[k], c[k]) for k in b) and b['records'].shape == (0, 5)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    import numpy as np
    outs = []
    for d in ('a', 'b'):
        r = _run(['--gpus', '1', '--steps', '7', '--warmup', '2', '--dump-outputs', str(tmp_path / d)], timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1
        outs.append(json.loads(lines[0]))
    j = outs[0]
    assert j['steps'] == 7 and j['warmup'] == 2 and j['ms_per_step'] > 0 and j['value'] > 0
    assert j['unit'] == 'lines/s' and j['higher_is_better'] is True and j['dtype'] == 'bf16'
    assert j['cpu_baseline'] is None and j['roofline'] is None and j['cer'] is None and j['other_configs'] is None   # --full's legs
    a = {f.stem: np.load(f) for f in (tmp_path / 'a').iterdir()}
    b = {f.stem: np.load(f) for f in (tmp_path / 'b').iterdir()}
    assert sorted(a) == ['logits', 'out_lens', 'records'] and sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a['logits'].dtype == np.float32 and a['logits'].shape == (32, 300, 128) and np.isfinite(a['logits']).all()
    assert a['out_lens'].tolist() == [300.0] * 32
    assert len(a['records']) == j['labels_emitted_last_step'] > 0
    assert all(np.array_equal(a[k], b[k]) for k in a)                 # same arguments, same inputs, same outputs
