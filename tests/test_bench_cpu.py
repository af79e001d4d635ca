"""CPU tests of the multi-rank plumbing of bench.py and of the collective watchdog (no GPU, no process group):
`python3 bench.py --gpus N` as typed starts its ranks as a CHILD job on 127.0.0.1 and relays the exit code; a phase that overruns its
budget ends the process with exit code 124 and one clear line."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_gpus_n_starts_a_child_job_on_loopback(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    class Done:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return Done()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1", "--fp8"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rc = bench.launch_ranks(4)
    cmd = seen["cmd"]
    assert rc == 7                                              # the child's exit code is the parent's
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"   # the container hostname may not resolve
    assert 0 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1", "--fp8"]      # the flags as typed reach every rank
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_main_without_world_size_never_touches_the_gpu_before_launching(monkeypatch):
    """--gpus 2 with WORLD_SIZE unset: main() must hand over to launch_ranks before any device call (a process that initialised HIP
    must not start / exec another program on this pool)."""
    sys.path.insert(0, ROOT)
    import bench
    import torch
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "launch_ranks", lambda n: 3)

    def boom(*a, **k):
        raise AssertionError("device call before the child job was started")

    monkeypatch.setattr(torch.cuda, "set_device", boom)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 3
    else:
        raise AssertionError("main() returned")


def test_watchdog_ends_the_process_with_124_when_a_phase_overruns():
    code = textwrap.dedent(f"""
        import sys, time
        sys.path.insert(0, {ROOT!r})
        from sfron import dp
        wd = dp.Watchdog(rank=3)
        wd.phase("stuck all-reduce", 0.2)
        time.sleep(30)            # the watchdog thread must end the process long before this returns
        print("not reached")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 124
    assert "rank 3" in r.stderr and "stuck all-reduce" in r.stderr and "not reached" not in r.stdout


def test_watchdog_stays_quiet_when_rearmed_and_stopped():
    code = textwrap.dedent(f"""
        import sys, time
        sys.path.insert(0, {ROOT!r})
        from sfron import dp
        wd = dp.Watchdog(rank=0)
        for i in range(4):
            wd.phase("step %d" % i, 1.5)
            time.sleep(0.6)
        wd.stop()
        time.sleep(1.2)
        print("done")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "done" in r.stdout and "watchdog" not in r.stderr


def test_steps_below_one_is_refused(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    try:
        bench.parse()
    except SystemExit as e:
        assert e.code == 2
    else:
        raise AssertionError("--steps 0 accepted")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.steps == 3 and a.dump_outputs == "d"


def test_plain_run_is_lean_unless_full(monkeypatch):
    """What the headline does not need (CPU baseline, other configs, the whole-sweep steps, the dp evidence) runs only with --full."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full", "--no-configs"])
    a = bench.parse()
    assert a.full and a.no_configs and not a.no_cpu_baseline


def test_dump_outputs_writes_float_arrays_of_the_last_step_within_the_cap(tmp_path):
    """--dump-outputs on a stand-in runner (CPU tensors): every array is float32 / float64, the state sample is drawn at the same seeded
    positions on every call, and the whole dump stays under the cap."""
    sys.path.insert(0, ROOT)
    import types

    import numpy as np
    import torch
    import bench
    nt = 3_000_000
    g = torch.Generator().manual_seed(7)
    p, m, v = (torch.randn(nt, generator=g) for _ in range(3))
    ema = torch.randn(nt + 10, generator=g)
    runner = types.SimpleNamespace(opt=types.SimpleNamespace(p=p, m=m, v=v), ema=ema,
                                   model=types.SimpleNamespace(engine=types.SimpleNamespace(n_trainable=nt)), sync_sweep=lambda: None)
    out = {"forget_mse": torch.rand(4), "forget_vb": torch.rand(4), "remain_mse": torch.rand(4), "remain_vb": torch.rand(4),
           "forget_sign": -1.0, "stats": torch.rand(4)}
    a1 = bench.capture_outputs(runner, out)
    a2 = bench.capture_outputs(runner, out)
    info = bench.write_outputs(str(tmp_path / "dump"), a1)
    assert info["bytes"] <= 64 << 20
    want = {"forget_mse", "forget_vb", "remain_mse", "remain_vb", "clip_stats", "state_sample_index", "params_sample", "ema_sample",
            "adam_exp_avg_sample", "adam_exp_avg_sq_sample"}
    assert set(a1) == want and sorted(os.listdir(tmp_path / "dump")) == sorted(n + ".npy" for n in want)
    for n in want:
        x = np.load(tmp_path / "dump" / (n + ".npy"))
        assert x.dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(x, a2[n])
    idx = a1["state_sample_index"].astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and idx.min() >= 0 and idx.max() < nt
    np.testing.assert_array_equal(a1["params_sample"], p.numpy()[idx])
    np.testing.assert_array_equal(a1["ema_sample"], ema.numpy()[idx])
    np.testing.assert_array_equal(a1["adam_exp_avg_sq_sample"], v.numpy()[idx])
    np.testing.assert_array_equal(a1["remain_mse"], out["remain_mse"].numpy())
