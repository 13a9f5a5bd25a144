"""not-gpu: bench.py's control flow end to end with the device API replaced by stand-ins — argument defaults, launch
grouping, the pipelined enqueue order per stream, the second (timed) pass and the JSON contract.  The numbers are
meaningless here; what is checked is that every step count is honoured and the line has every required field."""
import importlib
import json
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"]


class FakeJob:
    log = []

    def __init__(self, ctx, n_windows, t0=0):
        self.ctx, self.n_windows, self.state = ctx, n_windows, "new"
        self.n_targets, self.t0 = n_windows // 4, t0

    def featurize(self):
        FakeJob.log.append(("F", id(self)))
        self.state = "featurized"

    def infer(self, batch, mode):
        assert self.state == "featurized", "infer before featurize"
        FakeJob.log.append(("I", id(self)))
        self.state = "inferred"

    def consensus(self):
        assert self.state == "inferred"
        FakeJob.log.append(("C", id(self)))
        self.state = "done"

    def consensus_fetch(self):
        assert self.state == "done", "fetch before consensus"
        FakeJob.log.append(("D", id(self)))
        return 4000 * self.n_windows

    def close(self):
        pass

    def logits(self, w):   # a function of the job's data (its first target) and the window: the same inputs give the same logits
        assert self.state == "done"
        n = (self.t0 + w) % 5
        return np.full(n, self.t0 + w, np.float32), np.arange(5 * n, dtype=np.float32).reshape(n, 5) + w

    def consensus_fasta(self, t, read_id):
        assert self.state == "done"
        return f">{read_id}\n" + "ACGT"[(self.t0 + t) % 4] * 8 + "\n"

    def stats(self):
        n = self.n_windows
        return {"read_bytes": 169000 * n, "op_bytes": 13000 * n, "out_bytes": 292000 * n, "sum_len": 4711 * n,
                "sum_supported": 15 * n, "n_model_windows": n}


class FakeCtx:
    def __init__(self, dev):
        self.on = False

    def load_model(self, p): pass
    def set_precision(self, m): pass
    def precision(self): return 4
    def clock_probe(self): return 2100.0
    def calibration_error(self, m): return 4.0e-4 if m == 4 else 6.0e-4
    def set_reads(self, *a): pass
    def share_reads(self, other): assert isinstance(other, FakeCtx)
    def synchronize(self): pass
    def timing_enable(self, on=True): self.on = on
    def timing_reset(self): pass
    def close(self): pass

    def timing(self):
        names = ["cols", "win", "layout", "tokens", "supgather", "rf_quals",
                 "build_tokens", "conv_fused", "fc_gemm", "add_pe", "layers_fused", "consensus"]
        return {n: (1.0 + i, 4) for i, n in enumerate(names)}


@pytest.mark.parametrize("argv,steps,strong_mode", [(["--steps", "12", "--warmup", "4", "--group", "3", "--streams", "2"], 12, "ok"),
                                                    (["--steps", "7", "--warmup", "1", "--group", "32", "--streams", "2"], 7, "ok"),
                                                    (["--steps", "1", "--warmup", "0"], 1, "ok"),
                                                    (["--steps", "3", "--warmup", "0", "--precision", "6", "--sustained", "0.05"], 3, "ok"),   # the e4m3-remainder mode has its dtype / MFMA-terms entries
                                                    ([], None, "ok"),
                                                    (["--steps", "2", "--warmup", "0"], 2, "raises"),
                                                    (["--steps", "2", "--warmup", "0", "--strong-timeout", "0.3"], 2, "hangs")])
def test_bench_flow(monkeypatch, capsys, argv, steps, strong_mode):
    import torch
    from herro_amd import api, synth, model_io
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(api, "Context", FakeCtx)
    made = []

    def fake_job_from_synth(ctx, sb, W, targets=None):
        ts = list(targets)
        j = FakeJob(ctx, 4 * len(ts), ts[0] if ts else 0)
        made.append(j)
        return j
    monkeypatch.setattr(api, "job_from_synth", fake_job_from_synth)

    class FakePrep:
        def __init__(self, sb): pass
        def job(self, ctx, t0, t1, W): return fake_job_from_synth(ctx, None, W, range(t0, t1))
        def register(self, ctx): pass
        def unregister(self): pass
    monkeypatch.setattr(api, "PreparedAlignments", FakePrep)
    fake_sb = types.SimpleNamespace(seq=None, qual=None, off=None)
    monkeypatch.setattr(synth, "generate_parallel", lambda *a, **k: fake_sb)
    monkeypatch.setattr(synth, "generate", lambda *a, **k: fake_sb)
    monkeypatch.setattr(model_io, "default_model_file", lambda d: ("model.bin", None))
    from herro_amd import shard
    hang = __import__("threading").Event()

    def fake_strong(*a, **k):
        if strong_mode == "raises":
            raise RuntimeError("a peer went away")
        if strong_mode == "hangs":
            hang.wait(30)          # a rank stuck in a receive: the line must go out without the leg
        return {"windows_per_s": 2.0, "windows": 8, "ranks_seen": 1}
    monkeypatch.setattr(shard, "strong_leg", fake_strong)
    import subprocess
    spawned = []

    def fake_run(cmd, **kw):   # the default-size leg a short run appends ('long_run'): a child process of the same script
        spawned.append(cmd)
        line = json.dumps({"steps": 256, "warmup": 8, "value": 2.0e6, "ms_per_step": 0.064, "timed_region_s": 0.016, "repeat_ms_per_step": [0.064],
                           "roofline": {"frac": 0.22}, "config": {"streams_per_gpu": 2}})
        return types.SimpleNamespace(stdout="noise\n" + line + "\n", returncode=0)
    monkeypatch.setattr(subprocess, "run", fake_run)
    extra_legs = "--precision" in argv      # one case runs the `sustained` / `sensitivity` legs too (they re-run jobs back to back: the ordering checks below are about the timed passes)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--self-check", "0"] + ([] if extra_legs else ["--sensitivity", "0"]) + argv)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    FakeJob.log = []
    left = []
    monkeypatch.setattr(os, "_exit", lambda code: (left.append(code), (_ for _ in ()).throw(SystemExit(code))))
    try:
        bench.main()
    except SystemExit:
        assert strong_mode != "ok" and left == [3]     # a failed or stuck leg: the line is out, the exit status says so, the runtime is not torn down
    hang.set()
    assert (strong_mode != "ok") == bool(left)
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(out) == 1, out
    d = json.loads(out[0])
    for k in REQUIRED:
        assert k in d, k
    if steps is not None:
        assert d["steps"] == steps
    assert d["timed_region_s"] > 0 and d["strong_ok"] == (strong_mode == "ok")
    if d["steps"] < 64:   # a short run carries the default-size figure of the same leg
        assert len(spawned) == 1 and "--long-run-steps" in spawned[0] and "--full" in spawned[0] and d["long_run"]["value"] == 2.0e6 and d["long_run"]["steps"] == 256
    else:
        assert not spawned and "long_run" not in d
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["unit"] == "windows/s" and "workload" in d["config"]
    if strong_mode == "ok":
        assert d["strong"]["ranks_seen"] == d["n_gpus"] and d["strong"]["windows_per_s"] > 0   # the sharded leg rides in the same line
    else:   # the measured line survives a leg that fails or never comes back
        assert "error" in d["strong"] and d["value"] > 0
        assert ("peer went away" in d["strong"]["error"]) if strong_mode == "raises" else ("strong-timeout" in d["strong"]["error"])
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(d["roofline"])
    assert len(d["roofline_next_kernels"]) == 2 and all({"kernel", "bound", "frac"} <= set(r) for r in d["roofline_next_kernels"])
    assert d["roofline"]["launch_us"] >= d["roofline_next_kernels"][0]["launch_us"] >= d["roofline_next_kernels"][1]["launch_us"]
    if d["end_to_end"] is not None:   # job creation + D2H inside the timed region: every end-to-end job fetched its bases once
        assert d["end_to_end"]["windows_per_s"] > 0 and d["end_to_end"]["windows"] > 0
        n_fetch = sum(1 for ev, _ in FakeJob.log if ev == "D")   # timed jobs + the untimed warm-up jobs of each feeder
        e = d["end_to_end"]
        assert n_fetch == (e["jobs_per_feeder"] + e["warmup_jobs_per_feeder"]) * e["feeders_per_gpu"]
    # every job that ran went featurize -> infer -> consensus, and the timed region covered exactly `steps` batches:
    # windows run in the timed region = steps * batch; count via the log between warm-up and the kernel-timing pass is
    # not separable here, so check the invariant the pipeline relies on instead: no job is inferred twice in a row
    last = {}
    for ev, jid in FakeJob.log:
        if ev == "I":
            assert last.get(jid) == "F"
        last[jid] = ev
    if extra_legs:   # the extra legs of round 6 ride in the same line
        su = d["sustained"]
        assert su["seconds"] >= 0.05 and su["passes"] >= 1 and su["windows_per_s"] > 0 and su["shader_clock_mhz"][0][1] == 2100.0
        assert [x["p_snp"] for x in d["sensitivity"]] == [8e-3, 3e-2] and all(x["windows_per_s"] > 0 and x["mean_informative"] == 15 for x in d["sensitivity"])
        return
    assert d["sensitivity"] is None
    # a run of at least one full launch group cycles two or more DISTINCT jobs (the timed job is not the one that was just warmed)
    inferred = [jid for ev, jid in FakeJob.log if ev == "I"]
    if d["steps"] >= d["config"]["batches_per_launch_group"]:
        assert len(set(inferred)) >= 2 and d["config"]["distinct_windows_cycled"] >= 2 * d["config"]["batches_per_launch_group"] * 128
        assert all(a != b for a, b in zip(inferred, inferred[1:])) or d["config"]["streams_per_gpu"] > 1


def _plain_run(monkeypatch, capsys, argv):
    """bench.main() with the device API, the generator, the sharded leg and child processes replaced by stand-ins;
    returns (line, jobs by id, calls of the legs that a plain run must not reach)."""
    import subprocess
    import torch
    from herro_amd import api, synth, model_io, shard
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    extra = []

    class Ctx(FakeCtx):
        def timing_enable(self, on=True): extra.append("timing")
        def clock_probe(self): extra.append("sustained"); return 2100.0
    monkeypatch.setattr(api, "Context", Ctx)
    made = {}

    def fake_job_from_synth(ctx, sb, W, targets=None):
        ts = list(targets)
        j = FakeJob(ctx, 4 * len(ts), ts[0] if ts else 0)
        made[id(j)] = j
        return j
    monkeypatch.setattr(api, "job_from_synth", fake_job_from_synth)
    monkeypatch.setattr(api, "PreparedAlignments", lambda sb: extra.append("end_to_end"))
    fake_sb = types.SimpleNamespace(seq=None, qual=None, off=None)
    monkeypatch.setattr(synth, "generate_parallel", lambda *a, **k: (extra.append("sensitivity") if "p_snp" in k else None) or fake_sb)
    monkeypatch.setattr(synth, "generate", lambda *a, **k: fake_sb)
    monkeypatch.setattr(model_io, "default_model_file", lambda d: ("model.bin", None))
    monkeypatch.setattr(shard, "strong_leg", lambda *a, **k: extra.append("strong"))
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: extra.append("long_run"))
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    monkeypatch.setattr(bench, "cpu_baseline", lambda seed: extra.append("cpu_baseline"))
    monkeypatch.setattr(bench, "self_check", lambda *a: extra.append("self_check"))
    FakeJob.log = []
    bench.main()
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(out) == 1, out
    return json.loads(out[0]), made, extra


@pytest.mark.parametrize("argv,steps,group,streams", [(["--gpus", "1", "--steps", "20", "--warmup", "5"], 20, 20, 1),
                                                      (["--gpus", "1", "--steps", "12", "--warmup", "4", "--group", "3"], 12, 3, 2),
                                                      (["--gpus", "1", "--steps", "7", "--warmup", "1", "--group", "3"], 7, 3, 2),
                                                      (["--gpus", "1", "--steps", "256", "--warmup", "64"], 256, 32, 2)])
def test_bench_plain_run_times_only_its_steps(monkeypatch, capsys, tmp_path, argv, steps, group, streams):
    """A plain run (no --full): set-up, warm-up, exactly --steps timed steps, the line — none of the other legs — and with
    --dump-outputs the last timed step's results, the same in every run (the settle passes end where the job rotation
    starts over, however many of them ran)."""
    dumps = []
    for rep in range(2):
        d_out = tmp_path / f"out{rep}"
        # --settle 0: the windows the run infers are then the warm-up's and the timed pass's alone
        d, made, extra = _plain_run(monkeypatch, capsys, argv + ["--settle", "0" if rep == 0 else "0.05", "--dump-outputs", str(d_out)])
        assert extra == [], extra
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config"):
            assert k in d, k
        assert d["steps"] == steps and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "windows/s" and d["higher_is_better"] is True
        assert abs(d["ms_per_step"] - 1e3 * d["timed_region_s"] / steps) < 1e-9
        assert d["dtype"] == "f16 (encoder proj / FF GEMMs: activation hi+lo)" and d["config"]["batches_per_launch_group"] == group
        assert not {"roofline", "end_to_end", "sustained", "sensitivity", "self_check", "kernels", "cpu_baseline", "strong", "long_run",
                    "repeat_ms_per_step"} & set(d)
        assert d["config"]["streams_per_gpu"] == streams
        if rep == 0:
            pool = d["config"]["distinct_windows_cycled"] // (streams * group * 128)
            warm_jobs = streams * max(pool, (int(argv[argv.index("--warmup") + 1]) + group * streams - 1) // (group * streams))
            inferred = sum(made[j].n_windows for ev, j in FakeJob.log if ev == "I")
            assert inferred == warm_jobs * group * 128 + steps * 128
        files = sorted(os.listdir(d_out))
        assert files == sorted(["fasta.npy", "fasta_record_bytes.npy", "window_informative_rows.npy", "info_logits.npy", "base_logits.npy"])
        arrs = {f: np.load(d_out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values()) and sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert len(arrs["window_informative_rows.npy"]) == 128 and len(arrs["fasta_record_bytes.npy"]) == 32
        assert arrs["base_logits.npy"].shape == (arrs["window_informative_rows.npy"].sum(), 5)
        assert bytes(arrs["fasta.npy"].astype(np.uint8)).startswith(b">target0\n")
        dumps.append(arrs)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_bench_strong_mode_line(monkeypatch, capsys):
    """`bench.py --scaling strong`: the sharded data path as a line of its own, same contract keys (the leg itself is stubbed)."""
    import torch
    from herro_amd import shard
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(shard, "strong_leg", lambda args, rank, world, local, n, **k: {
        "windows_per_s": 5.0e5, "windows": n, "seconds": n / 5.0e5, "ranks_seen": 1, "timed": "scatter + ... + gather"})
    monkeypatch.setattr(sys, "argv", ["bench.py", "--scaling", "strong", "--steps", "16", "--warmup", "1"])
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    bench.main()
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(out) == 1
    d = json.loads(out[0])
    for k in REQUIRED:
        assert k in d, k
    assert d["scaling"] == "strong" and d["steps"] == 16 and d["n_gpus"] == 1 and d["value"] == 5.0e5
    assert d["strong"]["windows"] == 16 * 128 and abs(d["ms_per_step"] - 1e3 * d["strong"]["seconds"] / 16) < 1e-9


def test_model_file_when_the_tree_cannot_be_written(monkeypatch, tmp_path):
    """bench.py / smoke() in a checkout the running user cannot write: the random-init weight file goes to the user's cache
    directory instead of tests/_cache, with the same bytes, and a second call finds it there."""
    from herro_amd import model_io
    p0, raw0 = model_io.default_model_file(str(tmp_path / "writable"))
    (tmp_path / "file").write_bytes(b"")
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "xdg"))
    blocked = str(tmp_path / "file" / "_cache")          # below a regular file: no directory can be made there, whoever runs
    p1, raw1 = model_io.default_model_file(blocked)
    assert p1.startswith(str(tmp_path / "xdg")) and open(p1, "rb").read() == open(p0, "rb").read()
    assert all(np.array_equal(raw0[k], raw1[k]) for k in raw0)
    assert model_io.default_model_file(blocked)[0] == p1 and os.listdir(os.path.dirname(p1)) == [os.path.basename(p1)]


def test_bench_model_file_with_a_package_that_only_knows_the_tree(monkeypatch, tmp_path):
    """bench.py also drives builds of the package whose default_model_file writes tests/_cache or fails: in a checkout it
    cannot write, the script itself moves on to the user's cache directory."""
    from herro_amd import model_io
    tree = os.path.join(ROOT, "tests", "_cache")
    tried = []

    def tree_only(d):
        tried.append(d)
        if d == tree:
            raise PermissionError(13, "Permission denied", d)
        return os.path.join(d, "w.hrro"), {"d": d}
    monkeypatch.setattr(model_io, "default_model_file", tree_only)
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path))
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    path, raw = bench.model_file()
    assert tried == [tree, str(tmp_path / "herro_amd")] and path == str(tmp_path / "herro_amd" / "w.hrro")
