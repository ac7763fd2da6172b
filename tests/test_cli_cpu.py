"""The drop-in CLI surface (north star: scripts/benchmark.py and
scripts/print_optimal_config.py stay drop-in): same flags as the reference
(scripts/benchmark.py:34-79, scripts/print_optimal_config.py:8-48), the same method
search space and validity filter, the results cache, and the optimal-config table.
Parity unpinned: the reference's sweep needs tango/tyro/polars (absent), so the expected
counts below are derived from the reference's search space + is_valid rules by hand."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_dir):
    env = dict(os.environ, MMPT_RESULTS_DIR=str(env_dir))
    out = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_search_space_sizes():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from benchmark import search_space

    from multimodal_llm_pretraining_amd.sweep import TrainingTimeEmpiricalSweep

    # 8 GPUs: 2 (ac) × [6 shardings without offload + 5 with (offload needs sharding)]
    all8 = TrainingTimeEmpiricalSweep(search_space(1, 8, "mi355x", "vit-b16-pythia-1b", "all"))
    assert len(all8.experiments) == 2 * (6 + 5)
    # 1 GPU: sharding without offload is invalid (training_time_empirical.py:176-180)
    all1 = TrainingTimeEmpiricalSweep(search_space(1, 1, "mi355x", "vit-b16-pythia-1b", "all"))
    assert len(all1.experiments) == 2 * (1 + 5)
    naive = TrainingTimeEmpiricalSweep(search_space(1, 8, "mi355x", "pythia-1b", "naive"))
    assert len(naive.experiments) == 1 and naive.experiments[0].config["free_lunch"] is False


def test_benchmark_cli_count_and_incomplete(tmp_path):
    out = _run(["scripts/benchmark.py", "--num-nodes", "1", "--gpus-per-node", "8", "--gpu-type",
                "mi355x", "--model", "vit-b16-pythia-1b", "--methods", "all", "--cmd", "count"],
               tmp_path)
    assert "# cached experiments: 0 / 22" in out
    out = _run(["scripts/benchmark.py", "--num-nodes", "1", "--gpus-per-node", "8", "--gpu-type",
                "mi355x", "--model", "vit-b16-pythia-1b", "--methods", "naive", "--cmd",
                "print-incomplete"], tmp_path)
    assert out.count("TrainingTimeEmpirical(") == 1


def test_validation_matches_reference():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from benchmark import validate_arguments

    with pytest.raises(AssertionError, match="evenly divisible"):
        validate_arguments(1, 3, "mi355x", "vit-b16-pythia-1b")
    with pytest.raises(AssertionError, match="ampere"):
        validate_arguments(1, 8, "v100", "vit-b16-pythia-1b")
    validate_arguments(1, 8, "mi355x", "vit-b16-pythia-1b")


def test_print_optimal_config_sorts_cached_results(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from benchmark import search_space

    os.environ["MMPT_RESULTS_DIR"] = str(tmp_path)
    try:
        from multimodal_llm_pretraining_amd.sweep import TrainingTimeEmpiricalSweep

        sw = TrainingTimeEmpiricalSweep(search_space(1, 8, "mi355x", "vit-b16-pythia-1b", "all"))
        exps = sw.experiments
        # three cached results: one failed (None), two with days
        exps[0].write({"micro_batch_size": 32, "step_time": 2.0, "training_days": 0.05})
        exps[1].write({"micro_batch_size": 16, "step_time": 1.0, "training_days": 0.025})
        exps[2].write({"error": "exit status 1", "training_days": None})
        assert sw.num_cached == 3
        rec = json.load(open(exps[1].path))
    finally:
        del os.environ["MMPT_RESULTS_DIR"]
    out = _run(["scripts/print_optimal_config.py", "--num-nodes", "1", "--gpus-per-node", "8",
                "--gpu-type", "mi355x", "--model", "vit-b16-pythia-1b"], tmp_path)
    lines = [ln for ln in out.splitlines() if ln.startswith("1 ")]
    assert len(lines) == 2
    assert "0.025" in lines[0] and "0.05" in lines[1]
    # grad_acc_steps = 256 // (16 * 8) = 2 and 256 // (32 * 8) = 1
    assert lines[0].split()[-2] == "2" and lines[1].split()[-2] == "1"
    assert rec["experiment"]["model"] == "vit-b16-pythia-1b"


def test_training_script_reads_reference_training_arguments():
    """scripts/training.py maps the reference README's TrainingArguments JSON (ZeRO-1 +
    DeepSpeed optimizer block with "auto" values) onto the MI355X step's knobs."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from training import adam_from_args, sharding_from_args

    from multimodal_llm_pretraining_amd.models import get_model_class

    args = json.load(open(os.path.join(ROOT, "tests", "golden", "training_arguments_readme.json")))["args"]
    assert sharding_from_args(args) == ("zero_1", False)
    adam = adam_from_args(args, get_model_class("pythia-1b"))
    # DeepSpeed "auto" → TrainingArguments defaults, Adam (adam_w_mode false)
    assert adam.lr == 5e-5 and adam.betas == (0.9, 0.999) and adam.eps == 1e-8
    assert adam.weight_decay == 0.0 and adam.adamw is False and adam.max_grad_norm == 1.0
    z3 = dict(args, deepspeed={"zero_optimization": {"stage": 3, "offload_optimizer": {"device": "cpu"}}})
    assert sharding_from_args(z3) == ("zero_3", True)
    fs = dict(args, deepspeed=None, fsdp="full_shard auto_wrap offload")
    assert sharding_from_args(fs) == ("fsdp_full_shard", True)
    plain = dict(args, deepspeed=None, fsdp="")
    assert sharding_from_args(plain) == ("", False)
    a2 = adam_from_args(plain, get_model_class("vit-b16-pythia-1b"))
    assert a2.adamw and a2.lr == 1e-3 and a2.weight_decay == 0.0


def _bench(args, **env):
    import subprocess
    import sys

    e = dict(os.environ, MMPT_DIST_BACKEND="gloo", **env)
    e.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e,
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("n", [2, 8])
def test_bench_self_launches_n_ranks(n):
    """`python bench.py --gpus 2` with no launcher in front starts 2 ranks itself (VERDICT r04
    #1; the reference's experiments/utils/distribute.py:37-61) and rank 0's line says
    n_gpus 2.  Launcher check mode: every rank joins a gloo group, nothing touches a GPU."""
    r = _bench(["--gpus", str(n), "--model", "tiny-mm"], MMPT_BENCH_LAUNCH_CHECK="1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["ranks_seen"] == n and out["self_launched"]


def test_bench_self_launch_fails_when_a_rank_dies():
    r = _bench(["--gpus", "2", "--model", "tiny-mm"], MMPT_BENCH_LAUNCH_CHECK="fail1")
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_visible_gpus_counts_from_sysfs_without_hip(tmp_path):
    """the self-launching parent counts GPUs from the KFD topology in sysfs
    (GPU nodes have a non-zero gfx_target_version, the CPU node 0), narrowed by the visibility
    variables — no HIP call before the ranks start.  None without a topology."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    nodes = tmp_path / "nodes"
    for i, ver in enumerate([0] + [90500] * 8):  # node 0 = CPU, 8 gfx950 nodes
        d = nodes / str(i)
        d.mkdir(parents=True)
        (d / "properties").write_text(f"cpu_cores_count {0 if ver else 64}\n"
                                      f"gfx_target_version {ver}\nsimd_count {0 if not ver else 1024}\n")
    assert bench.visible_gpus({}, str(nodes), None) == 8
    assert bench.visible_gpus({"HIP_VISIBLE_DEVICES": "0,1"}, str(nodes), None) == 2
    assert bench.visible_gpus({"ROCR_VISIBLE_DEVICES": "3"}, str(nodes), None) == 1
    assert bench.visible_gpus({}, str(tmp_path / "absent"), None) is None
    # only the render nodes this process can open count (a container's own GPUs)
    for i in range(1, 9):
        p = nodes / str(i) / "properties"
        p.write_text(p.read_text() + f"drm_render_minor {127 + i}\n")
    dri = tmp_path / "dri"
    dri.mkdir()
    for minor in (128, 129, 130):
        (dri / f"renderD{minor}").write_text("")
    assert bench.visible_gpus({}, str(nodes), str(dri)) == 3
    # the self-launch path never initialises HIP in the parent
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("def self_launch"):src.index("def launch_check")]
    assert "torch.cuda" not in body


def _load_bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_plain_run_is_lean_and_full_is_an_option(monkeypatch):
    """A plain `bench.py --gpus 1 --steps N --warmup W` asks for neither the GEMM yardstick
    nor the CPU baseline; `--full` switches both on, and `--dump-outputs` takes a folder."""
    import sys

    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs == ""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    src = open(os.path.join(ROOT, "bench.py")).read()
    main = src[src.index("def main"):]
    for call in ("gemm_yardstick(", "cpu_baseline("):  # every use in main() is behind --full
        for line in main.splitlines():
            if call in line:
                at = main.index(line)
                assert "args.full" in main[max(0, at - 200):at + len(line)], line


def test_bench_dump_outputs_writes_float_arrays(tmp_path):
    """--dump-outputs: the last step's loss and a fixed, seeded sample of the weights it left,
    float32 / float64 `.npy`, the same positions on every call, at most 64 MB in all."""
    import types

    import numpy as np
    import torch

    bench = _load_bench()
    n = bench.DUMP_SAMPLE + 1000
    master = torch.arange(n, dtype=torch.float32)
    store = types.SimpleNamespace(master=master, shadow=torch.ones(64, dtype=torch.bfloat16))
    trainer = types.SimpleNamespace(store=store)
    loss = torch.tensor([12.5])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), trainer, loss, 5, 1)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["loss.npy", "loss_sum.npy", "master_sample.npy", "shadow_sample.npy"]
    total = 0
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
        total += x.nbytes
    assert total <= 64 * 2**20
    assert np.load(tmp_path / "a" / "loss.npy")[0] == 2.5
    assert np.load(tmp_path / "a" / "loss_sum.npy")[0] == 12.5
    m = np.load(tmp_path / "a" / "master_sample.npy")
    assert m.shape == (bench.DUMP_SAMPLE,) and (np.diff(m) >= 0).all() and m.max() < n
    assert np.load(tmp_path / "a" / "shadow_sample.npy").shape == (64,)
