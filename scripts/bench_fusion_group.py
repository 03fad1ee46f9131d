"""Grouped fusion training against the default sequential loop on a seeded synthetic MER2023-shaped corpus (3373 train clips,
test sets of 411 / 412 / 834, dims 768 / 768 / 512, hidden 128, batch 32): wall seconds and model-steps/s (optimiser steps of all
models) of main_release's default path, --parallel_folds, and --parallel_folds --num_trials 4 / 8.  Prints one JSON line.

    python scripts/bench_fusion_group.py [--epochs 10] [--skip_default]
    python scripts/bench_fusion_group.py --launches      # launches per training step for G = 5 and G = 40 (rocprofv3 --kernel-trace --stats)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SPLITS = {"train": 3373, "test1": 411, "test2": 412, "test3": 834}
DIMS = {"audio-UTT": 768, "text-UTT": 768, "video-UTT": 512}


def make_corpus(root, seed=0):
    d = os.path.join(root, "mer2023-dataset-process")
    rng = np.random.RandomState(seed)
    emos = ['neutral', 'angry', 'happy', 'sad', 'worried', 'surprise']
    names = {s: [f"{s}_{i:05d}" for i in range(n)] for s, n in SPLITS.items()}
    corp = {f"{s}_corpus": {n: {"emo": emos[rng.randint(6)], "val": float(rng.uniform(-3, 3))} for n in ns} for s, ns in names.items()}
    os.makedirs(os.path.join(d, "features"), exist_ok=True)
    np.savez_compressed(os.path.join(d, "label-6way.npz"), **{k: np.array(v, dtype=object) for k, v in corp.items()})
    for feat, dim in DIMS.items():
        os.makedirs(os.path.join(d, "features", feat), exist_ok=True)
        for ns in names.values():
            for n in ns:
                np.save(os.path.join(d, "features", feat, f"{n}.npy"), rng.randn(dim).astype(np.float32))


def run_cli(data, out, extra, epochs):
    from mertools_amd import main_release
    hyper = os.path.join(out, "tune.yaml")
    with open(hyper, "w") as fh:
        fh.write("attention:\n  hidden_dim: 128\n  dropout: 0.3\n  grad_clip: -1\n  lr: 1.0e-3\n")
    argv = ["--model", "attention", "--feat_type", "utt", "--dataset", "MER2023", "--audio_feature", "audio-UTT", "--text_feature",
            "text-UTT", "--video_feature", "video-UTT", "--epochs", str(epochs), "--batch_size", "32", "--gpu", "0", "--seed", "0",
            "--data_root", data, "--hyper_path", hyper, "--save_root", os.path.join(out, "saved-" + "-".join(extra).replace("--", ""))]
    import torch
    torch.cuda.synchronize()
    t0 = time.time()
    main_release.main(argv + extra)
    torch.cuda.synchronize()
    return time.time() - t0


def read_time(data):
    """Seconds of the corpus reading every run starts with (get_loaders: per-clip .npy reads, shared by all paths)."""
    from mertools_amd import config
    from mertools_amd.main_release import build_parser
    from mertools_amd.toolkit.dataloader import get_dataloaders
    config.set_data_root(data)
    config.dataset = "MER2023"
    args = build_parser().parse_args(["--model", "attention", "--feat_type", "utt", "--dataset", "MER2023", "--audio_feature", "audio-UTT",
                                      "--text_feature", "text-UTT", "--video_feature", "video-UTT"])
    args.feat_scale = 1
    t0 = time.time()
    get_dataloaders(args).get_loaders()
    return time.time() - t0


def train_steps_per_run(epochs, folds=5, B=32):
    n = SPLITS["train"]
    size = n // folds
    tr = [n - (size if f < folds - 1 else n - size * (folds - 1)) for f in range(folds)]
    return epochs * sum(-(-t // B) for t in tr)


def count_mode(G, steps):
    """Runs `steps` captured train steps of a G-model group (plus the one uncaptured warm-up step) for rocprofv3 to count."""
    import torch
    from mertools_amd.fusion_group import FusionGroupTrainer
    from mertools_amd.toolkit.models import get_models
    a = argparse.Namespace(model="attention", audio_dim=768, text_dim=768, video_dim=512, output_dim1=6, output_dim2=1, dropout=0.3,
                           hidden_dim=128, grad_clip=-1.0, feat_type="utt")
    torch.manual_seed(0)
    ms = [get_models(a).cuda() for _ in range(G)]
    tr = FusionGroupTrainer(ms, lr=1e-3, weight_decay=1e-5, grad_clip=-1.0, seeds=list(range(G)), batch_size=32)
    g = torch.Generator().manual_seed(0)
    n = 512
    tr.set_tables(torch.randn(n, 768, generator=g), torch.randn(n, 768, generator=g), torch.randn(n, 512, generator=g),
                  torch.randint(0, 6, (n,), generator=g), torch.randn(n, generator=g))
    index = torch.randint(0, n, (steps, G, 32), generator=g, dtype=torch.int32)
    tr.run(index, torch.full((steps, G), 32, dtype=torch.int32), True)
    torch.cuda.synchronize()


def launches(G, steps=10):
    """Kernel dispatches per training step of a G-model group, from a rocprofv3 --kernel-trace --stats run of count_mode."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "fg", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--count", str(G), "--steps", str(steps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        calls = 0
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "tg_" in row["Name"]:   # the group engine's kernels (csrc/fusion_topn_group.hip)
                    calls += int(row["Calls"])
    return calls / (steps + 1)   # + the one uncaptured warm-up step


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--skip_default", action="store_true")
    p.add_argument("--trials", type=str, default="4,8")
    p.add_argument("--launches", action="store_true")
    p.add_argument("--count", type=int, default=None)
    p.add_argument("--steps", type=int, default=10)
    a = p.parse_args()
    if a.count is not None:
        return count_mode(a.count, a.steps)
    if a.launches:
        print(json.dumps({"bench": "fusion_group_launches", "launches_per_train_step": {"G5": launches(5), "G40": launches(40)}}))
        return
    import contextlib
    import io
    out = {"bench": "fusion_group", "epochs": a.epochs, "hidden_dim": 128, "batch_size": 32}
    steps = train_steps_per_run(a.epochs)
    with tempfile.TemporaryDirectory() as d:
        make_corpus(os.path.join(d, "data"))
        runs = [("parallel_folds", ["--parallel_folds"], 1)] + [(f"trials{n}", ["--parallel_folds", "--num_trials", n], int(n))
                                                                for n in a.trials.split(",") if n]
        if not a.skip_default:
            runs.insert(0, ("default", [], 1))
        with contextlib.redirect_stdout(io.StringIO()):
            out["corpus_read_s"] = round(read_time(os.path.join(d, "data")), 3)
        for name, extra, n in runs:
            with contextlib.redirect_stdout(io.StringIO()):
                wall = run_cli(os.path.join(d, "data"), d, extra, a.epochs)
            out[name] = {"wall_s": round(wall, 3), "model_steps_per_s": round(steps * n / wall, 1)}
            print(name, out[name], file=sys.stderr, flush=True)
    if "default" in out:
        out["speedup_parallel_folds"] = round(out["default"]["wall_s"] / out["parallel_folds"]["wall_s"], 2)
        # the same ratio without the corpus reading both paths start with (n trials read the corpus once)
        r = out["corpus_read_s"]
        out["speedup_parallel_folds_after_read"] = round((out["default"]["wall_s"] - r) / (out["parallel_folds"]["wall_s"] - r), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
