"""Grouped Attention_TOPN training against the default sequential loop on a seeded synthetic MER2024-shaped corpus:
`--model attention_topn --fusion_topn 2 --fusion_modality AVT`, i.e. the 6 streams chinese-hubert-base / -large (768 / 1024),
bloom-7b1 / Baichuan-13B-Base (4096 / 5120), videomae-base-K400-mer2023-299 / clip-vit-large-patch14 (768 / 768), hidden 128,
batch 32, dropout 0.3.  Clip counts: 5030 train / 1169 test1, the Train&Val and MER-SEMI sizes of the MER2024 paper (the
reference ships no label file, so the counts are not in it; --clips overrides them).

Wall seconds (host clock around a whole main_release run, results on the host) of the default path, --parallel_folds and
--num_trials N: after one short warm-up run of each, the default and the grouped run alternate --reps times so the spread is
known before a ratio is quoted.  Prints one JSON line.

    python scripts/bench_fusion_topn_group.py [--epochs 10] [--reps 3] [--trials 8]
    python scripts/bench_fusion_topn_group.py --launches [--keep DIR]   # launches per train step for M in {3, 6, 18} x G in {5, 40}
                                                                        # (rocprofv3 --kernel-trace --stats; the G = 5 CSVs are kept in DIR)
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DATASET, TOPN, MODALITY = "MER2024", 2, "AVT"
WIDTHS = {"chinese-hubert-base": 768, "chinese-hubert-large": 1024, "bloom-7b1": 4096, "Baichuan-13B-Base": 5120,
          "videomae-base-K400-mer2023-299": 768, "clip-vit-large-patch14": 768}
COUNT_DIMS = {3: [768, 4096, 768], 6: [768, 1024, 4096, 5120, 768, 768],
              18: [768, 1024, 1280, 512, 768, 1024, 4096, 5120, 1024, 768, 1024, 4096, 768, 768, 1408, 512, 257, 1024]}


def make_corpus(root, clips, seed=0):
    from mertools_amd import config
    from mertools_amd.toolkit.data.feat_data_topn import topn_feature_names
    d = os.path.join(root, config._DATASETS[DATASET])
    rng = np.random.RandomState(seed)
    emos = ['neutral', 'angry', 'happy', 'sad', 'worried', 'surprise']
    names = {s: [f"{s}_{i:05d}" for i in range(n)] for s, n in zip(("train", "test1"), clips)}
    corp = {f"{s}_corpus": {n: {"emo": emos[rng.randint(6)]} for n in ns} for s, ns in names.items()}
    os.makedirs(os.path.join(d, "features"), exist_ok=True)
    np.savez_compressed(os.path.join(d, config._LABELS[DATASET]), **{k: np.array(v, dtype=object) for k, v in corp.items()})
    dims = []
    for feat in topn_feature_names(TOPN, MODALITY, None, dataset=DATASET):
        dim = WIDTHS[feat[:-len("-UTT")]]
        dims.append(dim)
        os.makedirs(os.path.join(d, "features", feat), exist_ok=True)
        for ns in names.values():
            for n in ns:
                np.save(os.path.join(d, "features", feat, f"{n}.npy"), rng.randn(dim).astype(np.float32))
    return dims


def cli_argv(data, out, tag, epochs):
    hyper = os.path.join(out, "tune.yaml")
    with open(hyper, "w") as fh:
        fh.write("attention_topn:\n  hidden_dim: 128\n  dropout: 0.3\n  grad_clip: -1\n  lr: 1.0e-3\n")
    return ["--model", "attention_topn", "--feat_type", "utt", "--dataset", DATASET, "--fusion_topn", str(TOPN), "--fusion_modality", MODALITY,
            "--epochs", str(epochs), "--batch_size", "32", "--gpu", "0", "--seed", "0", "--data_root", data, "--hyper_path", hyper,
            "--save_root", os.path.join(out, "saved-" + tag)]


def run_cli(data, out, tag, extra, epochs):
    import contextlib
    import io
    import torch
    from mertools_amd import main_release
    torch.cuda.synchronize()
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        main_release.main(cli_argv(data, out, tag, epochs) + extra)
    torch.cuda.synchronize()
    return time.time() - t0


def read_time(data):
    """Seconds of the corpus reading every run starts with (get_loaders: per-clip .npy reads, shared by all paths)."""
    import contextlib
    import io
    from mertools_amd import config
    from mertools_amd.main_release import build_parser
    from mertools_amd.toolkit.dataloader import get_dataloaders
    config.set_data_root(data)
    config.dataset = DATASET
    args = build_parser().parse_args(cli_argv(data, data, "read", 1))
    args.feat_scale = 1
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        get_dataloaders(args).get_loaders()
    return time.time() - t0


def train_steps_per_run(n, epochs, folds=5, B=32):
    size = n // folds
    tr = [n - (size if f < folds - 1 else n - size * (folds - 1)) for f in range(folds)]
    return epochs * sum(-(-t // B) for t in tr)


def count_mode(M, G, steps):
    """Runs `steps` captured train steps of a G-model, M-stream group (plus the one uncaptured warm-up step) for rocprofv3 to count."""
    import torch
    from mertools_amd.fusion_topn_group import FusionTopnGroupTrainer
    from mertools_amd.toolkit.models import get_models
    dims = COUNT_DIMS[M]
    a = argparse.Namespace(model="attention_topn", audio_dim=dims, output_dim1=6, output_dim2=0, dropout=0.3, hidden_dim=128,
                           grad_clip=-1.0, feat_type="utt")
    torch.manual_seed(0)
    ms = [get_models(a).cuda() for _ in range(G)]
    tr = FusionTopnGroupTrainer(ms, lr=1e-3, weight_decay=1e-5, grad_clip=-1.0, seeds=list(range(G)), batch_size=32)
    g = torch.Generator().manual_seed(0)
    n = 512
    tr.set_tables([torch.randn(n, d, generator=g) for d in dims], torch.randint(0, 6, (n,), generator=g))
    index = torch.randint(0, n, (steps, G, 32), generator=g, dtype=torch.int32)
    tr.run(index, torch.full((steps, G), 32, dtype=torch.int32), True)
    torch.cuda.synchronize()


def launches(M, G, steps=10, keep=None):
    """(kernel dispatches per training step, {kernel: share of GPU time in %}) of a G-model, M-stream group, from a
    rocprofv3 --kernel-trace --stats run of count_mode; the stats CSV is copied to `keep` when given."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "tg", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--count", f"{M},{G}", "--steps", str(steps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        calls, share = 0, {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "tg_" in row["Name"]:
                    calls += int(row["Calls"])
                    short = row["Name"].split("(")[0].replace("void ", "").replace("mer::", "")
                    share[short] = share.get(short, 0.0) + float(row["Percentage"])
            if keep:
                shutil.copy(f, keep)
    return calls / (steps + 1), {k: round(v, 2) for k, v in sorted(share.items(), key=lambda kv: -kv[1])}   # + the uncaptured warm-up step


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--trials", type=int, default=8)
    p.add_argument("--clips", type=str, default="5030,1169")
    p.add_argument("--launches", action="store_true")
    p.add_argument("--keep", type=str, default=None)
    p.add_argument("--count", type=str, default=None)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--corpus_only", action="store_true", help="stop after the corpus generation (a rehearsal without a device)")
    a = p.parse_args()
    if a.count is not None:
        M, G = (int(x) for x in a.count.split(","))
        return count_mode(M, G, a.steps)
    if a.launches:
        out = {"bench": "fusion_topn_group_launches", "launches_per_train_step": {}, "gpu_time_share_percent_g5": {}}
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
        for M in (3, 6, 18):
            for G in (5, 40):
                keep = os.path.join(a.keep, f"fusion_topn_group_m{M}_kernel_stats.csv") if a.keep and G == 5 else None
                n, share = launches(M, G, a.steps, keep)
                out["launches_per_train_step"][f"M{M}_G{G}"] = n
                if G == 5:
                    out["gpu_time_share_percent_g5"][f"M{M}"] = share
                print(f"M{M} G{G}", n, file=sys.stderr, flush=True)
        print(json.dumps(out))
        return
    clips = [int(x) for x in a.clips.split(",")]
    out = {"bench": "fusion_topn_group", "dataset": DATASET, "fusion_topn": TOPN, "modality": MODALITY, "epochs": a.epochs,
           "hidden_dim": 128, "batch_size": 32, "clips": {"train": clips[0], "test1": clips[1]}}
    steps = train_steps_per_run(clips[0], a.epochs)
    with tempfile.TemporaryDirectory() as d:
        data = os.path.join(d, "data")
        out["stream_widths"] = make_corpus(data, clips)
        if a.corpus_only:
            print(json.dumps(out))
            return
        out["corpus_read_s"] = round(read_time(data), 3)
        print("corpus_read_s", out["corpus_read_s"], file=sys.stderr, flush=True)
        group, trials = ["--parallel_folds"], ["--num_trials", str(a.trials)]
        for tag, extra in (("warm-default", []), ("warm-group", group), ("warm-trials", ["--num_trials", "2"])):   # warm-up: 1 epoch each
            print(tag, round(run_cli(data, d, tag, extra, 1), 3), file=sys.stderr, flush=True)
        walls = {"default": [], "parallel_folds": []}
        for r in range(a.reps):                                                  # alternated, so drift hits both alike
            walls["default"].append(run_cli(data, d, f"default{r}", [], a.epochs))
            walls["parallel_folds"].append(run_cli(data, d, f"group{r}", group, a.epochs))
            print(r, walls["default"][-1], walls["parallel_folds"][-1], file=sys.stderr, flush=True)
        walls[f"trials{a.trials}"] = [run_cli(data, d, "trials", trials, a.epochs)]
        for name, w in walls.items():
            n = a.trials if name.startswith("trials") else 1
            out[name] = {"wall_s": [round(x, 3) for x in w], "min_s": round(min(w), 3), "max_s": round(max(w), 3),
                         "model_steps_per_s": round(steps * n / min(w), 1)}
    dmin, gmax = out["default"]["min_s"], out["parallel_folds"]["max_s"]
    out["grouped_slowest_faster_than_default_fastest"] = gmax < dmin
    out["speedup_parallel_folds_worst_case"] = round(dmin / gmax, 2)             # default's fastest over the group's slowest
    out["speedup_parallel_folds_best_of"] = round(dmin / out["parallel_folds"]["min_s"], 2)
    r = out["corpus_read_s"]                                                     # the same without the corpus reading all paths start with
    out["speedup_parallel_folds_after_read"] = round((dmin - r) / (out["parallel_folds"]["min_s"] - r), 2)
    t = out[f"trials{a.trials}"]["min_s"]
    out["trials_vs_default_same_work"] = round(a.trials * dmin / t, 2)           # N default runs (N x the fastest) over one N-trial run
    print(json.dumps(out))


if __name__ == "__main__":
    main()
