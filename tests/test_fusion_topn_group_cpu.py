"""Host side of the grouped Attention_TOPN training (no GPU): the descriptor's layout and parameter count, the shape checks of
the C ABI, the new kernels' scratch usage, the --parallel_folds / --num_trials scope, the host plan against the real
DataLoaders on a MER2026 tree, and the MER2025 / MER2026 dataset keys against vectors the reference's own classes produced
(tests/golden/gen_golden_topn_train.py)."""
import argparse
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EMOS = ['neutral', 'angry', 'happy', 'sad', 'worried', 'surprise']


def topn_corpus(tmp_path, dataset="MER2026", topn=2, modality="AVT", n_train=23, n_test=7, seed=1, dims=(12, 9, 8, 16, 10, 7)):
    """A synthetic <dataset> tree: the label file and the 3 * topn utterance-level feature directories the run reads."""
    from mertools_amd import config
    from mertools_amd.toolkit.data.feat_data_topn import topn_feature_names
    root = tmp_path / "data" / config._DATASETS[dataset]
    rng = np.random.RandomState(seed)
    names = {"train": [f"tr_{i:03d}" for i in range(n_train)], "test1": [f"t1_{i:02d}" for i in range(n_test)]}
    corp = {f"{s}_corpus": {n: {"emo": EMOS[rng.randint(6)], "val": float(rng.uniform(-3, 3))} for n in ns} for s, ns in names.items()}
    os.makedirs(root / "features", exist_ok=True)
    np.savez_compressed(root / config._LABELS[dataset], **{k: np.array(v, dtype=object) for k, v in corp.items()})
    dirs = topn_feature_names(topn, modality, None, dataset=dataset)
    for feat, d in zip(dirs, dims):
        if os.path.exists(root / "features" / feat):     # AT / AV / VT repeat a slot
            continue
        os.makedirs(root / "features" / feat)
        for ns in names.values():
            for n in ns:
                np.save(root / "features" / feat / f"{n}.npy", rng.randn(d).astype(np.float32))
    return tmp_path / "data"


def base_argv(dataset, topn=2, modality="AVT"):
    return ["--model", "attention_topn", "--feat_type", "utt", "--dataset", dataset, "--fusion_topn", str(topn), "--fusion_modality", modality]


@pytest.fixture(scope="module")
def lib():
    from mertools_amd import _lib
    from mertools_amd import build as B
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(os.path.join(B.OBJ, "fusion_topn_group.hip.resources.txt")):
        B.build()
    return _lib.lib()


def _count(lib, dims, H, C1, C2):
    return lib.mer_fusion_topn_group_param_count(len(dims), (ctypes.c_int * max(len(dims), 1))(*dims), H, C1, C2)


@pytest.mark.parametrize("M", [1, 3, 6, 18])
@pytest.mark.parametrize("C2", [0, 1])
def test_descriptor_layout_and_param_count(lib, M, C2):
    from mertools_amd import _lib
    from mertools_amd.toolkit.models import get_models
    assert lib.mer_abi_sizeof(b"mer_fusion_topn_group") == ctypes.sizeof(_lib.FusionTopnGroup)
    dims = [17 + 5 * i for i in range(M)]
    a = argparse.Namespace(model="attention_topn", audio_dim=dims, output_dim1=6, output_dim2=C2, dropout=0.0, hidden_dim=24,
                           grad_clip=-1.0, feat_type="utt")
    assert _count(lib, dims, 24, 6, C2) == sum(p.numel() for p in get_models(a).parameters())


def test_bad_shapes_fail_without_a_gpu(lib):
    from mertools_amd import _lib
    ok = dict(dims=[8, 8, 8], H=8, C1=6, C2=0)
    bad = [dict(dims=[]), dict(dims=[8] * 19), dict(dims=[8, 0, 8]), dict(dims=[8, -3, 8]), dict(dims=[8, 65536, 8]),
           dict(dims=[8, 8, 8, 8], H=16384), dict(C1=0), dict(C1=65), dict(C2=2), dict(C2=-1)]
    assert _count(lib, **ok) > 0
    for b in bad:
        kw = {**ok, **b}
        assert _count(lib, **kw) < 0, kw
        assert b"mer_fusion_topn_group_param_count" in lib.mer_last_error(), (kw, lib.mer_last_error())

    def desc(dims=(8, 8, 8), **kw):
        d = _lib.FusionTopnGroup(**{**dict(G=2, B=4, n_steps=1, M=len(dims), H=8, C1=6, C2=0), **kw})
        for i, x in enumerate(dims[:18]):
            d.D[i] = x
        return d
    assert lib.mer_fusion_topn_group_workspace_bytes(ctypes.byref(desc())) > 0
    cases = [desc(M=0), desc(M=19), desc(dims=(8, 0, 8)), desc(dims=(8, 65536, 8)), desc(dims=(8,) * 4, H=16384), desc(B=0), desc(B=2049),
             desc(C1=0), desc(C1=65), desc(C2=2)]
    for d in cases:
        assert lib.mer_fusion_topn_group_step(ctypes.byref(d), 1, None) < 0
        assert b"mer_fusion_topn_group_step" in lib.mer_last_error(), lib.mer_last_error()
        assert lib.mer_fusion_topn_group_workspace_bytes(ctypes.byref(d)) < 0
        assert b"mer_fusion_topn_group_workspace_bytes" in lib.mer_last_error(), lib.mer_last_error()
    assert lib.mer_fusion_topn_group_dropout_mask(0, 0, 19, 4, 4, ctypes.c_float(0.5), None, None) < 0
    assert b"mer_fusion_topn_group_dropout_mask" in lib.mer_last_error()


def test_topn_group_kernels_use_no_scratch_memory(lib):
    """No kernel of the group engine touches scratch.  fusion_topn_group.hip is the only translation unit with group kernels, so
    this covers every launch of mer_fusion_topn_group_step and of mer_fusion_group_step (the 3-stream ABI on the same engine)."""
    from mertools_amd import build as B
    assert "fusion_topn_group.hip" in B.SOURCES and "fusion_group.hip" not in B.SOURCES
    name, seen = None, 0
    for line in open(os.path.join(B.OBJ, "fusion_topn_group.hip.resources.txt")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "tg_" in name:
            seen += 1
            assert int(m.group(1)) == 0, f"{name} uses {m.group(1)} bytes/lane of scratch"
    assert seen >= 13, seen


def test_group_scope():
    from mertools_amd.main_release import build_parser, check_group_scope
    parse = build_parser().parse_args
    for ds in ("MER2024", "MER2025", "MER2026"):
        assert check_group_scope(parse(base_argv(ds) + ["--parallel_folds", "--seed", "0"])) == "attention_topn"
        assert check_group_scope(parse(base_argv(ds, 1, "AT") + ["--num_trials", "3", "--seed", "0"])) == "attention_topn"
    ok = ["--model", "attention", "--feat_type", "utt", "--dataset", "MER2023", "--parallel_folds"]
    assert check_group_scope(parse(ok)) == "attention"
    no_topn = ["--model", "attention_topn", "--feat_type", "utt", "--dataset", "MER2026", "--parallel_folds", "--seed", "0"]
    rejected = [no_topn, base_argv("MER2026") + ["--parallel_folds", "--eager"], base_argv("MER2026") + ["--parallel_folds", "--test_snr", "snr5"],
                base_argv("MER2026") + ["--parallel_folds", "--train_snr", "snr5"], base_argv("MER2026") + ["--parallel_folds", "--feat_type", "frm_align"],
                base_argv("MER2023") + ["--parallel_folds"], ok + ["--fusion_topn", "2"], ok + ["--dataset", "MER2026"]]
    for argv in rejected:
        with pytest.raises(ValueError, match="--model attention --feat_type utt --dataset MER2023") as e:
            check_group_scope(parse(argv))
        assert "--model attention_topn --feat_type utt --dataset MER2024|MER2025|MER2026 --fusion_topn n" in str(e.value)
    with pytest.raises(ValueError, match="--seed"):
        check_group_scope(parse(base_argv("MER2026") + ["--num_trials", "2"]))


def test_host_plan_matches_dataloader_iteration_topn(tmp_path):
    """fold_plan for an attention_topn run on a MER2026 tree: model initialisations and per-epoch train / eval orders equal
    iterating the real DataLoaders, and the CPU generator ends in the same state."""
    from mertools_amd import config
    from mertools_amd.main_release import build_parser, fold_plan
    from mertools_amd.toolkit.dataloader import get_dataloaders
    from mertools_amd.toolkit.models import get_models
    from mertools_amd.toolkit.models.attention_topn import Attention_TOPN
    saved = {k: dict(getattr(config, k)) for k in ("PATH_TO_FEATURES", "PATH_TO_LABEL", "DATA_DIR")}
    try:
        config.set_data_root(str(topn_corpus(tmp_path, "MER2026")))
        args = build_parser().parse_args(base_argv("MER2026") + ["--batch_size", "4"])
        args.feat_scale, args.hidden_dim, args.dropout, args.grad_clip, args.epochs = 1, 8, 0.0, -1.0, 3
        config.dataset = args.dataset
        random.seed(5)
        dl = get_dataloaders(args)
        train_loaders, eval_loaders, test_loaders = dl.get_loaders()
        assert len(train_loaders) == 5 and len(test_loaders) == 1
        args.audio_dim, args.text_dim, args.video_dim = train_loaders[0].dataset.get_featdim()
        assert args.audio_dim == [12, 9, 8, 16, 10, 7]
        names = train_loaders[0].dataset.dataset.names

        torch.manual_seed(11)
        want_models, want_orders = [], []
        for ii in range(len(train_loaders)):
            want_models.append(get_models(args))
            per_epoch = []
            for _ in range(args.epochs):
                tr = [n for batch in train_loaders[ii] for n in batch[3]]
                ev = [n for batch in eval_loaders[ii] for n in batch[3]]
                for tl in test_loaders:
                    for _ in tl:
                        pass
                per_epoch.append((tr, ev))
            want_orders.append(per_epoch)
        after = torch.rand(4)

        torch.manual_seed(11)
        folds = [(list(t.sampler.indices), list(e.sampler.indices)) for t, e in zip(train_loaders, eval_loaders)]
        models, orders = fold_plan(args, folds, len(test_loaders), args.epochs)
        assert torch.equal(torch.rand(4), after), "the plan consumed a different number of CPU-generator draws"
        for f in range(len(folds)):
            assert isinstance(models[f].model, Attention_TOPN)
            for (k, p), (k2, q) in zip(models[f].state_dict().items(), want_models[f].state_dict().items()):
                assert k == k2 and torch.equal(p, q), (f, k)
            for e in range(args.epochs):
                assert [names[i] for i in orders[f][e][0]] == want_orders[f][e][0], (f, e, "train")
                assert [names[i] for i in orders[f][e][1]] == want_orders[f][e][1], (f, e, "eval")
    finally:
        for k, v in saved.items():
            getattr(config, k).clear()
            getattr(config, k).update(v)


@pytest.mark.parametrize("ds", ["MER2025", "MER2026"])
def test_mer2025_mer2026_labels_splits_metrics(ds):
    """--dataset MER2025 / MER2026 against vectors the REFERENCE's own mer2025.py / mer2026.py classes produced on the committed
    label file: labels (val = -10), the emotion-only head, the folds under random.seed(2024) and the metric string."""
    from mertools_amd import config
    from mertools_amd.toolkit.dataloader import DATALOADER_MAP, get_dataloaders
    from mertools_amd.toolkit.dataloader.mer2024 import MER2024
    gold = np.load(os.path.join(G, "index_paths_mer2025_2026.npz"), allow_pickle=True)
    g = {k[len(ds) + 1:]: gold[k] for k in gold.files if k.startswith(ds + "_")}
    lab = os.path.join(G, "mer2024_label-6way.npz")
    assert DATALOADER_MAP["MER2024"] is MER2024 and DATALOADER_MAP[ds].__name__ == ds and DATALOADER_MAP[ds] is not MER2024
    old = config.PATH_TO_LABEL.get(ds)
    assert old.endswith("track1_label_6way.npz") and os.path.basename(os.path.dirname(old)) == f"mer{ds[-4:]}-dataset-process"
    assert config.PATH_TO_FEATURES[ds].endswith(os.path.join(f"mer{ds[-4:]}-dataset-process", "features"))
    config.PATH_TO_LABEL[ds] = lab
    try:
        args = argparse.Namespace(debug=False, batch_size=32, num_workers=0, dataset=ds, train_dataset=None)
        dl = get_dataloaders(args)
        obj = dl.dataloader
        assert (args.output_dim1, args.output_dim2, args.metric_name) == (int(g["output_dim1"]), int(g["output_dim2"]), str(g["metric_name"]))
        assert (args.output_dim1, args.output_dim2, args.metric_name) == (6, 0, "emo")
        for split in ["train", "test1"]:
            names, labels = obj.read_names_labels(lab, split)
            assert names == g[f"labels_{split}_names"].tolist()
            assert [l["emo"] for l in labels] == g[f"labels_{split}_emo"].tolist()
            assert [float(l["val"]) for l in labels] == g[f"labels_{split}_val"].tolist() and all(l["val"] == -10 for l in labels)
        assert len(obj.read_names_labels(lab, "train", debug=True)[0]) == int(g["debug_n"])
        random.seed(2024)
        for i, (tr, ev) in enumerate(obj.random_split_indexes(137, 5)):
            assert np.array_equal(np.array(tr), g[f"fold{i}_train"]) and np.array_equal(np.array(ev), g[f"fold{i}_eval"])
        r, s = dl.calculate_results(g["metric_probs"], g["metric_labs"], [], [])
        assert r["emoacc"] == float(g["metric_acc"]) and r["emofscore"] == float(g["metric_f1"]) and s == str(g["metric_str"])
        assert sorted(r) == g["metric_keys"].tolist() and "valmse" not in r
        with pytest.raises(AssertionError):
            DATALOADER_MAP[ds](argparse.Namespace(debug=False, batch_size=32, num_workers=0, dataset="MER2024"))
    finally:
        config.PATH_TO_LABEL[ds] = old


def test_topn_feature_names_per_dataset():
    from mertools_amd.toolkit.data.feat_data_topn import _SLOTS, topn_feature_names
    from mertools_amd.toolkit.globals import (AUDIO_RANK_LOW2HIGH, FEATURE_DIR_OF, IMAGE_RANK_LOW2HIGH, TEXT_RANK_LOW2HIGH,
                                              TOPN_RANK_LOW2HIGH)
    assert TOPN_RANK_LOW2HIGH["MER2024"] == {"A": AUDIO_RANK_LOW2HIGH, "T": TEXT_RANK_LOW2HIGH, "V": IMAGE_RANK_LOW2HIGH}
    for ds, rank in TOPN_RANK_LOW2HIGH.items():
        for modality, slots in _SLOTS.items():
            for n in (1, 2, 4):
                want = [f"{FEATURE_DIR_OF[d]}-UTT" for s in slots for d in rank[s][-n:]]
                assert topn_feature_names(n, modality, dataset=ds) == want and len(want) == 3 * n
    # the run scripts' cases, spelled out (MER2025 / MER2026 run-multimodal.sh: --fusion_topn 1 2 --fusion_modality AVT)
    assert topn_feature_names(2, "AVT", dataset="MER2026") == ["chinese-hubert-large-UTT", "chinese-hubert-base-UTT", "chinese-macbert-base-UTT",
                                                               "chinese-macbert-large-UTT", "clip-vit-base-patch32-UTT", "clip-vit-large-patch14-UTT"]
    assert topn_feature_names(1, "AVT", dataset="MER2025") == ["chinese-hubert-large-UTT", "chinese-roberta-wwm-ext-UTT", "clip-vit-large-patch14-UTT"]
    assert topn_feature_names(6, "AV", dataset="MER2025")[0] == "wavlm-base-UTT"     # (5 text sets: AVT stops at n = 5)
    # the MER2024 default is unchanged
    assert topn_feature_names(1, "AT", None) == ["chinese-hubert-large-UTT", "Baichuan-13B-Base-UTT", "Baichuan-13B-Base-UTT"]
    assert topn_feature_names(2, "AVT") == topn_feature_names(2, "AVT", None, "UTT", dataset="MER2024")


@pytest.mark.parametrize("ds,stored", [("MER2023", False), ("MER2024", True), ("MER2025", True), ("MER2026", True)])
def test_save_results_stores_emo_probs_for_the_emotion_only_corpora(tmp_path, ds, stored):
    """MER2025 / MER2026 keep the fold-averaged test probabilities in test1_*.npz as MER2024 does (MER2026_Track1/main-release.py:280-288)."""
    from mertools_amd.main_release import _save_results
    from mertools_amd.toolkit.dataloader.mer2024 import emotion_metrics
    rng = np.random.RandomState(0)
    labels = rng.randint(0, 6, 11)
    folds = [dict(eval_emofscore=0.5, eval_emoacc=0.25, test1_emolabels=labels, test1_emoprobs=rng.rand(11, 6)) for _ in range(5)]

    class Results:
        def calculate_results(self, emo_probs=[], emo_labels=[], val_preds=[], val_labels=[]):
            return emotion_metrics(np.array(emo_probs), emo_labels)
    _save_results(argparse.Namespace(dataset=ds), folds, [1.0] * 5, Results(), 1, str(tmp_path), "prefix", 123.0)
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 2 and files[0].startswith("cv_prefix_f1:0.5000_acc:0.2500_") and files[1].startswith("test1_prefix_f1:")
    got = np.load(tmp_path / files[1], allow_pickle=True)
    assert ("emo_probs" in got.files) == stored
    if stored:
        assert np.array_equal(got["emo_probs"], np.mean([f["test1_emoprobs"] for f in folds], axis=0))
