"""Host side of the grouped fusion training (no GPU): --parallel_folds / --num_trials argument checks, the host plan's
minibatch orders against the real DataLoaders and the descriptor's layout.  (The kernels this ABI launches are the group
engine's: tests/test_fusion_topn_group_cpu.py::test_topn_group_kernels_use_no_scratch_memory checks their scratch usage.)"""
import ctypes
import os
import random

import numpy as np
import pytest
import torch


def _corpus(tmp_path, n_train=23, seed=1):
    root = tmp_path / "data" / "mer2023-dataset-process"
    rng = np.random.RandomState(seed)
    names = {"train": [f"tr_{i:03d}" for i in range(n_train)], "test1": [f"t1_{i:02d}" for i in range(5)],
             "test2": [f"t2_{i:02d}" for i in range(4)], "test3": [f"t3_{i:02d}" for i in range(3)]}
    emos = ['neutral', 'angry', 'happy', 'sad', 'worried', 'surprise']
    corp = {f"{s}_corpus": {n: {"emo": emos[rng.randint(6)], "val": float(rng.uniform(-3, 3))} for n in ns} for s, ns in names.items()}
    os.makedirs(root / "features", exist_ok=True)
    np.savez_compressed(root / "label-6way.npz", **{k: np.array(v, dtype=object) for k, v in corp.items()})
    for feat, d in {"audio-UTT": 12, "text-UTT": 8, "video-UTT": 10}.items():
        os.makedirs(root / "features" / feat, exist_ok=True)
        for ns in names.values():
            for n in ns:
                np.save(root / "features" / feat / f"{n}.npy", rng.randn(d).astype(np.float32))
    return tmp_path / "data"


BASE = ["--model", "attention", "--feat_type", "utt", "--dataset", "MER2023", "--audio_feature", "audio-UTT", "--text_feature", "text-UTT",
        "--video_feature", "video-UTT"]


@pytest.mark.parametrize("extra", [["--model", "lf_dnn"], ["--feat_type", "frm_align"], ["--dataset", "MER2024"],
                                   ["--model", "attention_topn"], ["--eager"]])
def test_unsupported_combinations_raise(extra):
    from mertools_amd import main_release
    argv = BASE + extra + ["--parallel_folds", "--seed", "0"]
    with pytest.raises(ValueError, match="--model attention --feat_type utt --dataset MER2023"):
        main_release.main(argv)


def test_num_trials_needs_seed():
    from mertools_amd import main_release
    with pytest.raises(ValueError, match="--seed"):
        main_release.main(BASE + ["--num_trials", "2"])


def test_host_plan_matches_dataloader_iteration(tmp_path):
    """fold_plan's per-epoch train / eval orders and its model initialisations equal what main()'s sequential loop gets from
    iterating the real DataLoaders (get_models per fold, then per epoch: train loader, eval loader, the test loaders)."""
    from mertools_amd import config
    from mertools_amd.main_release import build_parser, fold_plan
    from mertools_amd.toolkit.dataloader import get_dataloaders
    from mertools_amd.toolkit.models import get_models
    config.set_data_root(str(_corpus(tmp_path)))
    args = build_parser().parse_args(BASE + ["--batch_size", "4"])
    args.feat_scale, args.hidden_dim, args.dropout, args.grad_clip, args.epochs = 1, 8, 0.0, -1.0, 3
    config.dataset = args.dataset
    random.seed(5)
    dl = get_dataloaders(args)
    train_loaders, eval_loaders, test_loaders = dl.get_loaders()
    args.audio_dim, args.text_dim, args.video_dim = train_loaders[0].dataset.get_featdim()
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
        for (k, p), (k2, q) in zip(models[f].state_dict().items(), want_models[f].state_dict().items()):
            assert k == k2 and torch.equal(p, q), (f, k)
        for e in range(args.epochs):
            assert [names[i] for i in orders[f][e][0]] == want_orders[f][e][0], (f, e, "train")
            assert [names[i] for i in orders[f][e][1]] == want_orders[f][e][1], (f, e, "eval")


def test_descriptor_layout_and_param_count():
    from mertools_amd import _lib
    from mertools_amd import build as B
    if not os.path.exists(_lib.LIB_PATH):
        B.build()
    lib = _lib.lib()
    assert lib.mer_abi_sizeof(b"mer_fusion_group") == ctypes.sizeof(_lib.FusionGroup)
    import argparse
    from mertools_amd.toolkit.models import get_models
    a = argparse.Namespace(model="attention", text_dim=80, audio_dim=96, video_dim=64, output_dim1=6, output_dim2=1, dropout=0.0,
                           hidden_dim=64, grad_clip=-1.0, feat_type="utt")
    assert lib.mer_fusion_group_param_count(96, 80, 64, 64, 6, 1) == sum(p.numel() for p in get_models(a).parameters())
    d = _lib.FusionGroup(G=2, B=0, n_steps=1, Da=4, Dt=4, Dv=4, H=8, C1=6, C2=1)
    assert lib.mer_fusion_group_step(ctypes.byref(d), 1, None) < 0
    assert b"mer_fusion_group" in lib.mer_last_error()

