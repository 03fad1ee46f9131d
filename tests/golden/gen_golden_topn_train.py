#!/usr/bin/env python3
"""Generates tests/golden/fusion_attention_topn_train.npz and tests/golden/index_paths_mer2025_2026.npz by RUNNING THE
REFERENCE'S OWN CODE (see gen_golden.py: nothing is copied, classes are exec'd from the reference source at generation time).

  * fusion_attention_topn_train.npz — MER2024/toolkit/models/attention_topn.py's Attention_TOPN with 6 streams of unequal
    widths (33 is not a multiple of 16), the emotion-only head (output_dim2 = 0), dropout 0: 5 steps of B = 32 of the
    reference's CELoss + torch.optim.Adam(lr 1e-3, weight decay 1e-5), as main-release.py trains it.  Inputs, labels, init_*,
    final_*, grad0_* (step-0 gradients) and the 5 losses.
  * index_paths_mer2025_2026.npz — what index_paths_mer2024.npz records for MER2024 (labels, folds under random.seed(2024),
    metric string), from the reference's mer2025.py and mer2026.py on the committed mer2024_label-6way.npz.

    python tests/golden/gen_golden_topn_train.py
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, exec_defs  # noqa: E402

DIMS, HIDDEN, B, STEPS = [40, 24, 56, 33, 48, 72], 32, 32, 5


def topn_train_golden():
    torch.Tensor.cuda = lambda self, *a, **k: self  # attention_topn.py:88 hard-codes .cuda(); the fixture is made on the CPU
    ns = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional}
    exec_defs(REF + "/MER2024/toolkit/models/modules/encoder.py", {"MLPEncoder"}, ns)
    exec_defs(REF + "/MER2024/toolkit/models/attention_topn.py", {"Attention_TOPN"}, ns)
    exec_defs(REF + "/MER2024/toolkit/utils/loss.py", {"CELoss"}, ns)
    args = argparse.Namespace(audio_dim=DIMS, output_dim1=6, output_dim2=0, dropout=0.0, hidden_dim=HIDDEN, grad_clip=-1.0)
    torch.manual_seed(2026)
    model = ns["Attention_TOPN"](args)
    init = {k: v.clone().numpy() for k, v in model.state_dict().items()}
    xs = {f"feat{i}": torch.randn(STEPS, B, d) for i, d in enumerate(DIMS)}
    emos = torch.randint(0, 6, (STEPS, B))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    cls_loss = ns["CELoss"]()
    losses, grads0 = [], None
    for s in range(STEPS):
        opt.zero_grad()
        f, e, v, il = model({k: x[s] for k, x in xs.items()})
        assert tuple(v.shape) == (B, 0)
        loss = il + cls_loss(e, emos[s])          # main-release.py: the MSE term is skipped when output_dim2 == 0
        loss.backward()
        if s == 0:
            grads0 = {k: p.grad.clone().numpy() for k, p in model.named_parameters() if p.grad is not None}   # fc_out_2 is empty and unused
        opt.step()
        losses.append(loss.item())
    final = {k: v.clone().numpy() for k, v in model.state_dict().items()}
    np.savez_compressed(os.path.join(OUT, "fusion_attention_topn_train.npz"), dims=np.array(DIMS), hidden=np.array(HIDDEN),
                        losses=np.array(losses, dtype=np.float64), emos=emos.numpy(), **{f"x_{k}": v.numpy() for k, v in xs.items()},
                        **{f"init_{k}": v for k, v in init.items()}, **{f"final_{k}": v for k, v in final.items()},
                        **{f"grad0_{k}": v for k, v in grads0.items()})
    print("losses", losses)


def mer2025_2026_goldens():
    from sklearn.metrics import accuracy_score, f1_score, mean_squared_error
    emos = ['neutral', 'angry', 'happy', 'sad', 'worried', 'surprise']
    label_path = os.path.join(OUT, "mer2024_label-6way.npz")
    res = {}
    for ds, path in (("MER2025", "/MER2025/MER2025_Track1/toolkit/dataloader/mer2025.py"),
                     ("MER2026", "/MER2026/MER2026_Track1/toolkit/dataloader/mer2026.py")):
        cfg = argparse.Namespace(PATH_TO_LABEL={ds: label_path})
        ns = {"np": np, "random": random, "accuracy_score": accuracy_score, "f1_score": f1_score, "mean_squared_error": mean_squared_error,
              "emo2idx_mer": {e: i for i, e in enumerate(emos)}, "config": cfg}
        exec_defs(REF + path, {ds}, ns)
        args = argparse.Namespace(debug=False, batch_size=32, num_workers=0, dataset=ds)
        obj = ns[ds](args)
        p = ds + "_"
        res.update({p + "output_dim1": np.array(args.output_dim1), p + "output_dim2": np.array(args.output_dim2),
                    p + "metric_name": np.array(args.metric_name)})
        for split in ["train", "test1"]:
            names, labels = obj.read_names_labels(label_path, split)
            res[f"{p}labels_{split}_names"] = np.array(names)
            res[f"{p}labels_{split}_emo"] = np.array([l["emo"] for l in labels], dtype=np.int64)
            res[f"{p}labels_{split}_val"] = np.array([float(l["val"]) for l in labels], dtype=np.float64)
        res[p + "debug_n"] = np.array(len(obj.read_names_labels(label_path, "train", debug=True)[0]))
        random.seed(2024)
        for i, (tr, ev) in enumerate(obj.random_split_indexes(137, 5)):
            res[f"{p}fold{i}_train"] = np.array(tr, dtype=np.int64)
            res[f"{p}fold{i}_eval"] = np.array(ev, dtype=np.int64)
        rng = np.random.RandomState(int(ds[-4:]))
        probs, labs = rng.rand(40, 6), rng.randint(0, 6, 40)
        r, sres = obj.calculate_results(probs, labs, [], [])
        res.update({p + "metric_probs": probs, p + "metric_labs": labs, p + "metric_acc": np.array(r["emoacc"]),
                    p + "metric_f1": np.array(r["emofscore"]), p + "metric_str": np.array(sres), p + "metric_keys": np.array(sorted(r))})
    np.savez_compressed(os.path.join(OUT, "index_paths_mer2025_2026.npz"), **res)


if __name__ == "__main__":
    topn_train_golden()
    mer2025_2026_goldens()
