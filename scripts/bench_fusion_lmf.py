#!/usr/bin/env python3
"""LMF train-step time on seeded synthetic MER2023-shaped minibatches (dims 768 / 768 / 512, hidden 128, rank 4, batch 32,
dropout 0.3, Adam): the model as shipped (fusion in mer_lmf_fwd / mer_lmf_bwd, one launch each way), the same model with the
fusion written as ordinary torch ops on the GPU (the reference's formulas: cat, three batched matmuls, products, weighted sum,
bias), and the whole step replayed from one HIP graph (FusionGraphTrainer).  Also the fusion alone, forward + backward, at
that size and at the tuning grid's largest point (H 256, R 6).  Variants are timed alternately, `--repeats` rounds each,
every window ending in a device synchronise; prints one JSON line (microseconds: median [min, max] over the rounds).

    python scripts/bench_fusion_lmf.py [--steps 300] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def torch_fuse(ha, hv, ht, fa, fv, ft, w, bias):
    one = torch.ones(ha.shape[0], 1, dtype=ha.dtype, device=ha.device)
    pa, pv, pt = (torch.matmul(torch.cat([one, h], 1), f) for h, f in ((ha, fa), (hv, fv), (ht, ft)))
    zy = pa * pv * pt
    return torch.matmul(w, zy.permute(1, 0, 2)).squeeze(1) + bias


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def compare(variants, steps, repeats):
    for fn in variants.values():
        for _ in range(20):
            fn()
    rounds = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            rounds[k].append(window(fn, steps))
    return {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in rounds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU (there is no CPU path)"
    from mertools_amd import fusion_ops
    from mertools_amd.fusion_trainer import FusionGraphTrainer
    from mertools_amd.toolkit.models import get_models
    from mertools_amd.toolkit.models.lmf import LMF
    from mertools_amd.toolkit.utils.loss import CELoss, MSELoss
    dev = torch.device("cuda:0")
    B = 32
    args = argparse.Namespace(model="lmf", audio_dim=768, text_dim=768, video_dim=512, output_dim1=6, output_dim2=1, dropout=0.3,
                              hidden_dim=128, rank=4, grad_clip=-1.0, feat_type="utt")
    torch.manual_seed(0)
    batch = dict(audios=torch.randn(B, 768, device=dev), texts=torch.randn(B, 768, device=dev), videos=torch.randn(B, 512, device=dev))
    emos, vals = torch.randint(0, 6, (B,), device=dev), torch.randn(B, device=dev)
    cls, reg = CELoss(), MSELoss()
    res = {"unit": "us", "columns": "median, min, max", "steps_per_window": a.steps, "windows": a.repeats}

    class TorchOpsLMF(LMF):
        """The shipped model with nothing but the fusion replaced: encoders and heads stay on the HIP kernels."""

        def forward(self, batch):
            features = torch_fuse(self.audio_encoder(batch['audios']), self.video_encoder(batch['videos']), self.text_encoder(batch['texts']),
                                  self.audio_factor, self.video_factor, self.text_factor, self.fusion_weights, self.fusion_bias)
            return (features, fusion_ops.linear(features, self.fc_out_1), fusion_ops.linear(features, self.fc_out_2),
                    torch.zeros((), dtype=torch.int64, device=features.device))

    def stepper(m):
        m = m.to(dev).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)

        def step():
            opt.zero_grad()
            f, e, v, il = m(batch)
            (il + cls(e, emos) + reg(v, vals)).backward()
            opt.step()
        return step

    tr = FusionGraphTrainer(get_models(args).to(dev), lr=1e-3, weight_decay=1e-5)
    res["train_step"] = compare({"lmf_fuse_eager": stepper(get_models(args)), "torch_ops_fusion_eager": stepper(TorchOpsLMF(args)),
                                 "graph_replay": lambda: tr.train_step(batch, emos, vals)}, a.steps, a.repeats)

    for H, R in ((128, 4), (256, 6)):
        O = H // 2
        g = torch.Generator().manual_seed(H)
        mk = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev).requires_grad_(True)   # noqa: E731
        xs = [mk(B, H), mk(B, H), mk(B, H)] + [mk(R, H + 1, O, k=(H + 1) ** -0.5) for _ in range(3)] + [mk(1, R), mk(1, O)]
        dout = torch.randn(B, O, generator=g).to(dev)

        def fb(fuse):
            def run():
                for x in xs:
                    x.grad = None
                fuse(*xs).backward(dout)
            return run
        res[f"fusion_fwd_bwd_H{H}_R{R}_B{B}"] = compare({"lmf_fuse": fb(fusion_ops.lmf_fuse), "torch_ops": fb(torch_fuse)}, a.steps, a.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
