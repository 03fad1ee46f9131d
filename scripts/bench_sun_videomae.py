#!/usr/bin/env python3
"""Throughput of MER2024's fine-tuned VideoMAE extractor (extract_sun_videomae) on a synthetic corpus: videos/s for base-160 and
base-224, UTTERANCE and FRAME, the forwards per video against the reference's 4 x items, and achieved FLOP/s from shape-computed FLOPs
(2 x MACs of the patch GEMM, the blocks' GEMMs and attention; the per-view figures are computed, not measured).

    python scripts/bench_sun_videomae.py [--videos 64] [--frames 80] [--size 112] [--levels UTTERANCE,FRAME] [--models 160,224]
Prints one JSON line per (model, level).  Weights are synthetic (random, checkpoint layout); the corpus is random u8 frames."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def view_flops(S, D=768, depth=12, mlp=3072, P=16, F=16, ts=2):
    T = (S // P) ** 2 * (F // ts)
    K = 3 * ts * P * P
    per_block = 2 * T * D * 3 * D + 2 * 2 * T * T * D + 2 * T * D * D + 2 * 2 * T * D * mlp
    return 2 * T * K * D + depth * per_block


def synthetic_checkpoint(D=768, depth=12, mlp=3072, P=16, seed=0):
    g = torch.Generator().manual_seed(seed)

    def r(*s, sc=0.02):
        return torch.randn(*s, generator=g) * sc
    ck = {"patch_embed.proj.weight": r(D, 3, 2, P, P), "patch_embed.proj.bias": r(D), "norm.weight": 1 + r(D, sc=0.1), "norm.bias": r(D)}
    for l in range(depth):
        b = f"blocks.{l}."
        ck.update({b + "norm1.weight": 1 + r(D, sc=0.1), b + "norm1.bias": r(D), b + "attn.qkv.weight": r(3 * D, D), b + "attn.q_bias": r(D),
                   b + "attn.v_bias": r(D), b + "attn.proj.weight": r(D, D), b + "attn.proj.bias": r(D), b + "norm2.weight": 1 + r(D, sc=0.1),
                   b + "norm2.bias": r(D), b + "mlp.fc1.weight": r(mlp, D), b + "mlp.fc1.bias": r(mlp), b + "mlp.fc2.weight": r(D, mlp),
                   b + "mlp.fc2.bias": r(D)})
    return ck


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--levels", default="UTTERANCE,FRAME")
    ap.add_argument("--models", default="160,224")
    ap.add_argument("--windows_per_batch", type=int, default=32)
    ap.add_argument("--precision", default="mean")
    a = ap.parse_args()
    from mertools_amd.encoders import HipVideoMAEFinetuneModel as M
    from mertools_amd.extract.sun_videomae import plan_views
    from mertools_amd.extract.visual import extract_sun_videomae
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        fd = os.path.join(tmp, "faces")
        for i in range(a.videos):
            os.makedirs(os.path.join(fd, f"v{i:04d}"))
            np.save(os.path.join(fd, f"v{i:04d}", f"v{i:04d}.npy"), rng.integers(0, 256, size=(a.frames, a.size, a.size, 3), dtype=np.uint8))
        ck = synthetic_checkpoint()
        for S in (int(s) for s in a.models.split(",")):
            model = M.from_state_dict(ck, model=f"vit_base_patch16_{S}", device=dev, precision=a.precision, self_check=False)
            warm = os.path.join(tmp, "warm")
            extract_sun_videomae(model, fd, warm, "UTTERANCE", vids=["v0000"], skip_existing=False)
            for level in a.levels.split(","):
                plan = plan_views(a.frames, level)
                out = os.path.join(tmp, f"{S}-{level}")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                extract_sun_videomae(model, fd, out, level, windows_per_batch=a.windows_per_batch)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                fwd = len(plan.windows)
                flops = a.videos * fwd * view_flops(S)
                print(json.dumps(dict(model=f"vit_base_patch16_{S}", level=level, precision=a.precision, videos=a.videos, frames=a.frames,
                                      frame_size=a.size, seconds=round(dt, 3), videos_per_s=round(a.videos / dt, 2),
                                      forwards_per_video=fwd, reference_forwards_per_video=plan.n_items,
                                      gflop_per_view=round(view_flops(S) / 1e9, 1), achieved_tflops=round(flops / dt / 1e12, 1))), flush=True)
            del model


if __name__ == "__main__":
    main()
