#!/usr/bin/env python3
"""BLOOM text encoder on one GPU: time per layer of HipBloomModel under every precision preset against torch's own
BloomModel(...).half() on the same GPU, run sentence by sentence (batch 1, as the reference's extract_text_huggingface.py:216-233 does)
and as one batch.  Random weights at bloom-7b1 widths (hidden 4096, 32 heads of 128, MLP 4 x hidden) with a few layers; 64 sentences x
32 tokens.  The variants are timed alternately, several rounds; one JSON line with median [min, max] ms per layer of a whole pass over
the 64 sentences.  Usage: bench_bloom_text.py [--layers 4] [--sentences 64] [--tokens 32] [--rounds 7] [--hidden 4096 --heads 32]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--sentences", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--heads", type=int, default=32)
    a = ap.parse_args()
    import transformers as tr
    from mertools_amd.bloom import DEFAULT_PRECISION, LADDER, HipBloomModel
    if not torch.cuda.is_available():
        raise SystemExit("bench_bloom_text.py measures on a GPU; there is none")
    torch.manual_seed(0)
    cfg = tr.BloomConfig(hidden_size=a.hidden, n_head=a.heads, n_layer=a.layers, vocab_size=32000, attn_implementation="eager")
    hf = tr.BloomModel(cfg).eval()
    ids = torch.randint(3, cfg.vocab_size, (a.sentences, a.tokens), generator=torch.Generator().manual_seed(1))
    ours = {p: HipBloomModel.from_hf(hf, precision=p) for p in LADDER}
    half = hf.half().cuda()
    ids_d = ids.cuda()
    lens = [a.tokens] * a.sentences

    def run_ours(p):
        ours[p].extract_utterance(ids_d, lens, 0, None)

    def run_half_b1():
        with torch.no_grad():
            for b in range(a.sentences):
                half(input_ids=ids_d[b:b + 1], output_hidden_states=True)

    def run_half_batch():
        with torch.no_grad():
            half(input_ids=ids_d, output_hidden_states=True)

    variants = {f"hip_{p}": (lambda p=p: run_ours(p)) for p in LADDER}
    variants["torch_fp16_batch1"] = run_half_b1
    variants["torch_fp16_batch"] = run_half_batch
    times = {k: [] for k in variants}
    for k, fn in variants.items():       # warm-up: code objects, algorithm choices, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.layers)
    out = {"bench": "bloom_text", "hidden": a.hidden, "heads": a.heads, "layers": a.layers, "sentences": a.sentences,
           "tokens": a.tokens, "rounds": a.rounds, "default_precision": DEFAULT_PRECISION, "unit": "ms per layer for all sentences",
           "ms_per_layer": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
