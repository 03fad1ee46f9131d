#!/usr/bin/env python3
"""Generates tests/golden/sun_videomae.npz by RUNNING THE REFERENCE'S OWN CODE (MER2024/feature_extraction/visual/videomae):
VideoClsDatasetFrame (kinetics.py), VisionTransformer (modeling_finetune.py), utils.load_state_dict and final_test
(engine_for_finetuning.py), imported from the read-only reference tree with stubs for the absent cv2 / torchvision / timm /
tensorboardX.  Nothing is copied.  Like gen_golden.py it only runs where the reference is; the output is committed.

Contents:
  frames_{UTT|FRAME}_{N}   int32 [items, 16]  the source frame of every time step of every item, in item order, for
                           N in NS (read back from __getitem__'s output on frames whose pixels are their frame number)
  video_{N}                uint8 [N, 20, 24, 3] non-square frames (N in PX_NS)
  px_{UTT|FRAME}_{N}       float32 [3, 16, S, S] __getitem__(0) of that video
  px_item_{UTT|FRAME}_{N}  the item index px_ is of
  w/<key>                  a tiny ViT (D 128, 2 heads, 2 blocks, MLP 256, patch 8 at 16^2: 32 tokens) in the checkpoint's key layout
                           ('encoder.' prefix, a 'decoder.*' key), float16-representable values stored as float16
  feat_{norm|nonorm}_{UTT|FRAME}_{N}  float64  final_test's saved array for video_N, with and without the checkpoint's norm.*
"""
import argparse
import importlib.machinery
import os
import sys
import tempfile
import types
from functools import partial

import numpy as np
import torch

REF = "/root/reference/MER2024/feature_extraction/visual"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
NS = (1, 9, 12, 16, 17, 20, 27, 70)
PX_NS = (12, 20)
S, P, D, HEADS, DEPTH, MLP = 16, 8, 128, 2, 2, 256


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def stubs():
    """Only what the imported reference modules touch at import time or on the test path."""
    import collections.abc
    from unittest import mock

    def to_2tuple(x):
        return tuple(x) if isinstance(x, collections.abc.Iterable) else (x, x)

    def drop_path(x, drop_prob=0.0, training=False):
        assert not training or drop_prob == 0.0
        return x
    _mod("timm")
    _mod("timm.models")
    _mod("timm.models.layers", drop_path=drop_path, to_2tuple=to_2tuple, trunc_normal_=lambda t, std=1.0, **k: torch.nn.init.trunc_normal_(t, std=std))
    _mod("timm.models.registry", register_model=lambda f: f)
    _mod("timm.utils", get_state_dict=lambda m, *a, **k: m.state_dict())
    for name in ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "tensorboardX"):
        if name not in sys.modules:
            m = mock.MagicMock()
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            sys.modules[name] = m
    import torch as _t
    if "torch._six" not in sys.modules:
        _mod("torch._six", inf=float("inf"))
    _t._six = sys.modules["torch._six"]
    if REF not in sys.path:
        sys.path.insert(0, REF)


def args_for(level):
    return argparse.Namespace(feature_level=level, debug=False)


def dataset(path, level):
    from videomae.kinetics import VideoClsDatasetFrame
    return VideoClsDatasetFrame(path, None, mode="test", clip_len=16, frame_sample_rate=4, crop_size=S, short_side_size=S,
                                new_height=S, new_width=S, keep_aspect_ratio=True, num_segment=1, num_crop=1,
                                test_num_segment=2, test_num_crop=2, args=args_for(level))


def tiny_checkpoint(seed=0):
    g = torch.Generator().manual_seed(seed)

    def r(*shape, s=0.05):
        return (torch.randn(*shape, generator=g) * s).half()
    sd = {"patch_embed.proj.weight": r(D, 3, 2, P, P, s=0.04), "patch_embed.proj.bias": r(D, s=0.02),
          "norm.weight": (1 + r(D, s=0.1).float()).half(), "norm.bias": r(D, s=0.05),
          "head.weight": r(6, D), "head.bias": r(6), "decoder.pos_embed_extra": r(4)}
    for l in range(DEPTH):
        b = f"blocks.{l}."
        sd.update({b + "norm1.weight": (1 + r(D, s=0.1).float()).half(), b + "norm1.bias": r(D, s=0.05),
                   b + "attn.qkv.weight": r(3 * D, D, s=0.08), b + "attn.q_bias": r(D, s=0.05), b + "attn.v_bias": r(D, s=0.05),
                   b + "attn.proj.weight": r(D, D, s=0.08), b + "attn.proj.bias": r(D, s=0.02),
                   b + "norm2.weight": (1 + r(D, s=0.1).float()).half(), b + "norm2.bias": r(D, s=0.05),
                   b + "mlp.fc1.weight": r(MLP, D, s=0.08), b + "mlp.fc1.bias": r(MLP, s=0.02),
                   b + "mlp.fc2.weight": r(D, MLP, s=0.06), b + "mlp.fc2.bias": r(D, s=0.02)})
    return {("encoder." + k if not k.startswith("decoder.") else k): v for k, v in sd.items()}


def reference_model(ck, with_norm):
    from videomae import utils
    from videomae.modeling_finetune import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer(img_size=S, patch_size=P, embed_dim=D, depth=DEPTH, num_heads=HEADS, mlp_ratio=MLP / D, qkv_bias=True,
                              norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_classes=6, all_frames=16, tubelet_size=2,
                              use_mean_pooling=False, init_scale=0.001)
    sd = {k: v.float() for k, v in ck.items() if with_norm or not k.startswith("encoder.norm.")}
    # extract_sun_videomae.py:309-318: strip backbone. / encoder., then the non-strict load
    sd = {(k[9:] if k.startswith("backbone.") else k[8:] if k.startswith("encoder.") else k): v for k, v in sd.items()}
    if not with_norm:   # the module's own init survives: LayerNorm's ones / zeros
        assert torch.equal(model.norm.weight, torch.ones(D)) and torch.equal(model.norm.bias, torch.zeros(D))
    utils.load_state_dict(model, sd, prefix="")
    return model.eval()


def final_features(model, path, level):
    from videomae.engine_for_finetuning import final_test
    loader = torch.utils.data.DataLoader(dataset(path, level), batch_size=8, num_workers=0, drop_last=False)
    return final_test(loader, model, level, torch.device("cpu"))


def main():
    stubs()
    out = {}
    rng = np.random.default_rng(2024)
    with tempfile.TemporaryDirectory() as tmp:
        for N in NS:
            # frames whose every pixel is the frame's number, already S x S (PIL's resize to the same size is a copy): __getitem__'s
            # float output gives back which source frame each time step of each item read
            idx_path = os.path.join(tmp, f"idx_{N}.npy")
            np.save(idx_path, np.broadcast_to(np.arange(N, dtype=np.uint8)[:, None, None, None], (N, S, S, 3)).copy())
            for level in ("UTTERANCE", "FRAME"):
                ds = dataset(idx_path, level)
                fr = []
                for i in range(len(ds)):
                    x = ds[i][0]   # [3, 16, S, S]
                    v = (x[0, :, 0, 0].double() * 0.229 + 0.485) * 255.0
                    fr.append(np.rint(v.numpy()).astype(np.int32))
                out[f"frames_{level[:3]}_{N}"] = np.stack(fr)
        for N in PX_NS:
            video = rng.integers(0, 256, size=(N, 20, 24, 3), dtype=np.uint8)
            path = os.path.join(tmp, f"v{N}.npy")
            np.save(path, video)
            out[f"video_{N}"] = video
            for level in ("UTTERANCE", "FRAME"):
                ds = dataset(path, level)
                item = len(ds) - 1
                out[f"px_{level[:3]}_{N}"] = ds[item][0].numpy().astype(np.float32)
                out[f"px_item_{level[:3]}_{N}"] = np.int64(item)
        ck = tiny_checkpoint()
        for k, v in ck.items():
            out["w/" + k] = v.numpy()
        for with_norm in (True, False):
            model = reference_model(ck, with_norm)
            for N in PX_NS:
                for level in ("UTTERANCE", "FRAME"):
                    with torch.no_grad():
                        out[f"feat_{'norm' if with_norm else 'nonorm'}_{level[:3]}_{N}"] = final_features(model, os.path.join(tmp, f"v{N}.npy"), level)
    dst = os.path.join(OUT, "sun_videomae.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
