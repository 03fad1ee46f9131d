"""MER2024's fine-tuned VideoMAE extractor on the host (extract/sun_videomae.py, HipVideoMAEFinetuneModel's checkpoint loader),
against tests/golden/sun_videomae.npz — outputs of the reference's own VideoClsDatasetFrame / VisionTransformer / final_test
(tests/golden/gen_golden_sun_videomae.py).  No GPU."""
import argparse
import os

import numpy as np
import pytest
import torch

from mertools_amd.extract import sun_videomae as SV

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sun_videomae.npz")
NS = (1, 9, 12, 16, 17, 20, 27, 70)


class _NotAllowListed:
    pass


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def golden_checkpoint(gold, with_norm=True):
    sd = {k[2:]: torch.from_numpy(v).float() for k, v in gold.items() if k.startswith("w/")}
    if not with_norm:
        sd = {k: v for k, v in sd.items() if not k.startswith("encoder.norm.")}
    return sd


def oracle_features(hf_sd, cfg, px_items):
    """oracle forward (HF layout) + final LN (in the oracle when layernorm.* is present) + token mean, per item."""
    from oracle import encoders_ref as R
    px = torch.stack([torch.as_tensor(p) for p in px_items]).permute(0, 2, 1, 3, 4).contiguous()   # [B, C, T, H, W] -> [B, T, C, H, W]
    return R.videomae_last_hidden_state(hf_sd, cfg.to_dict(), px).mean(1)


@pytest.mark.parametrize("level", ["UTTERANCE", "FRAME"])
@pytest.mark.parametrize("N", NS)
def test_planner_frames_match_reference(gold, N, level):
    plan = SV.plan_views(N, level)
    got = plan.windows[plan.item_window]
    assert np.array_equal(got, gold[f"frames_{level[:3]}_{N}"])
    assert plan.n_items == (4 if level == "UTTERANCE" else 4 * N)


@pytest.mark.parametrize("level", ["UTTERANCE", "FRAME"])
@pytest.mark.parametrize("N", (12, 20))
def test_host_pixels_bit_exact(gold, N, level):
    video = gold[f"video_{N}"]
    resized = np.stack([SV.pil_resize_host(f, 16) for f in video])
    plan = SV.plan_views(N, level)
    item = int(gold[f"px_item_{level[:3]}_{N}"])
    px = SV.host_pixels(resized, plan.windows[plan.item_window[item]]).numpy()
    ref = gold[f"px_{level[:3]}_{N}"]
    assert px.dtype == np.float32 and px.shape == ref.shape
    assert px.tobytes() == ref.tobytes()


def test_window_counts_n80():
    assert len(SV.plan_views(80, "UTTERANCE").windows) == 2
    assert len(SV.plan_views(80, "FRAME").windows) == 63
    assert SV.plan_views(80, "FRAME").n_items == 320


def test_window_wraps_negative_index():
    """N = 12, frmid = 11: window (N-17, N-1) = (-5, 11); index -5 reads frames[7]."""
    items = SV.item_frames(12, "FRAME")
    fr = [it[3] for it in items if it[0] == 11]
    assert len(fr) == 4 and all(f == fr[0] for f in fr)
    assert fr[0][0] == 7 and fr[0][-1] == 10


@pytest.mark.parametrize("level", ["UTTERANCE", "FRAME"])
@pytest.mark.parametrize("N", (1, 9, 17, 27, 70))
def test_reduce_views_equals_plain_reduction(N, level):
    """reduce_views over distinct windows == final_test's loop over all 4 views of every item, byte for byte."""
    plan = SV.plan_views(N, level)
    rng = np.random.default_rng(N)
    per_window = rng.standard_normal((len(plan.windows), 24)).astype(np.float32)
    got = SV.reduce_views(per_window, plan)
    # the reference's own shape of it (engine_for_finetuning.py:26-45): lists of python floats per '%010d' key
    saved = {}
    for i, w in enumerate(plan.item_window):
        saved.setdefault("%010d" % plan.item_frmid[i], []).append(per_window[w].tolist())
    emb = [np.mean(saved[k], axis=0) for k in sorted(saved)]
    emb = np.array(emb).squeeze()
    if level == "FRAME" and emb.ndim == 1:
        emb = emb[np.newaxis, :]
    if level == "UTTERANCE" and emb.ndim == 2:
        emb = np.mean(emb, axis=0)
    assert got.dtype == np.float64 and got.shape == emb.shape
    assert got.tobytes() == emb.tobytes()
    assert got.shape == ((24,) if level == "UTTERANCE" else (N, 24))


@pytest.mark.parametrize("with_norm", [True, False])
def test_loader_and_oracle_reproduce_reference_features(gold, with_norm, tmp_path):
    from mertools_amd.encoders import HipVideoMAEFinetuneModel as M
    ck = {"model": golden_checkpoint(gold, with_norm), "args": argparse.Namespace(model="tiny", input_size=16)}
    path = tmp_path / "checkpoint-7.pth"
    torch.save(ck, path)
    hf_sd, unused = M.remap_state_dict(M.load_checkpoint(str(path)))
    assert unused == ["decoder.pos_embed_extra", "head.bias", "head.weight"]
    if not with_norm:
        assert torch.equal(hf_sd["layernorm.weight"], torch.ones(128)) and torch.equal(hf_sd["layernorm.bias"], torch.zeros(128))
    cfg = M.config_for(hf_sd, "tiny", img_size=16, patch_size=8)
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers, cfg.intermediate_size) == (128, 2, 2, 256)
    for N in (12, 20):
        resized = np.stack([SV.pil_resize_host(f, 16) for f in gold[f"video_{N}"]])
        for level in ("UTTERANCE", "FRAME"):
            plan = SV.plan_views(N, level)
            with torch.no_grad():
                f = oracle_features(hf_sd, cfg, [SV.host_pixels(resized, w) for w in plan.windows])
            got = SV.reduce_views(f.numpy(), plan)
            ref = gold[f"feat_{'norm' if with_norm else 'nonorm'}_{level[:3]}_{N}"]
            assert got.shape == ref.shape and got.dtype == np.float64
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err < 1e-5, (N, level, err)


def test_checkpoint_with_namespace_loads_weights_only(tmp_path):
    from mertools_amd.encoders import HipVideoMAEFinetuneModel as M
    sd = {"encoder.patch_embed.proj.weight": torch.zeros(64, 3, 2, 16, 16)}
    torch.save({"module": sd, "args": argparse.Namespace(lr=1e-3), "epoch": 3}, tmp_path / "a.pth")
    got = M.load_checkpoint(str(tmp_path / "a.pth"))
    assert list(got) == ["encoder.patch_embed.proj.weight"]
    torch.save(sd, tmp_path / "b.pth")   # neither 'model' nor 'module': the whole dict
    assert list(M.load_checkpoint(str(tmp_path / "b.pth"))) == ["encoder.patch_embed.proj.weight"]
    torch.save({"model": sd, "extra": _NotAllowListed()}, tmp_path / "c.pth")   # never a silent full unpickle
    with pytest.raises(Exception):
        M.load_checkpoint(str(tmp_path / "c.pth"))


def test_layer_scale_folds_and_non_joint_raises(gold):
    from mertools_amd import _lib
    from mertools_amd.encoders import HipVideoMAEFinetuneModel as M
    sd = golden_checkpoint(gold)
    g1, g2 = torch.full((128,), 0.5), torch.linspace(0.1, 1.0, 128)
    hf, _ = M.remap_state_dict(dict(sd, **{"encoder.blocks.0.gamma_1": g1, "encoder.blocks.0.gamma_2": g2}))
    assert torch.equal(hf["encoder.layer.0.attention.output.dense.weight"], g1[:, None] * sd["encoder.blocks.0.attn.proj.weight"])
    assert torch.equal(hf["encoder.layer.0.output.dense.bias"], g2 * sd["encoder.blocks.0.mlp.fc2.bias"])
    assert torch.equal(hf["encoder.layer.0.attention.attention.key.bias"], torch.zeros(128))
    q, k, v = sd["encoder.blocks.1.attn.qkv.weight"].chunk(3, 0)
    assert torch.equal(hf["encoder.layer.1.attention.attention.key.weight"], k)
    with pytest.raises(_lib.MerError, match="joint"):
        M.remap_state_dict(dict(sd, **{"encoder.blocks.0.temporal_attn.qkv.weight": torch.zeros(3)}))


@pytest.mark.parametrize("kw", [dict(attn_type="only_spatial"), dict(use_mean_pooling=True), dict(keep_temporal_dim=True)])
def test_out_of_scope_architectures_raise(gold, kw):
    from mertools_amd import _lib
    from mertools_amd.encoders import HipVideoMAEFinetuneModel as M
    with pytest.raises(_lib.MerError, match="not supported"):
        M.from_state_dict(golden_checkpoint(gold), model="tiny", img_size=16, patch_size=8, device="cpu", **kw)


def test_save_dir_names_match_feature_dirs():
    from mertools_amd.extract.visual import SUN_VIDEOMAE, sun_videomae_save_dir
    from mertools_amd.toolkit.globals import FEATURE_DIR_OF
    for name in ("VideoMAE-base (VoxCeleb2)", "VideoMAE-base (MER2023)"):
        rel, _ = SUN_VIDEOMAE[name]
        d = sun_videomae_save_dir("/feat", os.path.join("tools", rel), "UTTERANCE")
        assert d == os.path.join("/feat", FEATURE_DIR_OF[name] + "-UTT")
        assert sun_videomae_save_dir("/feat", rel, "FRAME").endswith(FEATURE_DIR_OF[name] + "-FRA")
    assert SUN_VIDEOMAE["VideoMAE-base (VoxCeleb2)"][1] == "vit_base_patch16_160"
    assert SUN_VIDEOMAE["VideoMAE-base (MER2023)"][1] == "vit_base_patch16_224"


def test_empty_video_raises():
    with pytest.raises(ValueError):
        SV.plan_views(0, "FRAME")
