"""MER2024's fine-tuned VideoMAE extractor on the GPU: mer_video_patchify_u8 against mer_video_patchify of the host pixels (bit for
bit), the driver against the reference's own outputs (tests/golden/sun_videomae.npz) and against the CPU fp32 oracle on base-size
models, the exactness of the view dedup, and the driver's file handling."""
import os

import numpy as np
import pytest
import torch

from mertools_amd.extract import sun_videomae as SV
from oracle import encoders_ref as R
from oracle import weights as W
from util import dim_rel, rel_err

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sun_videomae.npz")
TOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def golden_sd(gold, with_norm=True):
    sd = {k[2:]: torch.from_numpy(v).float() for k, v in gold.items() if k.startswith("w/")}
    return sd if with_norm else {k: v for k, v in sd.items() if not k.startswith("encoder.norm.")}


def tiny(gold, dev, precision="mean", with_norm=True):
    from mertools_amd.encoders import HipVideoMAEFinetuneModel as M
    return M.from_state_dict(golden_sd(gold, with_norm), model="tiny", img_size=16, patch_size=8, device=dev, precision=precision,
                             self_check=False)


def face_dir(root, videos):
    for vid, fr in videos.items():
        os.makedirs(os.path.join(root, vid), exist_ok=True)
        np.save(os.path.join(root, vid, f"{vid}.npy"), fr)
    return str(root)


@pytest.mark.parametrize("S", [160, 224])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("lo", [True, False])
def test_patchify_u8_bit_exact(dev, S, dtype, lo):
    from mertools_amd import _lib
    from mertools_amd.ops import dt_code, stream
    from mertools_amd.extract.sun_videomae import MEAN, STD
    import ctypes as C
    lib = _lib.lib()
    rng = np.random.default_rng(S)
    Nt, B, F, P, ts = 21, 3, 16, 16, 2
    table = rng.integers(0, 256, size=(Nt, S, S, 3), dtype=np.uint8)
    idx = rng.integers(0, Nt, size=(B, F)).astype(np.int32)
    px = torch.stack([SV.host_pixels(table, idx[b]) for b in range(B)]).permute(0, 2, 1, 3, 4).contiguous().to(dev)   # [B, F, C, S, S]
    rows, cols = B * (F // ts) * (S // P) ** 2, 3 * ts * P * P
    t16 = torch.float16 if dtype == "f16" else torch.bfloat16
    want = [torch.empty((rows, cols), dtype=t16, device=dev) for _ in range(2)]
    got = [torch.full((rows, cols), 7.0, dtype=t16, device=dev) for _ in range(2)]
    _lib.check(lib.mer_video_patchify(px.data_ptr(), B, F, 3, S, S, P, ts, want[0].data_ptr(), want[1].data_ptr() if lo else None,
                                      dt_code(dtype), stream()), "mer_video_patchify")
    tab, ix = torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev)
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    _lib.check(lib.mer_video_patchify_u8(tab.data_ptr(), Nt, S, ix.data_ptr(), B, F, C.addressof(m3), C.addressof(s3), P, ts,
                                         got[0].data_ptr(), got[1].data_ptr() if lo else None, dt_code(dtype), stream()), "mer_video_patchify_u8")
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16))
    if lo:
        assert torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))
    else:
        assert bool((got[1] == 7.0).all())   # no lo plane asked for: none written


@pytest.mark.parametrize("precision,tol", [("mean", TOL), ("accurate", 2e-5)])
@pytest.mark.parametrize("with_norm", [True, False])
def test_tiny_golden_through_driver(gold, dev, tmp_path, precision, tol, with_norm):
    """Non-square 20 x 24 frames: the GPU bilinear resize, the u8 gather, the model and the host reduction together reproduce the
    reference's final_test outputs."""
    from mertools_amd.extract.visual import extract_sun_videomae
    m = tiny(gold, dev, precision, with_norm)
    fd = face_dir(tmp_path / "faces", {f"v{N}": gold[f"video_{N}"] for N in (12, 20)})
    for level in ("UTTERANCE", "FRAME"):
        out = tmp_path / level
        extract_sun_videomae(m, fd, str(out), level, windows_per_batch=5)
        for N in (12, 20):
            got = np.load(out / f"v{N}.npy")
            ref = gold[f"feat_{'norm' if with_norm else 'nonorm'}_{level[:3]}_{N}"]
            assert got.dtype == np.float64 and got.shape == ref.shape
            e = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"sun-videomae tiny[{precision}, norm={with_norm}] {level} N={N}: {e:.2e}")
            assert e <= tol, (level, N, e)


def checkpoint_from_hf(sd, layers):
    """A synthetic HF-layout VideoMAE state dict in the fine-tuning checkpoint's layout (what remap_state_dict undoes)."""
    ck = {"encoder.patch_embed.proj.weight": sd["embeddings.patch_embeddings.projection.weight"],
          "encoder.patch_embed.proj.bias": sd["embeddings.patch_embeddings.projection.bias"],
          "encoder.norm.weight": sd.get("layernorm.weight", torch.ones(sd["embeddings.patch_embeddings.projection.bias"].shape)),
          "encoder.norm.bias": sd.get("layernorm.bias", torch.zeros(sd["embeddings.patch_embeddings.projection.bias"].shape)),
          "head.weight": torch.zeros(6, sd["embeddings.patch_embeddings.projection.bias"].shape[0])}
    for l in range(layers):
        a, q, b = f"encoder.layer.{l}.attention.attention.", f"encoder.layer.{l}.", f"encoder.blocks.{l}."
        ck[b + "attn.qkv.weight"] = torch.cat([sd[a + "query.weight"], sd[a + "key.weight"], sd[a + "value.weight"]], 0)
        ck[b + "attn.q_bias"], ck[b + "attn.v_bias"] = sd[a + "query.bias"], sd[a + "value.bias"]
        ck[b + "attn.proj.weight"], ck[b + "attn.proj.bias"] = sd[q + "attention.output.dense.weight"], sd[q + "attention.output.dense.bias"]
        ck[b + "norm1.weight"], ck[b + "norm1.bias"] = sd[q + "layernorm_before.weight"], sd[q + "layernorm_before.bias"]
        ck[b + "norm2.weight"], ck[b + "norm2.bias"] = sd[q + "layernorm_after.weight"], sd[q + "layernorm_after.bias"]
        ck[b + "mlp.fc1.weight"], ck[b + "mlp.fc1.bias"] = sd[q + "intermediate.dense.weight"], sd[q + "intermediate.dense.bias"]
        ck[b + "mlp.fc2.weight"], ck[b + "mlp.fc2.bias"] = sd[q + "output.dense.weight"], sd[q + "output.dense.bias"]
    return ck


@pytest.mark.parametrize("model,layers", [("vit_base_patch16_160", 12), ("vit_base_patch16_224", 4)])
def test_base_models_against_cpu_oracle(dev, tmp_path, model, layers):
    """Base-size models with synthetic weights re-keyed into the checkpoint layout: UTT and FRAME through the driver against the CPU
    fp32 oracle (planner, host PIL resize, host pixels, oracle forward, reduction)."""
    from mertools_amd.encoders import HipVideoMAEFinetuneModel as M
    from mertools_amd.extract.visual import extract_sun_videomae
    S = M.MODELS[model][0]
    cfg = W.videomae_config("base", num_hidden_layers=layers)
    ck = checkpoint_from_hf(W.videomae_state_dict(cfg, 0), layers)
    hf, _ = M.remap_state_dict(ck)
    hcfg = M.config_for(hf, model)
    rng = np.random.default_rng(3)
    N = 30   # FRAME: 13 distinct windows
    video = rng.integers(0, 256, size=(N, 24, 20, 3), dtype=np.uint8)
    video = np.ascontiguousarray(np.repeat(np.repeat(video, 4, 1), 4, 2)[:, :, :, :])   # smooth-ish 96 x 80 frames
    fd = face_dir(tmp_path / "faces", {"a": video})
    resized = np.stack([SV.pil_resize_host(f, S) for f in video])
    refs = {}
    for level in ("UTTERANCE", "FRAME"):
        plan = SV.plan_views(N, level)
        px = torch.stack([SV.host_pixels(resized, w) for w in plan.windows]).permute(0, 2, 1, 3, 4).contiguous()
        with torch.no_grad():
            f = R.videomae_last_hidden_state(hf, hcfg.to_dict(), px).mean(1)
        refs[level] = SV.reduce_views(f.numpy(), plan)
    for prec, tol in (("mean", TOL), ("accurate", 1e-5)):
        m = M.from_state_dict(ck, model=model, device=dev, precision=prec, self_check=False)
        for level in ("UTTERANCE", "FRAME"):
            out = tmp_path / f"{prec}-{level}"
            extract_sun_videomae(m, fd, str(out), level)
            got = np.load(out / "a.npy")
            ref = refs[level]
            assert got.shape == ref.shape and got.dtype == np.float64
            e = rel_err(torch.from_numpy(got), torch.from_numpy(ref))[0]
            # (dim_rel: per-dimension RMS over the frames — a FRAME figure; one UTT row has no spread to measure it on)
            dr = dim_rel(torch.from_numpy(got), torch.from_numpy(ref)) if level == "FRAME" else float("nan")
            print(f"sun-videomae {model} ({layers} blocks)[{prec}] {level}: max-norm {e:.2e} dim_rel {dr:.2e}")
            assert e <= tol, (prec, level, e)
            if prec == "mean" and level == "FRAME":
                assert dr <= 2e-2, (level, dr)
        del m


def test_dedup_and_batching_are_exact(gold, dev, tmp_path):
    from mertools_amd.extract.visual import extract_sun_videomae
    m = tiny(gold, dev)
    rng = np.random.default_rng(5)
    videos = {f"v{n}": rng.integers(0, 256, size=(n, 28, 22, 3), dtype=np.uint8) for n in (1, 9, 17, 30)}
    fd = face_dir(tmp_path / "faces", videos)
    for level in ("UTTERANCE", "FRAME"):
        runs = {"dedup": dict(dedup=True), "all_views": dict(dedup=False, windows_per_batch=64),
                "one_per_group": dict(videos_per_group=1, windows_per_batch=1), "one_group": dict(videos_per_group=64, windows_per_batch=512)}
        outs = {}
        for name, kw in runs.items():
            d = tmp_path / f"{level}-{name}"
            extract_sun_videomae(m, fd, str(d), level, **kw)
            outs[name] = {v: open(d / f"{v}.npy", "rb").read() for v in videos}
        for name in runs:
            assert outs[name] == outs["dedup"], (level, name)
        a = np.load(tmp_path / f"{level}-one_per_group" / "v30.npy")
        b = np.load(tmp_path / f"{level}-one_group" / "v30.npy")
        assert np.abs(a - b).max() == 0.0


def test_driver_on_synthetic_face_dir(gold, dev, tmp_path):
    from mertools_amd.extract.visual import extract_sun_videomae
    m = tiny(gold, dev)
    rng = np.random.default_rng(7)
    Ns = (1, 9, 12, 17, 40, 80)
    videos = {f"vid{n:02d}": rng.integers(0, 256, size=(n, 112, 112, 3), dtype=np.uint8) for n in Ns}
    fd = face_dir(tmp_path / "faces", videos)
    for level in ("UTTERANCE", "FRAME"):
        out = tmp_path / level
        os.makedirs(out)
        sentinel = np.arange(3.0)
        np.save(out / "vid09.npy", sentinel)   # exists already: left alone
        written = extract_sun_videomae(m, fd, str(out), level, workers=2)
        assert sorted(os.path.basename(p) for p in written) == sorted(f"{v}.npy" for v in videos if v != "vid09")
        assert sorted(os.listdir(out)) == sorted(f"{v}.npy" for v in videos)
        assert np.array_equal(np.load(out / "vid09.npy"), sentinel)
        for v, fr in videos.items():
            if v == "vid09":
                continue
            a = np.load(out / f"{v}.npy")
            assert a.dtype == np.float64
            assert a.shape == ((128,) if level == "UTTERANCE" else (len(fr), 128))
        # two ranks' shares cover the set, each file once
        shares = []
        for r in range(2):
            d = tmp_path / f"{level}-rank{r}"
            shares.append(set(os.path.basename(p) for p in extract_sun_videomae(m, fd, str(d), level, rank=r, world=2)))
        assert not (shares[0] & shares[1]) and shares[0] | shares[1] == set(f"{v}.npy" for v in videos)
        for v in videos:
            if v != "vid09":
                r = 0 if f"{v}.npy" in shares[0] else 1
                assert open(tmp_path / f"{level}-rank{r}" / f"{v}.npy", "rb").read() == open(out / f"{v}.npy", "rb").read()
    empty = face_dir(tmp_path / "empty", {"z": np.zeros((0, 112, 112, 3), dtype=np.uint8)})
    with pytest.raises(ValueError, match="z.npy"):
        extract_sun_videomae(m, empty, str(tmp_path / "z_out"), "UTTERANCE")
    bad = face_dir(tmp_path / "bad", {"f": np.zeros((4, 112, 112, 3), dtype=np.float32)})
    with pytest.raises(ValueError, match="f.npy"):
        extract_sun_videomae(m, bad, str(tmp_path / "f_out"), "FRAME")


def test_finetune_call_takes_reference_layout(gold, dev):
    """__call__ on float pixels [B, C, T, H, W] == forward_frames on the u8 table they came from (same planes: bit for bit)."""
    m = tiny(gold, dev)
    rng = np.random.default_rng(11)
    table = rng.integers(0, 256, size=(20, 16, 16, 3), dtype=np.uint8)
    idx = np.stack([np.arange(16), np.arange(4, 20)]).astype(np.int32)
    px = torch.stack([SV.host_pixels(table, w) for w in idx])   # [2, 3, 16, 16, 16]
    a = m(px.to(dev))
    b = m.forward_frames(torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev))[1]
    torch.cuda.synchronize()
    assert a.shape == (2, 128) and torch.equal(a, b)
