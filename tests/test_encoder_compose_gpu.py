"""Encoder forwards against op-level compositions, bit for bit (GPU).

mertools_amd/csrc/encoders.cpp (tf_forward, run_gemm, the four *_plan arenas, the HuBERT / ViT / VideoMAE / BERT forwards) is held
elsewhere to 1e-3 max-norm against the CPU oracle — a bar that a correction read from the wrong tile, a table with the wrong
n_first or a lost valid_rows pointer slips under.  Here every forward is compared with tests/encoder_compose.py: the same recipe,
written from include/mer_hip.h, issued op by op from Python on operands packed independently from the state dict (sub-ranges of
fused planes packed on their own).  The ops' dispatch variants are bit-identical by the project's own tests, so the comparison is
torch.equal; a failure names the layer.

branch of encoders.cpp                                       -> test
  tf_forward, post-LN block (plain / fp32 attention)         -> test_bert_layers_bitwise
  ... V split under mx_skip bit 0, passes == 4 (D 128 / 256 / 384: V at tile 1 / 2 / 3; D 192: no split, no MX plane)
                                                             -> test_bert_layers_bitwise[*-mx-s1-*], test_hubert_layers_bitwise
  ... passes 5 / 6 tables (n_first = 2D / 0, valid_rows, seg_rows >= 40 staged, < 40)  -> test_bert_layers_bitwise[*mean*]
  ... ps1 / ps2 (mx_skip bits 1, 2), fc2 with K % 128 != 0    -> the ffn 320 / skip 2 / 4 / 7 cases
  ... bf16 (the MX preset on two passes)                     -> the bf16 cases
  ... pre-LN block, score bias + WavLM gate (gin32)          -> test_hubert_layers_bitwise (stable / wavlm cases)
  ... SwiGLU FFN, baked attn_bias                            -> test_tokensum_end_to_end
  ... CLS-only block (tiles true / false), strided Q rows    -> test_clip_end_to_end (cls path)
  HsMap ring of 5, last4_pool with < 4 states                -> test_ring_and_last4, test_output_combinations
  bert forward: embeddings, emb_dim projection (no table)    -> test_bert_layers_bitwise (emb cases)
  hubert forward: both conv0 norms, conv GEMMs (conv passes 2 .. 5), projection (fp_tab / fp_passes), ragged valid frames,
      positional conv, stable final LayerNorm                -> test_hubert_layers_bitwise
  vit forward: patchify (592 padded columns), patch table, assemble, post-LN + projection (5 -> 4 -> 2, 6 -> 3), tokens_out
                                                             -> test_clip_end_to_end (both paths), test_tokensum_end_to_end
  videomae forward: tubelet GEMM, add_pos, final LN, pooling -> test_videomae_end_to_end
  Arena / *_plan (guard, poison, ENOMEM, alignment)          -> test_workspace_contract
  CLS-only path vs full path vs the fp64-grade oracle        -> test_cls_only_and_full_path_against_oracle
  `accurate` at the new widths vs oracle/encoders_ref (4e-4) -> test_accurate_anchor_new_widths

Negative controls (test_negative_controls): the composition mis-composed on purpose differs from the forward every time.  Its
max-norm relative distance to the forward's hidden_states[1] — BERT post-LN, mx_skip 1, B 3 x T 24 ragged (lengths 24 / 12 / 17) —
measured on the MI355X; all of them sit under the 1e-3 parity bar (TOL) that was the only check of encoders.cpp before:
  preset   width  drop_table  n_first0   no_valid   v_from_q   two_pass_for_table
  mean     256    3.71e-04    2.47e-04   2.85e-04   2.99e-04   3.35e-04
  mean     384    3.02e-04    2.58e-04   2.26e-04   2.75e-04   3.69e-04
  mx       256    -           -          -          3.34e-04   -      (V's MX / lo planes packed from the Q rows: the wrong-tile mistake)
  mx       384    -           -          -          3.05e-04   -
  mean_a2  256    -           1.03e-04   -          -          -      (mx_skip bit 0 is honoured under passes == 6 as well)
  mean_a2  384    -           1.04e-04   -          -          -
  drop_table: every corrected GEMM of the block issued as ONE pass with the plain bias and the hi planes alone — run_gemm's silent
  fall-back.  two_pass_for_table (an extra, not one of the four): the table replaced by an exact second pass over the `lo` plane,
  a MORE accurate GEMM than the recipe's; its distance is the residual the mean-token correction leaves.
  CLS-only K | V GEMM handed an MX plane at hidden 384 (test_cls_only_kv_planes_follow_the_tile_rule): 2.64e-04 on image_features

Findings on the parent commit: every layer-local and end-to-end comparison is torch.equal and every workspace / ring / output
contract holds — no arithmetic defect in encoders.cpp.  Three contracts the library follows were not stated in include/mer_hip.h
and are now: (1) the CLS-only last block of mer_vit_forward, with its rule that the K | V GEMM reads the MX / pre-blocked planes
only when hidden % 256 == 0 (at 384 a passes == 4 K | V GEMM runs two passes); (2) mx_skip bit 0 is honoured under passes == 6 as
well (n_first = 2 * hidden), which the header gave to passes 4 / 5 alone.  Both are pinned by the last three rows above.
(3) HuBERT's feature projection runs with the per-sequence table behind its LayerNorm under tf.passes 5 / 6 (two MFMA passes where
the conv stack hands over hi + lo planes), and the positional conv runs conv_passes 4 / 5 as 2: now at mer_hubert_config.conv_passes,
pinned by hidden_states[0] of test_hubert_layers_bitwise.  One
defect of the suite itself: tests/test_extract_gpu.py::test_audio_extract_files left extract.audio.MAXLEN at 10000, which failed
tests/test_round6_cpu.py::test_constant_chunks_of_a_long_clip whenever both ran in one process; it now puts the value back.  (tests/test_dist_cpu.py: stand-in encoders made row-count invariant.)
"""

import pytest
import torch

import encoder_compose as EC
from oracle import encoders_ref as R
from oracle import weights as W
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu
TOL, X3 = 1e-3, 4e-4          # tests/test_encoders_gpu.py's bars (no new tolerance in this file)
MER_EINVAL, MER_ENOMEM = -1, -4


def _id(d):
    r = d.get("rows")
    parts = [str(d["D"]), "f%d" % d["F"], d["preset"], "s%d" % d["skip"], d["dtype"]]
    if r is not None:
        parts.append("%dx%d" % r)
    for k in ("layers", "emb", "norm", "L", "image", "N"):
        if d.get(k) not in (None, 2):
            parts.append("%s%s" % (k[0], d[k]))
    for k in ("stable", "wavlm", "ragged"):
        if d.get(k):
            parts.append(k)
    return "-".join(parts)


def _eq(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if not torch.equal(got, want):
        e = rel_err(got, want)[0]
        bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero().flatten()
        raise AssertionError(f"{what}: composition differs from the forward (max-norm rel {e:.3e}, {bad.numel()} of {got.shape[0]} rows, "
                             f"first row {int(bad[0])})")


def _valid_rows(B, T, lens, dev):
    if lens is None:
        return torch.arange(B * T, device=dev)
    return torch.cat([torch.arange(b * T, b * T + int(n), device=dev) for b, n in enumerate(lens)])


# ------------------------------------------------------------------------------------------------------------------------------
# BERT family
# ------------------------------------------------------------------------------------------------------------------------------
def _bert_setup(case, dev, monkeypatch, seed=4):
    from mertools_amd.encoders import HipBertModel
    monkeypatch.setenv("MER_MX_SKIP", str(case["skip"]))
    B, T = case["rows"]
    over = dict(hidden_size=case["D"], num_attention_heads=case["D"] // 64, intermediate_size=case["F"], num_hidden_layers=case["layers"],
                max_position_embeddings=T + 4)
    if case.get("emb"):
        cfg = W.electra_config("tiny", embedding_size=case["emb"], **over)
    else:
        cfg = W.bert_config("tiny", **over)
    sd = W.bert_state_dict(cfg, seed)
    m = HipBertModel(sd, cfg, device=dev, dtype=case["dtype"], precision=case["preset"], self_check=False)
    ids = W.synth_tokens(B, T, vocab=300, seed=8, bos=3, eos=4)
    lens = None
    if (B, T) == EC.SMALL:       # ragged: one row at full length, one at T // 2
        lens = [T, T // 2, 17]
        for b, n in enumerate(lens):
            ids[b, n:] = cfg.pad_token_id
    c = EC.tf_cfg(case["D"], case["F"], case["layers"], pre_ln=False, act=cfg.hidden_act, eps=cfg.layer_norm_eps, dtype=case["dtype"],
                  preset=case["preset"], mx_skip=case["skip"])
    return m, cfg, sd, c, ids.to(dev), lens


@pytest.mark.parametrize("case", EC.BERT_CASES, ids=_id)
def test_bert_layers_bitwise(dev, monkeypatch, case):
    """hidden_states[0] from the composed front end; then every block on its own: block(hidden_states[l]) of the forward's own bits
    must equal hidden_states[l + 1] (valid rows: the header leaves rows >= kv_len unspecified); frames / pooled from the last four."""
    m, cfg, sd, c, ids, lens = _bert_setup(case, dev, monkeypatch)
    B, T = case["rows"]
    D = case["D"]
    ss = [b * T + 1 for b in range(B)]
    sl = [(lens[b] if lens else T) - 2 for b in range(B)]
    hs, fr, pooled = m.forward_raw(ids, lengths=lens, hidden_states=True, frames=True, seg_start=ss, seg_len=sl)
    torch.cuda.synchronize()
    rows = _valid_rows(B, T, lens, dev)
    assert torch.isfinite(hs.view(case["layers"] + 1, B * T, D)[:, rows]).all()
    kv = torch.tensor(lens, dtype=torch.int32, device=dev) if lens else None
    h0 = EC.bert_front(sd, cfg, c, ids, dev)
    _eq(h0[rows], hs[0].view(B * T, D)[rows], "hidden_states[0]")
    layers = EC.bert_layers(sd, case["layers"])
    for l in range(case["layers"]):
        Lw = EC.Layer(c, layers[l], dev)
        y = EC.block(hs[l].view(B * T, D).contiguous(), Lw, B, T, kv_len=kv)
        _eq(y[rows], hs[l + 1].view(B * T, D)[rows], f"hidden_states[{l + 1}] from hidden_states[{l}]")
        assert Lw.trace == EC.expected_path(c, block=l, T=T, Bseq=B), "the path the composition took is not the restated dispatch"
    f2, p2 = EC.last4([hs[i].view(B * T, D) for i in range(case["layers"] + 1)], torch.tensor(ss, dtype=torch.int32, device=dev),
                      torch.tensor(sl, dtype=torch.int32, device=dev))
    _eq(f2[rows], fr[rows], "frames")
    _eq(p2, pooled, "pooled")


# ------------------------------------------------------------------------------------------------------------------------------
# HuBERT / WavLM
# ------------------------------------------------------------------------------------------------------------------------------
def _hubert_setup(case, dev, monkeypatch, layers=None):
    from mertools_amd.encoders import HipHubertModel
    monkeypatch.setenv("MER_MX_SKIP", str(case["skip"]))
    D = case["D"]
    over = dict(hidden_size=D, num_attention_heads=D // 64, intermediate_size=case["F"], num_hidden_layers=layers or case["layers"],
                feat_extract_norm=case["norm"], conv_bias=case["norm"] == "layer", do_stable_layer_norm=case["stable"])
    cfg = W.wavlm_config("tiny", **over) if case["wavlm"] else W.hubert_config("tiny", **over)
    sd = W.hubert_state_dict(cfg, 3)
    m = HipHubertModel(sd, cfg, device=dev, dtype=case["dtype"], precision=case["preset"], self_check=False)
    B, L = case["B"], case["L"]
    wav = W.synth_audio(B, L, seed=11)
    vs = None
    if case["ragged"]:      # full length, about 60 %, and the minimum that still leaves one frame (the conv stack's receptive field: 400)
        vs = [L, int(0.6 * L), 400][:B]
        for b, n in enumerate(vs):
            wav[b, n:] = 0
    c = EC.tf_cfg(D, case["F"], over["num_hidden_layers"], pre_ln=case["stable"], act="gelu", eps=cfg.layer_norm_eps, dtype=case["dtype"],
                  preset=case["preset"], mx_skip=case["skip"], gated=case["wavlm"])
    return m, cfg, sd, c, wav.to(dev), vs


@pytest.mark.parametrize("case", EC.HUBERT_CASES, ids=_id)
def test_hubert_layers_bitwise(dev, monkeypatch, case):
    """Base-style post-LN, large-style stable-LN and WavLM (bias table + gates): hidden_states[0] from the composed front end (both
    conv0 norms, the conv GEMMs under every conv pass code, the projection's table, the batched positional conv), every block on
    its own from the forward's bits, the stable encoder's final LayerNorm, frames / pooled.  In a ragged batch only the frames inside
    each clip's own length are compared (the header leaves the rest unspecified)."""
    m, cfg, sd, c, wav, vs = _hubert_setup(case, dev, monkeypatch)
    B, L, D, nl = case["B"], case["L"], case["D"], c.layers
    T = m.out_frames(L)
    lens = [m.out_frames(v) for v in vs] if vs else None
    if vs:
        assert lens[0] == T and lens[-1] == 1
    ss = [b * T for b in range(B)]
    sl = lens if lens else [T] * B
    hs, fr, pooled = m.forward_raw(wav, hidden_states=True, frames=True, seg_start=ss, seg_len=sl, valid_samples=vs, constant_rows=[])
    torch.cuda.synchronize()
    rows = _valid_rows(B, T, lens, dev)
    assert torch.isfinite(hs.view(nl + 1, B * T, D)[:, rows]).all()
    vsd = torch.tensor(vs, dtype=torch.int32, device=dev) if vs else None
    h0, Tn, tn_len = EC.hubert_front(sd, cfg, c, wav, dev, valid_samples=vsd)
    assert Tn == T
    _eq(h0[rows], hs[0].view(B * T, D)[rows], "hidden_states[0]")
    pb = EC.wavlm_bias(sd, cfg, T, dev)
    layers = EC.hubert_layers(sd, nl)
    y = None
    for l in range(nl):
        Lw = EC.Layer(c, layers[l], dev)
        y = EC.block(hs[l].view(B * T, D).contiguous(), Lw, B, T, kv_len=tn_len, pos_bias=pb)
        assert Lw.trace == EC.expected_path(c, block=l, T=T, Bseq=B, score_bias=pb is not None), "composition path != restated dispatch"
        want = hs[l + 1].view(B * T, D)
        if case["stable"] and l == nl - 1:     # the returned last state is the block's output after the encoder's final LayerNorm
            y = EC.hubert_final_ln(sd, c, y, dev)
        _eq(y[rows], want[rows], f"hidden_states[{l + 1}] from hidden_states[{l}]")
    f2, p2 = EC.last4([hs[i].view(B * T, D) for i in range(nl + 1)], torch.tensor(ss, dtype=torch.int32, device=dev),
                      torch.tensor(sl, dtype=torch.int32, device=dev))
    _eq(f2[rows], fr[rows], "frames")
    _eq(p2, pooled, "pooled")


# ------------------------------------------------------------------------------------------------------------------------------
# the encoders that return final tensors only: end to end
# ------------------------------------------------------------------------------------------------------------------------------
def _clip_setup(case, dev, monkeypatch):
    from mertools_amd.encoders import HipCLIPModel
    monkeypatch.setenv("MER_MX_SKIP", str(case["skip"]))
    D = case["D"]
    cfg = W.clip_config("tiny", hidden_size=D, num_attention_heads=D // 64, intermediate_size=case["F"], num_hidden_layers=case["layers"],
                        image_size=case["image"], patch_size=case["patch"])
    sd = W.clip_state_dict(cfg, 6)
    m = HipCLIPModel(sd, cfg, device=dev, dtype=case["dtype"], precision=case["preset"], self_check=False)
    px = W.synth_frames(case["N"], case["image"], seed=12).to(dev)
    c = EC.tf_cfg(D, case["F"], case["layers"], pre_ln=True, act=cfg.vision_config.hidden_act, eps=cfg.vision_config.layer_norm_eps,
                  dtype=case["dtype"], preset=case["preset"], mx_skip=case["skip"])
    return m, cfg, sd, c, px


def _vit_tokens(m, px, T, D, proj):
    """mer_vit_forward_tokens through the C ABI with tokens_out (which disables the CLS-only path) -> (features, tokens)."""
    from mertools_amd import _lib, ops
    N = px.shape[0]
    feats = torch.empty((N, proj), dtype=torch.float32, device=px.device)
    tok = torch.empty((N, T, D), dtype=torch.float32, device=px.device)
    wp, wn = m._workspace(_lib.lib().mer_vit_workspace_bytes(m._handle, N))
    _lib.check(_lib.lib().mer_vit_forward_tokens(m._handle, px.data_ptr(), N, wp, wn, feats.data_ptr(), None, None, 0, None, tok.data_ptr(),
                                                 ops.stream()), "mer_vit_forward_tokens")
    return feats, tok


@pytest.mark.parametrize("case", EC.CLIP_CASES, ids=_id)
def test_clip_end_to_end(dev, monkeypatch, case):
    """CLIP image_features through the CLS-only path (mer_vit_forward) and through the full path (tokens_out given), each against its
    own composition; the full path's token states too."""
    m, cfg, sd, c, px = _clip_setup(case, dev, monkeypatch)
    T = (case["image"] // case["patch"]) ** 2 + 1
    cls_path = EC.vit_cls_only(c, T)
    feats = m.forward_raw(px)[0]
    f_tok, tok = _vit_tokens(m, px, T, case["D"], cfg.projection_dim)
    torch.cuda.synchronize()
    assert torch.isfinite(feats).all() and torch.isfinite(tok).all()
    tr, tr_full = [], []
    want, _ = EC.clip_forward(sd, cfg, c, px, dev, cls_path=cls_path, traces=tr)
    _eq(want, feats, "image_features (%s path)" % ("CLS-only" if cls_path else "full"))
    want_f, want_x = EC.clip_forward(sd, cfg, c, px, dev, cls_path=False, traces=tr_full)
    for l in range(c.layers):       # the path each composed block took is the restated dispatch
        assert tr[l] == EC.expected_path(c, block=l, T=T, Bseq=case["N"], cls_only=cls_path), f"block {l}"
        assert tr_full[l] == EC.expected_path(c, block=l, T=T, Bseq=case["N"], cls_only=False), f"block {l}, full path"
    _eq(want_x.view(tok.shape), tok, "tokens_out")
    _eq(want_f, f_tok, "image_features (full path, tokens_out given)")


@pytest.mark.parametrize("kind,D,preset,skip", EC.TOKSUM_CASES)
def test_tokensum_end_to_end(dev, monkeypatch, kind, D, preset, skip):
    """DINOv2-giant style SwiGLU blocks and data2vec-vision with a baked attn_bias (shared + per-layer tables): token-sum features
    and the last residual stream."""
    from mertools_amd.encoders import HipData2VecVisionModel, HipDinov2Model
    monkeypatch.setenv("MER_MX_SKIP", str(skip))
    if kind == "dinov2":
        cfg = W.dinov2_config("tiny", hidden_size=D, num_attention_heads=D // 64, num_hidden_layers=2, image_size=28, use_swiglu_ffn=True)
        sd = W.dinov2_state_dict(cfg, 5)
        m = HipDinov2Model(sd, cfg, device=dev, precision=preset, input_size=28, self_check=False)
        S, F = 28, (int(D * cfg.mlp_ratio * 2 / 3) + 7) // 8 * 8
        pos = R.dinov2_pos_embed(sd, vars(cfg), S, S)[0]
    else:
        cfg = W.data2vec_vision_config("tiny", hidden_size=D, num_attention_heads=D // 64, num_hidden_layers=2, use_relative_position_bias=True)
        sd = W.data2vec_vision_state_dict(cfg, 5)
        m = HipData2VecVisionModel(sd, cfg, device=dev, precision=preset, self_check=False)
        S, F = cfg.image_size, cfg.intermediate_size
        pos = torch.zeros((S // cfg.patch_size) ** 2 + 1, D)
    px = W.synth_frames(3, S, seed=13).to(dev)
    c = EC.tf_cfg(D, F, 2, pre_ln=True, act="gelu", eps=cfg.layer_norm_eps, dtype="f16", preset=preset, mx_skip=skip, swiglu=kind == "dinov2")
    feats, tok, _ = m.forward_raw(px, tokens=True)
    torch.cuda.synchronize()
    assert torch.isfinite(tok).all()
    tr = []
    want_f, want_x = EC.tokensum_forward(sd, cfg, c, px, dev, kind, pos, traces=tr)
    assert tr == [EC.expected_path(c, block=l, T=tok.shape[1], Bseq=3, score_bias=kind == "d2v") for l in range(2)]
    _eq(want_x, tok, "last residual stream")
    _eq(want_f, feats, "token-sum features")


@pytest.mark.parametrize("D,F,preset,skip", EC.VMAE_CASES)
def test_videomae_end_to_end(dev, monkeypatch, D, F, preset, skip):
    """VideoMAE last_hidden_state (final LayerNorm in place) and the per-segment means."""
    from mertools_amd.encoders import HipVideoMAEModel
    monkeypatch.setenv("MER_MX_SKIP", str(skip))
    cfg = W.videomae_config("tiny", hidden_size=D, num_attention_heads=D // 64, intermediate_size=F, num_hidden_layers=2, image_size=48,
                            num_frames=4)
    sd = W.videomae_state_dict(cfg, 9)
    m = HipVideoMAEModel(sd, cfg, device=dev, precision=preset, self_check=False)
    px = W.synth_video(2, 4, 48, seed=14).to(dev)
    c = EC.tf_cfg(D, F, 2, pre_ln=True, act="gelu", eps=cfg.layer_norm_eps, dtype="f16", preset=preset, mx_skip=skip)
    NP = m.num_patches
    per = NP // 2
    ss = [b * NP + s * per for b in range(2) for s in range(2)]
    out, pooled = m.forward_raw(px, seg_start=ss, seg_len=[per] * 4)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    tr = []
    want, wp = EC.videomae_forward(sd, cfg, c, px, dev, torch.tensor(ss, dtype=torch.int32, device=dev),
                                   torch.tensor([per] * 4, dtype=torch.int32, device=dev), traces=tr)
    assert tr == [EC.expected_path(c, block=l, T=NP, Bseq=2) for l in range(2)]
    _eq(want, out.view(2 * NP, D), "last_hidden_state")
    _eq(wp, pooled, "segment means")


# ------------------------------------------------------------------------------------------------------------------------------
# negative controls
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 384])
@pytest.mark.parametrize("preset", ["mean", "mx", "mean_a2"])
def test_negative_controls(dev, monkeypatch, preset, D):
    """The bit comparison sees what 1e-3 cannot: the composition mis-composed on purpose (Python only, every read in bounds) —
    table dropped (every corrected GEMM of the block on ONE pass with the plain bias, no lo / MX plane: run_gemm's silent fall-back),
    n_first = 0 where the recipe says 2D, valid_rows omitted on a ragged batch, V's correction built from the Q rows' plane —
    differs from the forward each time ("mx" has no table: its one control is V's MX / lo planes packed from the Q rows;
    "mean_a2": mx_skip bit 0 is honoured under passes == 6 too, so n_first = 0 there is a mis-composition as well).  One more,
    "two_pass_for_table", replaces the table by an exact second pass over the `lo` plane: more accurate than the recipe, and
    still not the recipe — its distance is what the mean-token correction itself leaves.
    The distances are printed; nothing is asserted on their size."""
    case = dict(D=D, F=256, preset=preset, skip=1, dtype="f16", rows=EC.SMALL, layers=2, emb=None)
    m, cfg, sd, c, ids, lens = _bert_setup(case, dev, monkeypatch)
    B, T = case["rows"]
    hs, _, _ = m.forward_raw(ids, lengths=lens, hidden_states=True)
    torch.cuda.synchronize()
    rows = _valid_rows(B, T, lens, dev)
    kv = torch.tensor(lens, dtype=torch.int32, device=dev)
    w0 = EC.bert_layers(sd, 2)[0]
    x = hs[0].view(B * T, D).contiguous()
    want = hs[1].view(B * T, D)[rows]
    assert torch.equal(EC.block(x, EC.Layer(c, w0, dev), B, T, kv_len=kv)[rows], want), "the control itself must match"
    for mis in {"mean": EC.MISCOMPOSE + ("two_pass_for_table",), "mx": ("v_from_q",), "mean_a2": ("n_first0",)}[preset]:
        got = EC.block(x, EC.Layer(c, w0, dev, mis=(mis,)), B, T, kv_len=kv)[rows]
        assert torch.isfinite(got).all()
        print(f"negative control {preset} D={D} {mis}: max-norm rel distance to the forward {rel_err(got, want)[0]:.3e} (TOL {TOL:.0e})")
        assert not torch.equal(got, want), f"mis-composition {mis!r} was not seen by the bit comparison"


def test_cls_only_kv_planes_follow_the_tile_rule(dev, monkeypatch):
    """hidden = 384 under the MX preset: the CLS-only block's K | V GEMM must run WITHOUT an MX plane (the fused plane is stored per
    256-row tile and row 384 is no tile boundary): the composition that hands it one differs from the forward."""
    case = dict(D=384, F=256, preset="mx", skip=1, dtype="f16", image=64, patch=16, N=5, layers=2)
    m, cfg, sd, c, px = _clip_setup(case, dev, monkeypatch)
    feats = m.forward_raw(px)[0]
    torch.cuda.synchronize()
    good, _ = EC.clip_forward(sd, cfg, c, px, dev, cls_path=True)
    bad, _ = EC.clip_forward(sd, cfg, c, px, dev, cls_path=True, mis=("kv_mx",))
    print(f"CLS-only K | V with an MX plane at hidden 384: max-norm rel distance to the forward {rel_err(bad, feats)[0]:.3e} (TOL {TOL:.0e})")
    assert torch.equal(good, feats) and torch.isfinite(bad).all() and not torch.equal(bad, feats)


# ------------------------------------------------------------------------------------------------------------------------------
# workspace and output contracts, through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
class _Fam:
    """One encoder family behind a uniform face: call(ws_ptr, ws_bytes, fill) -> (rc, {name: (tensor, specified rows or None)})."""

    def __init__(self, name, dev, monkeypatch):
        from mertools_amd import _lib, ops
        self.lib, self.ops, self.dev, self.name = _lib.lib(), ops, dev, name
        if name == "bert":
            case = dict(D=128, F=256, preset="mean", skip=1, dtype="f16", rows=EC.SMALL, layers=2, emb=None)
            self.m, _, _, _, self.x, lens = _bert_setup(case, dev, monkeypatch)
            B, T = EC.SMALL
            self.B, self.T, self.D, self.nl = B, T, 128, 2
            self.lens = torch.tensor(lens, dtype=torch.int32, device=dev)
            self.rows = _valid_rows(B, T, lens, dev)
            self.ss = torch.tensor([b * T for b in range(B)], dtype=torch.int32, device=dev)
            self.sl = self.lens.clone()
            self.nbytes = lambda hs: self.lib.mer_bert_workspace_bytes(self.m._handle, B, T, int(hs))
        elif name == "hubert":
            case = dict(D=128, F=256, preset="mean", skip=1, norm="group", stable=False, wavlm=False, L=8000, B=3, ragged=True, dtype="f16", layers=2)
            self.m, _, _, _, self.x, vs = _hubert_setup(case, dev, monkeypatch)
            B, T = 3, self.m.out_frames(8000)
            self.B, self.T, self.D, self.nl = B, T, 128, 2
            lens = [self.m.out_frames(v) for v in vs]
            self.vs = torch.tensor(vs, dtype=torch.int32, device=dev)
            self.rows = _valid_rows(B, T, lens, dev)
            self.ss = torch.tensor([b * T for b in range(B)], dtype=torch.int32, device=dev)
            self.sl = torch.tensor(lens, dtype=torch.int32, device=dev)
            self.nbytes = lambda hs: self.lib.mer_hubert_workspace_bytes(self.m._handle, B, 8000, int(hs))
        elif name == "vit":
            case = dict(D=128, F=256, preset="mean", skip=7, dtype="f16", image=64, patch=16, N=5, layers=2)
            self.m, cfg, _, _, self.x = _clip_setup(case, dev, monkeypatch)
            self.N, self.P = 5, cfg.projection_dim
            self.ss = torch.tensor([0, 2], dtype=torch.int32, device=dev)
            self.sl = torch.tensor([2, 3], dtype=torch.int32, device=dev)
            self.nbytes = lambda hs: self.lib.mer_vit_workspace_bytes(self.m._handle, 5)
        else:
            from mertools_amd.encoders import HipVideoMAEModel
            monkeypatch.setenv("MER_MX_SKIP", "7")
            cfg = W.videomae_config("tiny", image_size=48, num_frames=4)
            self.m = HipVideoMAEModel(W.videomae_state_dict(cfg, 9), cfg, device=dev, precision="mean", self_check=False)
            self.x = W.synth_video(2, 4, 48, seed=14).to(dev)
            self.NP = self.m.num_patches
            self.ss = torch.tensor([0, self.NP], dtype=torch.int32, device=dev)
            self.sl = torch.tensor([self.NP, self.NP], dtype=torch.int32, device=dev)
            self.nbytes = lambda hs: self.lib.mer_videomae_workspace_bytes(self.m._handle, 2)

    def call(self, wp, wn, *, hs=True, frames=True, pooled=True, seg=None, canary=7.25):
        """-> (rc, outputs): every output pre-filled with `canary`; `seg` overrides the (seg_start, seg_len) tensors."""
        dev, lib, st = self.dev, self.lib, self.ops.stream()
        full = lambda *s: torch.full(s, canary, dtype=torch.float32, device=dev)   # noqa: E731
        ss, sl = seg if seg is not None else (self.ss, self.sl)
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        out = {}
        if self.name in ("bert", "hubert"):
            B, T, D = self.B, self.T, self.D
            h = full(self.nl + 1, B * T, D) if hs else None
            f = full(B * T, D) if frames else None
            q = full(ss.numel(), D) if pooled else None
            if self.name == "bert":
                rc = lib.mer_bert_forward(self.m._handle, self.x.data_ptr(), None, self.lens.data_ptr(), B, T, wp, wn, p(h), p(f),
                                          p(ss) if pooled else None, p(sl) if pooled else None, ss.numel() if pooled else 0, p(q), st)
            else:
                rc = lib.mer_hubert_forward_ragged(self.m._handle, self.x.data_ptr(), B, 8000, self.vs.data_ptr(), wp, wn, p(h), p(f),
                                                   p(ss) if pooled else None, p(sl) if pooled else None, ss.numel() if pooled else 0, p(q),
                                                   None, 0, st)
            if hs:
                out["hidden_states"] = (h, self.rows, 1)
            if frames:
                out["frames"] = (f, self.rows, 0)
            if pooled:
                out["pooled"] = (q, None, 0)
        elif self.name == "vit":
            f = full(self.N, self.P) if frames else None
            q = full(ss.numel(), self.P) if pooled else None
            rc = lib.mer_vit_forward(self.m._handle, self.x.data_ptr(), self.N, wp, wn, p(f), p(ss) if pooled else None,
                                     p(sl) if pooled else None, ss.numel() if pooled else 0, p(q), st)
            if frames:
                out["image_features"] = (f, None, 0)
            if pooled:
                out["pooled"] = (q, None, 0)
        else:
            f = full(2 * self.NP, 128) if frames else None
            q = full(ss.numel(), 128) if pooled else None
            rc = lib.mer_videomae_forward(self.m._handle, self.x.data_ptr(), 2, wp, wn, p(f), p(ss) if pooled else None,
                                          p(sl) if pooled else None, ss.numel() if pooled else 0, p(q), st)
            if frames:
                out["last_hidden_state"] = (f, None, 0)
            if pooled:
                out["pooled"] = (q, None, 0)
        torch.cuda.synchronize()
        return rc, out


def _spec(entry):
    """The specified elements of an output (valid rows only where the header calls the rest unspecified)."""
    t, rows, dim = entry
    return t if rows is None else t.index_select(dim, rows)


def _arena(nbytes, dev, extra=4096):
    buf = torch.empty(nbytes + extra + 512, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 256
    return buf, off


@pytest.mark.parametrize("family", ["bert", "hubert", "vit", "videomae"])
def test_workspace_contract(dev, monkeypatch, family):
    """Guard: nothing is written past workspace_bytes.  Poison: the outputs do not depend on what the arena held before (NaN bit
    patterns, zeros, a previous run) and are finite on every specified element.  workspace_bytes - 257 (below the plan: the planner
    adds 256 of slack) -> MER_ENOMEM with every output untouched; a workspace off the 256-byte grid by 128 -> MER_EINVAL."""
    fam = _Fam(family, dev, monkeypatch)
    # two arena layouts where the encoder returns hidden states: the full tensor (want_hidden_states = 1) and the ring of 5 (0)
    for hs in ((True, False) if family in ("bert", "hubert") else (True,)):
        what = f"{family} (hidden_states {'given' if hs else 'NULL: the ring'})"
        n = int(fam.nbytes(hs))
        assert n > 0
        buf, off = _arena(n, dev)
        wp = buf.data_ptr() + off
        tail = buf[off + n: off + n + 4096]
        buf.fill_(0xFF)          # fp32 / f16 / bf16 NaN bit patterns everywhere, the guard tail included
        tail.fill_(0xA5)
        rc, a = fam.call(wp, n, hs=hs)
        assert rc == 0, fam.lib.mer_last_error()
        assert bool((tail == 0xA5).all()), f"{what}: the forward wrote past workspace_bytes"
        buf[off: off + n].zero_()
        rc, b = fam.call(wp, n, hs=hs)
        assert rc == 0
        rc, c2 = fam.call(wp, n, hs=hs)       # two consecutive runs on one workspace
        assert rc == 0
        assert bool((tail == 0xA5).all())
        for k in a:
            sa, sb, sc = _spec(a[k]), _spec(b[k]), _spec(c2[k])
            assert torch.isfinite(sa).all(), f"{what} {k}: non-finite specified elements"
            assert torch.equal(sa, sb), f"{what} {k}: depends on what the workspace held before (NaN-filled vs zero-filled)"
            assert torch.equal(sb, sc), f"{what} {k}: two consecutive runs on one workspace disagree"
        rc, small = fam.call(wp, n - 257, hs=hs)
        assert rc == MER_ENOMEM, f"{what}: workspace_bytes - 257 gave {rc}"
        for k, (t, _, _) in small.items():
            assert bool((t == 7.25).all()), f"{what} {k}: written although the call failed with MER_ENOMEM"
        rc, mis = fam.call(wp + 128, n, hs=hs)      # (the buffer has the room: 4096 + 256 bytes behind the plan)
        assert rc == MER_EINVAL, f"{what}: a workspace misaligned by 128 bytes gave {rc}"
        for k, (t, _, _) in mis.items():
            assert bool((t == 7.25).all())


@pytest.mark.parametrize("family", ["bert", "hubert", "vit", "videomae"])
def test_output_combinations(dev, monkeypatch, family):
    """frames only, pooled only, or both: the same bits; so is a segment that spans two batch rows."""
    fam = _Fam(family, dev, monkeypatch)
    n = int(max(fam.nbytes(True), fam.nbytes(False)))
    buf, off = _arena(n, dev)
    wp = buf.data_ptr() + off
    fk = {"bert": "frames", "hubert": "frames", "vit": "image_features", "videomae": "last_hidden_state"}[family]
    _, both = fam.call(wp, n, hs=False)
    _, f_only = fam.call(wp, n, hs=False, pooled=False)
    _, p_only = fam.call(wp, n, hs=False, frames=False)
    assert torch.equal(_spec(both[fk]), _spec(f_only[fk])), f"{family}: {fk} changes when pooled is asked for too"
    assert torch.equal(both["pooled"][0], p_only["pooled"][0]), f"{family}: pooled changes when {fk} is asked for too"
    # one segment across the boundary of two batch rows (full rows of row 0's tail and row 1's head are valid in every family here)
    rows_per = {"bert": 24, "hubert": fam.T if family == "hubert" else 0, "vit": 1, "videomae": getattr(fam, "NP", 0)}[family]
    if family == "bert":
        start, ln = 20, 10                # rows 20..23 of sequence 0 (length 24) and 0..5 of sequence 1 (length 12)
    elif family == "hubert":
        start, ln = rows_per - 3, 6
    elif family == "vit":
        start, ln = 1, 3
    else:
        start, ln = rows_per - 2, 5
    seg = (torch.tensor([start], dtype=torch.int32, device=dev), torch.tensor([ln], dtype=torch.int32, device=dev))
    _, sp = fam.call(wp, n, hs=False, seg=seg)
    want = fam.ops.sum_pool([sp[fk][0]], seg[0], seg[1])[1]
    assert torch.isfinite(sp["pooled"][0]).all()
    assert torch.equal(sp["pooled"][0], want), f"{family}: a segment spanning two batch rows is not the mean of its {fk} rows"


@pytest.mark.parametrize("family", ["bert", "hubert"])
@pytest.mark.parametrize("layers", [1, 2, 3, 4, 5, 7])
def test_ring_and_last4(dev, monkeypatch, family, layers):
    """hidden_states = NULL runs on the ring of 5 states: frames / pooled must equal those of the run with the full tensor, and
    frames must be mer_sum_pool over the returned last four states (fewer than four: as many as exist)."""
    from mertools_amd import ops
    if family == "bert":
        case = dict(D=128, F=256, preset="mean", skip=1, dtype="f16", rows=EC.SMALL, layers=layers, emb=None)
        m, _, _, _, ids, lens = _bert_setup(case, dev, monkeypatch)
        B, T = EC.SMALL
        ss, sl = [b * T + 1 for b in range(B)], [n - 2 for n in lens]
        run = lambda hs: m.forward_raw(ids, lengths=lens, hidden_states=hs, frames=True, seg_start=ss, seg_len=sl)   # noqa: E731
    else:
        case = dict(D=128, F=256, preset="mean", skip=1, norm="group", stable=False, wavlm=False, L=4000, B=3, ragged=True, dtype="f16", layers=2)
        m, _, _, _, wav, vs = _hubert_setup(case, dev, monkeypatch, layers=layers)
        B, T = 3, m.out_frames(4000)
        lens = [m.out_frames(v) for v in vs]
        ss, sl = [b * T for b in range(B)], lens
        run = lambda hs: m.forward_raw(wav, hidden_states=hs, frames=True, seg_start=ss, seg_len=sl, valid_samples=vs, constant_rows=[])   # noqa: E731
    hs, fr, pooled = run(True)
    _, fr_ring, pooled_ring = run(False)
    torch.cuda.synchronize()
    rows = _valid_rows(B, T, lens, dev)
    assert torch.isfinite(fr[rows]).all() and torch.isfinite(pooled).all()
    assert torch.equal(fr_ring[rows], fr[rows]), f"{family} layers={layers}: frames differ between the ring and the full tensor"
    assert torch.equal(pooled_ring, pooled), f"{family} layers={layers}: pooled differs between the ring and the full tensor"
    D = hs.shape[-1]
    want = ops.sum_pool([hs[i].view(B * T, D) for i in range(max(0, layers - 3), layers + 1)], frames=True)[0]
    assert torch.equal(fr[rows], want[rows]), f"{family} layers={layers}: frames != sum of the returned last four states"


# ------------------------------------------------------------------------------------------------------------------------------
# ties to the fp64-grade oracle (existing tolerances only)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,tol", [("accurate", X3), ("balanced", TOL), ("mx", TOL), ("mean", TOL), ("fast", 2e-3)])
def test_cls_only_and_full_path_against_oracle(dev, monkeypatch, preset, tol):
    """The CLS-only path and the full path differ in arithmetic (mer_attention_cls vs the tiled kernel): no bit claim between them;
    both are held to tests/test_encoders_gpu.py's per-preset bars against oracle.encoders_ref.clip_image_features at D = 256."""
    case = dict(D=256, F=256, preset=preset, skip=7, dtype="f16", image=64, patch=16, N=5, layers=2)
    m, cfg, sd, c, px = _clip_setup(case, dev, monkeypatch)
    ref = R.clip_image_features(sd, dict(vars(cfg.vision_config), projection_dim=cfg.projection_dim), px.cpu())
    feats = m.forward_raw(px)[0]
    f_tok, _ = _vit_tokens(m, px, 17, 256, cfg.projection_dim)
    torch.cuda.synchronize()
    assert_close(feats.cpu(), ref, tol, f"clip-256[{preset}] image features, mer_vit_forward")
    assert_close(f_tok.cpu(), ref, tol, f"clip-256[{preset}] image features, full path")


@pytest.mark.parametrize("D", [192, 256, 384])
def test_accurate_anchor_new_widths(dev, monkeypatch, D):
    """Ties the compositions to an fp64-grade reference at the widths no other test runs: `accurate` against oracle/encoders_ref
    at the suite's X3 = 4e-4 (BERT hidden states on their valid rows, CLIP image features)."""
    case = dict(D=D, F=320, preset="accurate", skip=1, dtype="f16", rows=EC.SMALL, layers=2, emb=None)
    m, cfg, sd, c, ids, lens = _bert_setup(case, dev, monkeypatch)
    B, T = case["rows"]
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).long()
    ref = R.bert_hidden_states(sd, dict(vars(cfg), roberta=True), ids.cpu(), mask)
    hs, _, _ = m.forward_raw(ids, lengths=lens, hidden_states=True)
    torch.cuda.synchronize()
    for i, r in enumerate(ref):
        for b, n in enumerate(lens):
            assert_close(hs[i, b, :n].cpu(), r[b, :n], X3, f"bert-{D}[accurate] hs[{i}] row {b}")
    ccase = dict(D=D, F=320, preset="accurate", skip=7, dtype="f16", image=64, patch=16, N=3, layers=2)
    m2, ccfg, csd, _, px = _clip_setup(ccase, dev, monkeypatch)
    cref = R.clip_image_features(csd, dict(vars(ccfg.vision_config), projection_dim=ccfg.projection_dim), px.cpu())
    out = m2.forward_raw(px)[0]
    torch.cuda.synchronize()
    assert_close(out.cpu(), cref, X3, f"clip-{D}[accurate] image features")
