"""What the case table of tests/test_encoder_compose_gpu.py reaches (no GPU).

encoder_compose.expected_path restates tf_forward's dispatch from include/mer_hip.h — the QKV form, the attention kernel, the FFN
form, what every GEMM's pass code turns into, CLS-only and its `tiles` condition.  This file asserts that the GPU case table
reaches every value of every field, and that the two widths no model ever ran (192, 384) land on the branches they are there for."""
import encoder_compose as EC


def _paths():
    """[(what, path dict, rows, T)] for every block configuration of every GPU case."""
    out = []
    for k in EC.BERT_CASES:
        c = EC.tf_cfg(k["D"], k["F"], k["layers"], pre_ln=False, act="gelu", eps=1e-5, dtype=k["dtype"], preset=k["preset"], mx_skip=k["skip"])
        B, T = k["rows"]
        out.append(("bert", k, EC.expected_path(c, T=T, Bseq=B), B * T, T))
    for k in EC.HUBERT_CASES:
        c = EC.tf_cfg(k["D"], k["F"], 2, pre_ln=k["stable"], act="gelu", eps=1e-5, dtype=k["dtype"], preset=k["preset"], mx_skip=k["skip"],
                      gated=k["wavlm"])
        T = 24 if k["L"] == 8000 else 12
        out.append(("hubert", k, EC.expected_path(c, T=T, Bseq=k["B"], score_bias=k["wavlm"]), k["B"] * T, T))
    for k in EC.CLIP_CASES:
        c = EC.tf_cfg(k["D"], k["F"], 2, pre_ln=True, act="quick_gelu", eps=1e-5, dtype=k["dtype"], preset=k["preset"], mx_skip=k["skip"])
        T = (k["image"] // k["patch"]) ** 2 + 1
        cls = EC.vit_cls_only(c, T)
        for blk in (0, 1):
            out.append(("clip", k, EC.expected_path(c, block=blk, T=T, Bseq=k["N"], cls_only=cls), k["N"] * T, T))
        out.append(("clip-tokens", k, EC.expected_path(c, block=1, T=T, Bseq=k["N"], cls_only=False), k["N"] * T, T))
    for kind, D, preset, skip in EC.TOKSUM_CASES:
        F = (int(D * 4 * 2 / 3) + 7) // 8 * 8 if kind == "dinov2" else 256
        c = EC.tf_cfg(D, F, 2, pre_ln=True, act="gelu", eps=1e-6, dtype="f16", preset=preset, mx_skip=skip, swiglu=kind == "dinov2")
        T = 5 if kind == "dinov2" else 17
        out.append((kind, dict(D=D, preset=preset, skip=skip), EC.expected_path(c, T=T, Bseq=3, score_bias=kind == "d2v"), 3 * T, T))
    for D, F, preset, skip in EC.VMAE_CASES:
        c = EC.tf_cfg(D, F, 2, pre_ln=True, act="gelu", eps=1e-12, dtype="f16", preset=preset, mx_skip=skip)
        out.append(("videomae", dict(D=D, preset=preset, skip=skip), EC.expected_path(c, T=18, Bseq=2), 36, 18))
    return out


def test_case_table_reaches_every_branch():
    paths = _paths()
    reached = {"qkv": set(), "attention": set(), "ffn": set(), "cls_only": set(), "tiles": set(), "corr": set()}
    per_gemm = {}
    for _, _, p, _, _ in paths:
        for f in ("qkv", "attention", "ffn", "cls_only", "tiles"):
            reached[f].add(p[f])
        for g, kind in p["corr"].items():
            reached["corr"].add(kind.split(" ")[0])
            per_gemm.setdefault(g, set()).add(kind)
    assert reached["qkv"] == {"fused", "fused fp32", "split: qk one pass + v", "cls: kv + q"}
    assert reached["attention"] == {"plain", "f32", "bias", "bias+gate", "cls"}
    assert reached["ffn"] == {"plain", "swiglu"}
    assert reached["cls_only"] == {True, False}
    assert reached["tiles"] == {True, False, None}
    # what a pass code can turn into: plain 1 / 2 / 3 passes, the MX kernel, its two-pass stand-in, the table over one / two passes
    assert reached["corr"] == {"1", "2", "3", "mx", "2(mx)", "tab1", "tab2"}
    # the fused QKV table with and without the uncorrected Q | K columns, for both table forms
    assert {k for k in per_gemm["qkv"] if k.startswith("tab")} >= {"tab1 n_first=0", "tab2 n_first=0"} | \
        {k for D in (128, 192, 256, 384) for k in ("tab1 n_first=%d" % (2 * D),)}
    assert any(k.startswith("tab2 n_first=") and not k.endswith("=0") for k in per_gemm["qkv"])
    # every GEMM of the block runs corrected AND uncorrected (mx_skip bits 1 / 2 for the FFN), every sub-range GEMM both of its forms
    for g in ("fc1", "fc2"):
        assert per_gemm[g] >= {"1", "2", "3", "2(mx)", "tab1", "tab2"}, (g, per_gemm[g])
    assert "mx" in per_gemm["fc1"] and "mx" in per_gemm["fc2"]
    assert per_gemm["v"] == {"mx", "2(mx)"}           # D 256 / 384 reach the MX kernel (N >= 192), D 128 its stand-in
    assert per_gemm["kv"] >= {"mx", "2(mx)", "tab1", "tab2", "1", "2"}
    assert per_gemm["q"] >= {"2(mx)", "tab1", "tab2", "1", "2"} and "mx" not in per_gemm["q"]
    assert per_gemm["wo"] >= {"1", "2", "3", "mx", "2(mx)", "tab1", "tab2"}


def test_case_table_reaches_the_row_and_preset_edges():
    paths = _paths()
    presets = {k["preset"] for _, k, _, _, _ in paths}
    assert presets >= set(EC.PUBLIC_PRESETS) | {"mean_a2f", "x3_conv4", "mean_all", "mean_conv"}
    assert {k["preset"] for k in EC.HUBERT_CASES} >= {"x3_conv4", "mean_all", "mean_conv", "mean", "mx", "mean_conv3", "a2_conv3", "accurate", "fast"}
    for fam in ("bert", "clip"):
        skips = {k["skip"] for f, k, _, _, _ in paths if f == fam}
        assert skips >= {0, 1, 2, 4, 7}, (fam, skips)
        # ... and bits 1 / 2 on their own sit on pass codes that read them (4 / 5): fc1 / fc2 alone loses its correction
        for bit, g, other in ((2, "fc1", "fc2"), (4, "fc2", "fc1")):
            alone = [p for f, k, p, _, _ in paths if f == fam and k["skip"] == bit]
            assert alone and all(p["corr"][g] == "1" and p["corr"][other] != "1" for p in alone), (fam, bit)
    assert {k["dtype"] for k in EC.BERT_CASES} == {"f16", "bf16"}
    assert any(k["dtype"] == "bf16" and k["preset"] == "mx" for k in EC.BERT_CASES)        # the MX preset on two passes
    assert any(k["layers"] == 7 and k["D"] == 128 for k in EC.BERT_CASES)                 # the ring of 5 wraps
    assert all(k["layers"] == 2 for k in EC.BERT_CASES if k["D"] != 128)
    for D in (128, 192, 256, 384):
        rows = {(r >= 1024 and T >= 40, r < 1024 and T < 40) for f, k, _, r, T in paths if f == "bert" and k["D"] == D}
        assert (True, False) in rows and (False, True) in rows, D                         # per width: >= 1024 rows of T >= 40, and a ragged T < 40
        assert any(k["F"] == 320 for f, k, _, _, _ in paths if k["D"] == D and f in ("bert", "clip"))   # fc2 with K % 128 != 0
    assert max(r for _, _, _, r, _ in paths) == 1088                                      # CLIP N = 64 at D = 256: the largest launch
    assert {(k["image"], k["patch"]) for k in EC.CLIP_CASES} == {(64, 16), (56, 14)}
    assert {k["N"] for k in EC.CLIP_CASES} == {5, 64}
    assert {k["L"] for k in EC.HUBERT_CASES} == {4000, 8000} and {k["norm"] for k in EC.HUBERT_CASES} == {"group", "layer"}
    assert any(k["ragged"] for k in EC.HUBERT_CASES) and any(k["wavlm"] and k["stable"] for k in EC.HUBERT_CASES)
    assert max(k["D"] for _, k, _, _, _ in paths) == 384


def _tf(D, preset, skip, dtype="f16", F=256):
    return EC.tf_cfg(D, F, 2, pre_ln=True, act="gelu", eps=1e-5, dtype=dtype, preset=preset, mx_skip=skip)


def test_widths_192_and_384_land_where_claimed():
    # 192: 2D % 256 != 0 and K = D % 128 != 0 -> no V split and no MX plane for any D-deep GEMM (the MX preset's two-pass stand-in);
    # only fc2 (K = ffn = 256, N = 192) keeps the MX kernel — and loses it at ffn 320
    p = EC.expected_path(_tf(192, "mx", 1))
    assert p["qkv"] == "fused" and p["corr"] == {"qkv": "2(mx)", "wo": "2(mx)", "fc1": "2(mx)", "fc2": "mx"}
    assert EC.expected_path(_tf(192, "mx", 1, F=320))["corr"]["fc2"] == "2(mx)"
    # 384: 2D % 256 == 0 -> V split, V starts at tile 3 of the fused plane (whose last tile is partial) and reaches the MX kernel
    p = EC.expected_path(_tf(384, "mx", 1))
    assert p["qkv"] == "split: qk one pass + v" and p["corr"]["v"] == "mx" and p["corr"]["qk"] == "1"
    assert (2 * 384) // 256 == 3 and (3 * 384) % 256 != 0
    # ... but D % 256 != 0: the CLS-only block's K | V GEMM gets no MX / pre-blocked plane and runs two passes; at 256 it keeps the MX kernel
    p = EC.expected_path(_tf(384, "mx", 7), block=1, cls_only=True)
    assert p["tiles"] is False and p["corr"]["kv"] == "2(mx)" and p["corr"]["q"] == "2(mx)" and p["corr"]["wo"] == "mx"
    p = EC.expected_path(_tf(256, "mx", 7), block=1, cls_only=True)
    assert p["tiles"] is True and p["corr"]["kv"] == "mx" and p["corr"]["q"] == "2(mx)"
    # 128: 2D % 256 == 0 -> split, V at tile 1 of a 1.5-tile plane, N = 128 < 192 -> the stand-in
    p = EC.expected_path(_tf(128, "mx", 1))
    assert p["qkv"] == "split: qk one pass + v" and p["corr"]["v"] == "2(mx)"
    # bf16 never carries an MX plane
    assert set(EC.expected_path(_tf(256, "mx", 1, "bf16"))["corr"].values()) == {"2(mx)"}


def test_documented_degradations():
    # no sequence structure (CLIP's projection, BERT's emb_dim projection): 5 -> 4 -> 2, 6 -> 3
    assert EC.corr_kind(5, a_lo=False, w_lo=True, w_mx=False, seq=False) == "2(mx)"
    assert EC.corr_kind(6, a_lo=True, w_lo=True, w_mx=False, seq=False) == "3"
    assert EC.corr_kind(6, a_lo=False, w_lo=True, w_mx=False, seq=True) == "tab1"       # passes 6 without a lo activation plane is 5
    assert EC.corr_kind(5, a_lo=False, w_lo=False, w_mx=False, seq=True) == "1"
    # mx_skip only selects under passes 4 / 5: bits 1 / 2 leave a passes == 6 FFN corrected
    p = EC.expected_path(EC.tf_cfg(256, 256, 2, pre_ln=False, act="gelu", eps=1e-5, dtype="f16", preset="mean_a2", mx_skip=7))
    assert p["corr"]["fc1"] == "tab2" and p["corr"]["fc2"] == "tab2" and p["corr"]["qkv"] == "tab2 n_first=512"
    p = EC.expected_path(EC.tf_cfg(256, 256, 2, pre_ln=False, act="gelu", eps=1e-5, dtype="f16", preset="mean", mx_skip=7))
    assert p["corr"]["fc1"] == "1" and p["corr"]["fc2"] == "1" and p["corr"]["wo"] == "tab1"
    # the CLS-only path is off under fp32 attention and when token states are asked for
    assert not EC.vit_cls_only(_tf(256, "accurate", 7), 17) and not EC.vit_cls_only(_tf(256, "mean_a2f", 7), 17)
    assert EC.vit_cls_only(_tf(256, "mean_a2", 7), 17) and not EC.vit_cls_only(_tf(256, "mean", 7), 17, tokens_out=True)
    assert not EC.vit_cls_only(_tf(256, "mean", 7), 585)
