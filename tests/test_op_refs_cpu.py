"""Pins the fp64 references of tests/op_refs.py against torch's own operators (CPU only): the GPU op tests are only as good as
the functions they compare with."""
import pytest
import torch
import torch.nn.functional as F

import op_refs as R


def _case(B, T, H, seed, dtype=torch.float16):
    return R.rand((B * T, 3 * H * 64), seed).to(dtype)


@pytest.mark.parametrize("B,T,H,lens", [(2, 50, 2, None), (3, 70, 2, [70, 1, 33]), (2, 129, 3, [100, 129])])
@pytest.mark.parametrize("biased", [False, True])
def test_attention_ref_equals_sdpa(B, T, H, lens, biased):
    qkv = _case(B, T, H, 1)
    bias = gate = None
    mask = torch.zeros(B, H, T, T, dtype=torch.float64)
    if biased:
        bias = F.pad(R.rand((H, T, T), 2), (0, 4), value=1e30)         # pad columns must never reach a score
        gate = R.rand((B, H, T), 3) + 2.0
        mask = mask + gate.double()[..., None] * bias.double()[None, :, :, :T]
    if lens is not None:
        dead = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
        mask = mask.masked_fill(dead[:, None, None, :], float("-inf"))
    q, k, v = [t.double().view(B, T, H, 64).transpose(1, 2) for t in qkv.split(H * 64, dim=1)]
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=0.125).transpose(1, 2).reshape(B, T, H * 64)
    got = R.attention_ref(qkv, B, T, H, 0.125, lens, bias, gate)
    assert torch.isfinite(got).all()
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T,lens", [(70, [70, 1, 17, 69]), (300, [300, 255, 1])])
def test_poison_is_invisible_behind_the_mask_and_loud_without_it(dtype, T, lens):
    B, H = len(lens), 2
    qkv = _case(B, T, H, 4, dtype)
    bad = R.poison_masked(qkv, B, T, H, lens)
    assert torch.isfinite(bad.float()).all()
    clean = R.attention_ref(qkv, B, T, H, 0.125, lens)
    masked = R.attention_ref(bad, B, T, H, 0.125, lens)
    leaky = R.attention_ref(bad, B, T, H, 0.125, None)
    for b, n in enumerate(lens):
        scale = clean[b, :n].abs().max().item()
        assert (masked[b, :n] - clean[b, :n]).abs().max().item() <= 1e-12 * scale
        if n < T:
            assert (leaky[b, :n] - clean[b, :n]).abs().max().item() > 0.1 * scale, "the poison must be loud"
    D = H * 64
    assert torch.equal(bad.view(B, T, 3 * D)[0], qkv.view(B, T, 3 * D)[0]), "a full-length sequence is left alone"
    assert torch.equal(bad[:, :D], qkv[:, :D]), "queries are never touched"


@pytest.mark.parametrize("dtype,lo,hi", [("f16", 5e-5, 8e-4), ("bf16", 4e-4, 6e-3)])
def test_rounding_model_sits_below_the_project_bounds(dtype, lo, hi):
    """The 16-bit P costs what the format's unit roundoff says (2^-11 / 2^-8 per term, averaged down by the sum): the model's error
    is a real, non-zero figure well inside the bounds the GPU tests hold the kernels to."""
    B, T, H = 2, 150, 2
    qkv = _case(B, T, H, 5, R.T16[dtype])
    e = R.attention_rounding_model(qkv, B, T, H, 0.125, dtype=dtype)
    assert lo < e < hi / 1.5, e
    e_out = R.attention_rounding_model(qkv, B, T, H, 0.125, [150, 40], dtype=dtype, round_out=True)
    assert e_out > e / 4 and e_out < hi * 1.5, (e, e_out)


def test_negative_score_family_makes_one_leaked_zero_key_fatal():
    """Input family (ii) of the attention sweep: +1.6 on Q, -1.6 on K puts every valid score near -22, so a key row of zeros
    (score 0) that escapes the mask owns the softmax — relative error of order 1 where plain N(0, 1) inputs give 1 / n."""
    B, T, H, n = 1, 128, 1, 111
    x = R.rand((B * T, 3 * 64), 6)
    x[:, :64] += 1.6
    x[:, 64:128] -= 1.6
    qkv = x.half()
    s, _ = R.attention_scores(qkv, B, T, H, 0.125)
    assert -26.0 < s[..., :n].mean().item() < -18.0
    ref = R.attention_ref(qkv, B, T, H, 0.125, [n])
    leak = qkv.clone()
    leak[n:, 64:] = 0                                   # masked keys as the single-pass kernels keep them in LDS: zero rows
    got = R.attention_ref(leak, B, T, H, 0.125, [n + 1])  # ... and a compare that is off by one
    assert R.seq_rel_err(got, ref, [n]) > 0.9


def test_valid_frame_counts_equal_the_hf_formula():
    kernels, strides = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
    lengths = list(range(400, 2001))
    rows = R.valid_frames_ref(lengths, 2000, kernels, strides)
    n = torch.tensor(lengths)
    for i, (k, s) in enumerate(zip(kernels, strides)):      # HubertModel._get_feat_extract_output_lengths
        n = torch.div(n - k, s, rounding_mode="floor") + 1
        assert rows[i] == n.tolist()
    # clips shorter than the receptive field: zero frames after the stack, conv-0 count kept >= 1, L clamps the input
    rows = R.valid_frames_ref([1, 9, 10, 399, 5000], 2000, kernels, strides)
    assert rows[0] == [1, 1, 1, 78, 399] and rows[-1] == [0, 0, 0, 0, 6]


def test_patchify_refs_equal_unfold_and_conv():
    px = R.rand((2, 3, 12, 18), 7)
    got = R.vit_patchify_ref(px, 6)
    want = F.unfold(px, 6, stride=6).transpose(1, 2).reshape(-1, 108)
    assert got.shape == (12, 112) and torch.equal(got[:, :108], want) and (got[:, 108:] == 0).all()
    vid = R.rand((2, 6, 3, 8, 12), 8).double()
    w = R.rand((5, 3, 3, 4, 4), 9).double()                   # Conv3d weight [O, C, ts, P, P]
    want = F.conv3d(vid.permute(0, 2, 1, 3, 4), w, stride=(3, 4, 4)).permute(0, 2, 3, 4, 1).reshape(-1, 5)
    got = R.video_patchify_ref(vid, 4, 3) @ w.reshape(5, -1).t()
    assert (got - want).abs().max().item() < 1e-12 * want.abs().max().item()


def test_row_refs():
    x = R.rand((5, 3, 8), 10)
    y = R.conv0_gn_gelu_ref(R.rand((2, 100), 11), R.rand((4, 3), 12), 2, torch.ones(4), torch.zeros(4), 1e-5)
    conv = F.conv1d(R.rand((2, 100), 11)[:, None].double(), R.rand((4, 3), 12)[:, None].double(), stride=2)
    assert torch.allclose(y, F.gelu(F.group_norm(conv, 4, eps=1e-5)).transpose(1, 2), rtol=0, atol=1e-12)
    p = R.posconv_pack_ref(x, 2, 4, [3, 1, 2, 3, 3])
    assert p.shape == (5, 2, 7, 4) and (p[:, :, :2] == 0).all() and (p[1, :, 3:] == 0).all()
    assert torch.equal(p[0, 1, 2:5], x[0, :, 4:].double())
    assert torch.equal(R.add_pos_ref(x.view(15, 8), x[0]), x.view(15, 8) + x[0].repeat(5, 1))
    g = R.swiglu_ref(torch.tensor([[-100.0, 30.0, 2.0, -3.0]]), 2)
    assert g[0, 0].item() == pytest.approx(-100.0 / (1 + torch.exp(torch.tensor(100.0, dtype=torch.float64)).item()) * 2.0) and g[0, 1].item() == pytest.approx(-90.0)


# ------------------------------------------------------------------------------------------------------------------ gemm16
GEMM_SHAPES = [(129, 136, 8), (129, 136, 160), (257, 264, 72), (1, 8, 8), (129, 75, 40)]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_gemm16_planes_ref_reproduces_a_true_split(dtype):
    """On a true hi / lo split the 3-pass plane sum is the fp32-grade product: a.w up to the dropped a_lo.w_lo term and the
    rounding of the lo planes — 1e-6 for f16 (2^-22 per operand), U2-grade for bf16 (2^-16 per operand, two operands, averaged
    down by the sum over k: bounded by 4 U2)."""
    M, N, K = 129, 136, 160
    a, w = R.rand((M, K), 21), R.rand((N, K), 22, 0.05)
    ah, al = R.split_planes(a, dtype)
    wh, wl = R.split_planes(w, dtype)
    want = a.double() @ w.double().T
    got = R.gemm16_planes_ref(ah, al, wh, wl, 3)
    e = (got - want).abs().max().item() / want.abs().max().item()
    assert e <= (1e-6 if dtype == "f16" else 4 * R.U2), e
    assert e > 0.0
    for passes, terms in R.GEMM_TERMS.items():                                   # the table in the docstring, term by term
        z = ah.double() @ wh.double().T
        if "hl" in terms:
            z = z + ah.double() @ wl.double().T
        if "lh" in terms:
            z = z + al.double() @ wh.double().T
        assert torch.equal(R.gemm16_planes_ref(ah, al, wh, wl, passes), z)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_indep_planes_discriminate_every_pass_set(dtype, M, N, K):
    """The "indep" family must keep telling the pass sets apart: for every passes value, every OTHER set of lo terms (a dropped or
    an extra pass) and a_lo.w_lo in place of either lo term move the fp64 reference by at least 1000 x the GPU tolerance (max-norm
    relative) — while plain fp32 arithmetic on the same planes stays far inside that tolerance."""
    P = R.indep_planes(M, N, K, dtype, 500 + M + N + K)
    for passes, terms in R.GEMM_TERMS.items():
        ref = R.gemm16_planes_ref(*P, passes)
        scale = ref.abs().max().item()
        wrong = [t for p, t in R.GEMM_TERMS.items() if p != passes]
        wrong += [tuple("ll" if t == x else t for t in terms) for x in terms if x != "hh"]
        for alt in wrong:
            moved = (R.gemm16_terms_ref(*P, alt) - ref).abs().max().item() / scale
            assert moved >= 1000 * R.GEMM_TOL, (passes, alt, moved)
        f32 = sum({"h": P[0], "l": P[1]}[t[0]].float() @ {"h": P[2], "l": P[3]}[t[1]].float().T for t in terms)
        assert (f32.double() - ref).abs().max().item() / scale <= 1e-6, passes


def test_gemm_epilogue_ref_and_act_model():
    z, bias, res = R.rand((7, 5), 31, 3.0), R.rand((5,), 32), R.rand((7, 5), 33)
    tab = R.rand((3, 8), 34)                                                     # a table wider than N: only its first N columns count
    want = F.gelu(z.double() + bias.double(), approximate="tanh") + res.double()
    assert torch.equal(R.gemm_epilogue_ref(z, bias=bias, act="gelu_tanh", residual=res), want)
    rows = torch.tensor([0, 0, 0, 1, 1, 1, 2])
    assert torch.equal(R.gemm_epilogue_ref(z, table=tab, seg_rows=3, act="relu"), F.relu(z.double() + tab.double()[rows, :5]))
    assert torch.equal(R.gemm_epilogue_ref(z, act="quick_gelu"), z.double() * torch.sigmoid(1.702 * z.double()))
    x = R.rand((4000,), 35, 4.0)
    for act in ("quick_gelu", "gelu_tanh"):
        bound, model = R.act_bound(x, act)
        assert 0.0 < model < 1e-6 and bound == R.GEMM_TOL, (act, model)             # fp32 arithmetic alone is far inside 2e-5
    assert R.act_bound(x, "gelu") == (R.GEMM_TOL, 0.0)


def test_auto_tile_rule_at_its_edges():
    assert [R.auto_tile(2000, n, 1) for n in (8, 64, 65)] == [2, 2, 1]
    assert R.auto_tile(1023, 1280, 1) == 1 and R.auto_tile(1024, 1280, 1) == 3
    assert R.auto_tile(1024, 191, 1) == 1 and R.auto_tile(1024, 192, 1) == 1    # 4 tiles of 256 x 256, N <= 1024: few_narrow
    assert R.auto_tile(1024, 1024, 1) == 1 and R.auto_tile(1024, 1032, 1) == 3  # few_narrow on / off at N = 1024
    assert R.auto_tile(6400, 1024, 1) == 3 and R.auto_tile(6144, 1024, 1) == 1  # 100 / 96 tiles of 256 x 256
    assert R.auto_tile(1024, 191, 4) == 1 and R.auto_tile(1024, 192, 4) == 3    # passes 4 is never few_narrow: the N >= 192 edge
