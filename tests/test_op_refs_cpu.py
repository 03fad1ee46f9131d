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


# ----------------------------------------------------------------------------------------------- fp32 training kernels
GEMM32_K = (1, 3, 4, 5, 15, 16, 17, 32, 49)           # the K set of tests/test_train_kernels_gpu.py


def _gemm32_operands(M, N, K, seed):
    return R.rand((M, K), seed), R.rand((N, K), seed + 1, 0.3), R.rand((N,), seed + 2)


@pytest.mark.parametrize("K", GEMM32_K)
def test_gemm32_ref_forms_and_bound_holds_for_fp32_arithmetic(K):
    """The four stored forms give the same fp64 result as F.linear; torch's own fp32 matmul + bias (some order of fp32 roundings) sits
    inside the derived bound, and so does its accumulate form."""
    M, N = 33, 17
    A, W, b = _gemm32_operands(M, N, K, 100 + K)
    want = F.linear(A.double(), W.double(), b.double())
    for ta in (False, True):
        for tw in (False, True):
            a_st, w_st = (A.T.contiguous() if ta else A), (W.T.contiguous() if tw else W)
            z, S = R.gemm32_pre(a_st, w_st, b, ta, tw)
            assert torch.equal(z, want) or (z - want).abs().max() < 1e-12
            assert torch.equal(R.gemm32_ref(a_st, w_st, b, "relu", ta, tw), F.relu(z))
    out32 = F.linear(A, W, b)
    assert R.worst_ratio(out32, want, R.gemm32_bound(S, K)) <= 1.0
    base = R.rand((M, N), 7, 2.0)
    acc32 = base + out32
    assert R.worst_ratio(acc32, want + base.double(), R.gemm32_bound(S, K, acc32)) <= 1.0
    assert R.worst_ratio(F.relu(out32), F.relu(want), R.gemm32_bound(S, K)) <= 1.0


@pytest.mark.parametrize("K", GEMM32_K)
def test_gemm32_bound_rejects_mutated_references(K):
    """A kernel that drops the last k, drops the last row of W, or reads a transposed operand untransposed misses the bound by at
    least 100 x at every K of the matrix (the last one at every K > 1)."""
    M, N = 33, 17                                      # A is [33, K]: never square for a K of the matrix
    A, W, b = _gemm32_operands(M, N, K, 200 + K)
    z, S = R.gemm32_pre(A, W, b)
    bound = R.gemm32_bound(S, K)
    drop_k = A[:, :K - 1].double() @ W[:, :K - 1].double().T + b.double()
    drop_row = z.clone()
    drop_row[:, N - 1] = b.double()[N - 1]
    untransposed = A.T.contiguous().reshape(M, K).double() @ W.double().T + b.double()       # the [K, M] storage read as [M, K]
    muts = [("last k dropped", drop_k), ("last W row dropped", drop_row), ("transposed A read untransposed", untransposed)]
    if K == 1:      # a [1, M] and an [M, 1] array are the same memory: at K = 1 the third mutation is not a different kernel
        assert torch.equal(untransposed, z)
        muts.pop()
    for name, mut in muts:
        r = R.worst_ratio(mut, z, bound)
        assert r >= 100.0, f"K={K} {name}: only {r:.1f} x the bound"


def test_fusion_kernel_refs():
    """colsum / fuse / CE / MSE references against torch's own operators and autograd in fp64; fp32 restatements of the kernels'
    formulas sit inside the derived bounds."""
    x = R.rand((33, 130), 1)
    assert torch.allclose(R.colsum_ref(x, x[0]), x.double().sum(0) + x[0].double(), rtol=0, atol=1e-12)
    s32 = torch.zeros(130)
    for m in range(33):
        s32 = s32 + x[m]
    assert R.worst_ratio(s32, R.colsum_ref(x), R.colsum_bound(x)) <= 1.0
    B, H, E = 5, 65, 3
    h, att, dout = R.rand((B, E * H), 2), R.rand((B, E), 3), R.rand((B, H), 4)
    hd, ad = h.double().requires_grad_(True), att.double().requires_grad_(True)
    fused = torch.matmul(torch.stack(hd.split(H, 1), dim=2), ad.unsqueeze(2)).squeeze(2)           # attention.py:48-50
    fused.backward(dout.double())
    ref, mag = R.fuse_fwd_ref(h, att)
    assert torch.allclose(ref, fused.detach(), rtol=0, atol=1e-12)
    assert R.worst_ratio(R.fuse_fwd_chain32(h, att), ref, (E + 1) * R.U32 * mag) <= 1.0
    dh, datt, dmag = R.fuse_bwd_ref(dout, h, att)
    assert R.max_rel(dh, hd.grad) < 1e-7 and torch.allclose(datt, ad.grad, rtol=0, atol=1e-12)
    dropped = ref - h[:, (E - 1) * H:].double() * att[:, E - 1:].double()                          # a kernel that stops at E - 1
    assert R.worst_ratio(dropped, ref, (E + 1) * R.U32 * mag) >= 100.0
    # CE
    for C, off in ((1, 0.0), (6, 0.0), (130, 80.0)):
        lg = R.rand((7, C), 5 + C) + off * torch.where(torch.arange(7) % 2 == 0, 1.0, -1.0)[:, None]
        tgt = torch.randint(0, C, (7,), generator=torch.Generator().manual_seed(C))
        lr = lg.double().requires_grad_(True)
        loss = F.cross_entropy(lr, tgt, reduction="sum") / 7
        (0.37 * loss).backward()
        probs, rows, l_ref, d_ref = R.ce_ref(lg, tgt, 0.37)
        assert torch.allclose(probs, torch.softmax(lg.double(), 1), rtol=1e-12, atol=0) and abs(l_ref - loss.item()) < 1e-12
        assert torch.allclose(d_ref, lr.grad, rtol=0, atol=1e-15)
        bp, br, bd = R.ce_bounds(lg, tgt, 0.37)
        mx = lg.max(1, keepdim=True).values                                                         # the kernel's formula in torch fp32
        lse = mx + torch.log(torch.exp(lg - mx).sum(1, keepdim=True))
        p32 = torch.exp(lg - lse)
        r32 = (lse - lg.gather(1, tgt.view(-1, 1))).squeeze(1)
        onehot = torch.zeros_like(lg).scatter_(1, tgt.view(-1, 1), 1.0)
        d32 = torch.tensor(0.37) * (p32 - onehot) / 7.0
        assert R.worst_ratio(p32, probs, bp) <= 1.0 and R.worst_ratio(r32, rows, br) <= 1.0 and R.worst_ratio(d32, d_ref, bd) <= 1.0
        if C > 1:      # probabilities left un-normalised (exp(l - max) without the log of the sum) are far outside the bound
            assert R.worst_ratio(torch.exp(lg.double() - mx.double()), probs, bp) >= 100.0
    # MSE
    pred, tgt = R.rand((257,), 8, 3.0), R.rand((257,), 9, 3.0)
    pr = pred.double().requires_grad_(True)
    loss = F.mse_loss(pr.view(-1, 1), tgt.double().view(-1, 1), reduction="sum") / 257
    (0.37 * loss).backward()
    rows, l_ref, d_ref = R.mse_ref(pred, tgt, 0.37)
    assert abs(l_ref - loss.item()) < 1e-12 and torch.allclose(d_ref, pr.grad, rtol=0, atol=1e-15)
    d = pred - tgt
    assert R.worst_ratio(d * d, rows, R.MSE_ROW_REL * rows) <= 1.0
    assert R.worst_ratio(torch.tensor(0.37) * 2.0 * d / 257.0, d_ref, R.MSE_BWD_REL * d_ref.abs()) <= 1.0


ADAM_CASES = [(s, c, w) for s in (1, 2, 10, 1000) for c in (-1.0, 0.05) for w in (0.0, 1e-2)]
ADAM_HYP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _adam32(p, g, m, v, lr, b1, b2, eps, wd, step, clip):
    """The kernel's formula statement by statement in torch fp32 (csrc/fusion.hip: adam_kernel), corrections formed in fp32."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    bc1 = 1.0 - b1 ** step
    bc2s = torch.sqrt(1.0 - b2 ** step)
    gi = g.clamp(-clip, clip) if clip > 0 else g
    gi = wd * p + gi
    mi = b1 * m + (1.0 - b1) * gi
    vi = b2 * v + (1.0 - b2) * gi * gi
    return p - (lr / bc1) * (mi / (torch.sqrt(vi) / bc2s + eps)), mi, vi


def test_adam_ref_is_torch_adam():
    """R.adam_ref against torch.optim.Adam in fp64 over 12 steps (L2 weight decay, clip_grad_value_ before the step), fed the same
    fp32-rounded hyper-parameters."""
    f = lambda x: float(torch.tensor(x, dtype=torch.float32))
    p0, _, _, _ = R.adam_inputs(300, 1)
    for clip, wd in ((-1.0, 0.0), (0.05, 1e-2)):
        w = p0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=f(1e-3), betas=(f(0.9), f(0.999)), eps=f(1e-8), weight_decay=f(wd))
        p, m, v = p0.double(), torch.zeros(300, dtype=torch.float64), torch.zeros(300, dtype=torch.float64)
        for step in range(1, 13):
            g = R.adam_inputs(300, 10 + step)[1]
            w.grad = g.double().clone()
            if clip > 0:
                torch.nn.utils.clip_grad_value_([w], f(clip))
            opt.step()
            p, m, v, _ = R.adam_ref(p, g, m, v, wd=wd, step=step, clip=clip, **ADAM_HYP)
            assert torch.allclose(p, w.detach(), rtol=1e-12, atol=1e-15), (clip, wd, step)


@pytest.mark.parametrize("step,clip,wd", ADAM_CASES)
def test_adam_bounds_hold_for_fp32_and_reject_mutations(step, clip, wd):
    """The fp32 restatement of the kernel sits inside R.adam_bounds on the GPU test's inputs; a reference that clips after adding the
    weight decay, one with eps inside the square root, and one whose bias corrections use step - 1 (adam_dev reading the counter
    without the + 1) each miss the bound by at least 100 x."""
    p, g, m, v = R.adam_inputs(257, 9000 + 257)
    p1, m1, v1, aux = R.adam_ref(p, g, m, v, wd=wd, step=step, clip=clip, **ADAM_HYP)
    bp, bm, bv = R.adam_bounds(p1, aux)
    p32, m32, v32 = _adam32(p, g, m, v, wd=wd, step=step, clip=clip, **ADAM_HYP)
    assert R.worst_ratio(p32, p1, bp) <= 1.0 and R.worst_ratio(m32, m1, bm) <= 1.0 and R.worst_ratio(v32, v1, bv) <= 1.0
    muts = ["eps_in_sqrt", "step_minus_1"] + (["clip_after_wd"] if clip > 0 and wd > 0 else [])
    for mut in muts:
        if mut == "step_minus_1" and step == 1:
            pm = R.adam_ref(p, g, m, v, wd=wd, step=step, clip=clip, mutate=mut, **ADAM_HYP)[0]
            assert not torch.isfinite(pm).all()            # 1 - b^0 = 0: the update is not even finite
            continue
        pm, mm, vm, _ = R.adam_ref(p, g, m, v, wd=wd, step=step, clip=clip, mutate=mut, **ADAM_HYP)
        r = max(R.worst_ratio(pm, p1, bp), R.worst_ratio(mm, m1, bm), R.worst_ratio(vm, v1, bv))
        assert r >= 100.0, f"{mut} at step {step}, clip {clip}, wd {wd}: only {r:.1f} x the bound"


def test_lstm_and_small_attention_refs():
    import torch.nn as nn
    torch.manual_seed(0)
    rnn = nn.LSTM(24, 16, num_layers=1, batch_first=True)
    x, wgt = torch.randn(3, 5, 24), torch.randn(3, 16)
    h, g = R.lstm_ref(x, rnn.state_dict(), wgt)
    xr = x.clone().requires_grad_(True)
    _, (hn, _) = rnn(xr)
    (hn[0] * wgt).sum().backward()
    assert h.dtype == torch.float64 and R.max_rel(hn[0], h) < 1e-6 and R.max_rel(xr.grad, g["x"]) < 1e-5
    assert all(R.max_rel(getattr(rnn, k).grad, g[k]) < 1e-5 for k in g if k != "x")
    B, Tq, Tk, H = 2, 3, 257, 3
    q, k, v = R.rand((B * Tq, H * 64), 1), R.rand((B * Tk, H * 64), 2), R.rand((B * Tk, H * 64), 3)
    heads = [t.double().view(B, -1, H, 64).transpose(1, 2) for t in (q, k, v)]
    want = F.scaled_dot_product_attention(*heads, scale=0.125).transpose(1, 2).reshape(B * Tq, H * 64)
    assert torch.allclose(R.small_attention_ref(q, k, v, B, Tq, Tk, H, 0.125), want, rtol=1e-12, atol=1e-14)
    qc, kc, vc = q[:B * 3], k[:B * 3], v[:B * 3]
    heads = [t.double().view(B, -1, H, 64).transpose(1, 2) for t in (qc, kc, vc)]
    want = F.scaled_dot_product_attention(*heads, scale=0.125, is_causal=True).transpose(1, 2).reshape(B * 3, H * 64)
    assert torch.allclose(R.small_attention_ref(qc, kc, vc, B, 3, 3, H, 0.125, True), want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("case", R.GROUP_CASES, ids=[c["id"] for c in R.GROUP_CASES])
def test_group_reference_gates_and_sensitivity(case):
    """Per case of the group-engine matrix: (1) no gated pre-activation of the fp64 reference lies within 1e-4 max|z| of zero, in any
    layer, model or step — a ReLU gate taken on fp32 values cannot flip against the reference for rounding alone; (2) the gates depend
    on the row: in every gated layer at least a quarter of the units are open for some rows of a minibatch and shut for others (the
    B = 1 cases have one row per minibatch and are exempt); where biases were nudged (R.group_case_data) they are few: under 0.2 % of
    the pre-activations; (3) a reference that divides by B instead of n_g, one that sums the bias gradients over all B rows, and one
    that drops the last k of the first hidden layer (encoder 0's linear_1) each move the result by at least 10 x the case's tolerance
    (the first two exist only where some n_g < B: not in the B = 1 cases)."""
    data = R.group_case_data(case)
    ref, pres = R.group_reference(case, data, collect_pre=True)
    assert len(pres) == sum(3 * (len(case["D"]) + 1) for g in range(3) for s in range(3) if data["count"][s, g])
    for g, s, name, z in pres:
        assert z.abs().min() >= R.GROUP_MARGIN * z.abs().max(), (g, s, name, z.abs().min().item())
    assert ("seed" in case) == (data["nudged"] == 0) and data["nudged"] <= 2e-3 * sum(z.numel() for *_, z in pres)
    if case["B"] > 1:
        assert R.group_mixed_share(case, pres) >= 0.25
    assert [r["step"] for r in ref] == [2, 2, 1] and ref[2]["grad0"] is None and ref[2]["losses"][0] is None
    tol = R.group_tol(case)
    muts = ["drop_last_k"] + (["div_by_B", "bias_over_B"] if case["B"] > 1 else [])
    for mut in muts:
        w = R.group_diff(R.group_reference(case, data, mutate=mut), ref)
        assert max(w[k] / tol[k] for k in w) >= 10.0, (mut, w)


def test_group_param_spec_is_the_modules_parameter_order():
    """R.group_param_spec against the two modules' own named_parameters() (names, shapes, order = the engine's flat layout)."""
    import argparse
    from mertools_amd.toolkit.models import get_models
    for case in (R.GROUP_CASES[0], R.GROUP_CASES[1], R.GROUP_CASES[9]):
        if case["kind"] == "att3":
            a = argparse.Namespace(model="attention", audio_dim=case["D"][0], text_dim=case["D"][1], video_dim=case["D"][2], output_dim1=case["C1"],
                                   output_dim2=case["C2"], dropout=0.0, hidden_dim=case["H"], grad_clip=-1.0, feat_type="utt")
        else:
            a = argparse.Namespace(model="attention_topn", audio_dim=list(case["D"]), output_dim1=case["C1"], output_dim2=case["C2"], dropout=0.0,
                                   hidden_dim=case["H"], grad_clip=-1.0, feat_type="utt")
        m = get_models(a)
        assert [(k, tuple(p.shape)) for k, p in m.model.named_parameters()] == R.group_param_spec(case)
        m.model.load_state_dict(R.group_case_data(case)["inits"][0])


def test_small_attention_bound_holds_for_fp32_and_is_tight_enough_to_bite():
    """R.small_attention_bound at score scale 30 on continuous inputs: torch's own fp32 attention sits inside it, the bound stays
    below 1e-3 of max|ref|, and a kernel that pairs each weight with the next key's value row is at least 100 x outside (the softmax is near one-hot at this scale: it is insensitive to the score scale itself)."""
    B, Tq, Tk, H = 2, 3, 257, 1
    q, k, v = R.rand((B * Tq, H * 64), 1, 30.0), R.rand((B * Tk, H * 64), 2), R.rand((B * Tk, H * 64), 3)
    ref = R.small_attention_ref(q, k, v, B, Tq, Tk, H, 0.125)
    bound = R.small_attention_bound(q, k, v, B, Tq, Tk, H, 0.125)
    heads = [t.view(B, -1, H, 64).transpose(1, 2) for t in (q, k, v)]
    out32 = F.scaled_dot_product_attention(*heads, scale=0.125).transpose(1, 2).reshape(B * Tq, H * 64)
    assert R.worst_ratio(out32, ref, bound) <= 1.0
    assert bound.max() <= 1e-3 * ref.abs().max()
    assert R.worst_ratio(R.small_attention_ref(q, k, v.roll(1, 0), B, Tq, Tk, H, 0.125), ref, bound) >= 100.0


# --------------------------------------------------------------------------------------------------------------- mer_seq_bias
def _brute_rows(T, valid, rows_left):
    s = max(p for p in (2 ** i for i in range(13)) if p == 1 or 16 * p <= T)
    return [r for r in range(T) if r % s == s // 2 and r < valid and r < rows_left]


def test_seq_sample_rows_against_enumeration():
    """Every T <= 2100, at valid / rows_left on both sides of every sample boundary; no T up to 5000 yields more than 32 samples, and
    32 is first reached at T = 127."""
    for T in range(1, 2101):
        s = R.seq_sample_stride(T)
        h = s // 2
        assert s & (s - 1) == 0 and (s == 1 or 16 * s <= T) and 32 * s > T
        for valid in {0, h, h + 1, h + s, h + s + 1, T - 1, T, T + 5}:
            assert R.seq_sample_rows(T, valid, T) == _brute_rows(T, valid, T), (T, valid)
        for left in {1, h, h + 1, T - 1} - {0}:
            assert R.seq_sample_rows(T, T, left) == _brute_rows(T, T, left), (T, left)
            assert R.seq_sample_rows(T, h + s + 1, left) == _brute_rows(T, h + s + 1, left), (T, left)
    counts = [len(R.seq_sample_rows(T, T, T)) for T in range(1, 5001)]
    assert max(counts) == R.SEQ_MAX_SAMPLES == 32 and counts.index(32) + 1 == 127
    assert all(c >= min(T, 16) for T, c in enumerate(counts, 1))               # "leaves at least 16 samples" (all rows below T = 16)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_round16_direct_is_the_formats_rounding(dtype):
    """On fp32 inputs (no double rounding possible) the hand-written one-step rounding equals torch's cast, subnormals and ties
    included."""
    x = torch.cat([R.seq_grid_values((4096,), 3, "f16").float() * 1.0009765, R.rand((4096,), 4, 100.0),
                   torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 0.0, -2.0 ** -14, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])])
    assert torch.equal(R.round16_direct(x, dtype), x.to(R.T16[dtype]).double())


def _mean_case(dtype, T=70, nseq=3, K=24):
    a = R.seq_grid_values((T * nseq - 9, K), 11, dtype)
    valid = torch.tensor([T, T - 13, T])[:nseq]
    return a, T, valid


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_seq_mean16_ref_plain_statement_and_controls(dtype):
    """The integer model keeps the plain statement (|mean16 - fp64 sample mean| <= 2^-15 + the roundings), and every mutation of the
    sample moves at least one bit of the plane."""
    a, T, valid = _mean_case(dtype)
    good = R.seq_mean16_ref(a, T, valid)
    m64 = R.seq_sample_mean64(a, T, valid)
    assert R.worst_ratio(good, m64, R.seq_mean16_plain_bound(m64, dtype)) <= 1.0
    assert (good.double() != m64).any(), "the grid must matter on these inputs"
    # an independent restatement in exact rational arithmetic
    from fractions import Fraction
    s, h = R.seq_sample_stride(T), R.seq_sample_stride(T) // 2
    rows = list(range(T + h, T + min(int(valid[1]), T), s))
    for k in (0, 7, 23):
        tot = sum(round(Fraction(float(a[r, k])) * 16384) for r in rows)          # round(): ties to even, exact
        want = torch.tensor(float(tot) * (1.0 / (len(rows) * 16384.0)), dtype=torch.float64).float().to(a.dtype)
        assert good[1, k].item() == want.item()
    for mut in ("offset0", "stride2", "drop_last", "no_valid"):
        bad = R.seq_mean16_ref(a, T, valid, mutate=mut)
        assert not torch.equal(bad.view(torch.int16), good.view(torch.int16)), mut
    # no sample: valid = h, and a last sequence with h rows left
    z = R.seq_mean16_ref(a[:2 * T + h], T, torch.tensor([h, T, T]))
    assert not z[0].any() and not z[2].any() and z[1].any()


@pytest.mark.parametrize("dtype,big,odd", [("f16", 1024.0, 2056.0), ("bf16", 128.0, 264.0)])
def test_seq_mean16_ref_rounds_through_fp32(dtype, big, odd):
    """16 samples whose mean is half an ulp of the 16-bit format above `big`, plus 2^-18: fp32 drops the 2^-18, the tie then goes
    to even; one rounding from fp64 goes up.  The model must give the former."""
    col = torch.tensor([big] * 14 + [odd, 2.0 ** -14]).to(R.T16[dtype])
    assert col.double().sum().item() == 16 * (big + 0.5) + 2.0 ** -14
    a = col[:, None].repeat(1, 8)
    good, direct = R.seq_mean16_ref(a, 16), R.seq_mean16_ref(a, 16, mutate="no_f32")
    assert good[0, 0].item() == big and direct[0, 0].item() == big + 1.0           # one ulp of either format at `big` is 1


def test_seq_mean16_ref_clamp_and_nonfinite():
    """bf16 samples of 2^17 and 2^20 count as 131000; +inf as 131000, -inf and NaN as -131000."""
    a = torch.zeros((16, 8), dtype=torch.bfloat16)
    a[:, 0] = 2.0 ** 17
    a[::2, 1] = 2.0 ** 20
    a[3, 2] = float("inf")
    a[3, 3] = float("nan")
    a[3, 4] = float("-inf")
    m = R.seq_mean16_ref(a, 16).double()
    want = torch.tensor([131000.0, 65500.0, 131000.0 / 16, -131000.0 / 16, -131000.0 / 16, 0, 0, 0]).bfloat16().double()
    assert torch.equal(m[0], want)


def _table_case(K, N, nseq, dtype, bias=True):
    mean16 = (R.rand((nseq, K), 21) * 0.7 + 0.3).to(R.T16[dtype])
    w_lo = R.rand((-(-N // 16) * 16, K), 22).to(R.T16[dtype])             # order 1, with the rows a partial block would overread
    return mean16, w_lo, (R.rand((N,), 23) if bias else None)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K,N,n_first", [(8, 17, 0), (40, 40, 32), (544, 16, 0), (2080, 40, 16)])
def test_seq_bias_bound_holds_fp32_and_sees_the_mutations(dtype, K, N, n_first):
    """An honest fp32 evaluation in the kernel's shape stays inside seq_bias_bound; a dropped k-slice, a clamp one column low and an
    n_first one block off are each at least 100 bounds out."""
    mean16, wbuf, bias = _table_case(K, N, 5, dtype)
    w_lo = wbuf[:N]
    ref = R.seq_bias_table_ref(mean16, w_lo, bias, n_first)
    bound = R.seq_bias_bound(mean16, w_lo, bias, n_first)
    assert torch.equal(ref[:, :n_first], bias.double()[None, :n_first].expand(5, -1))
    assert R.worst_ratio(R.seq_bias_model32(mean16, w_lo, bias, n_first), ref, bound) <= 1.0
    for mut in ("drop_kslice", "n_clamp_low", "n_first_block"):
        bad = R.seq_bias_table_ref(mean16, w_lo, bias, n_first, mutate=mut)
        assert R.worst_ratio(bad, ref, bound.clamp_min(1e-30)) >= 100.0, mut


def test_a_missing_n_clamp_is_a_read_not_a_value():
    """Column n of the table depends on row n of w_lo alone, so lanes 16 .. ceil16(N) - 1 of a partial column block, whose columns are
    never written, cannot move a written value whatever they read: without the clamp they read rows N .. of the buffer (NaN here),
    and the N written columns are the reference's, bit for bit.  What the clamp is for is the READ — the GPU test surrounds w_lo with
    NaN rows it does not own — and the value-moving neighbour of that defect is the clamp taken one row low ("n_clamp_low")."""
    mean16, wbuf, bias = _table_case(40, 17, 5, "f16")
    wbuf = wbuf.clone()
    wbuf[17:] = float("nan")
    ref = R.seq_bias_table_ref(mean16, wbuf[:17], bias)
    free = R.seq_bias_table_ref(mean16, wbuf, bias, mutate="no_n_clamp")
    assert free.shape == ref.shape and torch.equal(free, ref)
    low = R.seq_bias_table_ref(mean16, wbuf[:17], bias, mutate="n_clamp_low")
    assert torch.equal(low[:, :16], ref[:, :16])
    assert R.worst_ratio(low, ref, R.seq_bias_bound(mean16, wbuf[:17], bias)) >= 100.0
