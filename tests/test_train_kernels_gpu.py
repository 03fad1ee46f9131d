"""The fp32 training kernels at their dispatch edges (csrc/gemm32.hip, csrc/fusion.hip, csrc/fusion_topn_group.hip), each against a
plain fp64 reference of the same operation (tests/op_refs.py; the references and the bounds are pinned on the CPU in
tests/test_op_refs_cpu.py).  Every case prints its observed error; u = 2^-24 throughout.

mer_gemm32.  The dispatch conditions, restated: four kernels by (trans_a, trans_w); an operand stored with k contiguous (A without
trans_a, W without trans_w) is read with one 16-byte load per lane and 16-deep k step when ld % 4 == 0, the base pointer is 16-byte
aligned and K % 16 == 0, otherwise (and always for a transposed operand) element by element with k and row guards.  The cases are the
product of those conditions, not workload shapes: operands sit inside NaN-filled buffers (ld > width, rows after the last), outputs
inside canary buffers (ldc > N, rows after M - 1).
  Bound (derived, R.gemm32_bound): with S = |a| |w|^T + |bias|, |out - fp64| <= (2K + 3) u S elementwise: every product is rounded at
  most once and enters at most K additions whatever their order (K u + K u to first order; no assumption on whether the MFMA fuses
  its multiply-add), the bias add is one rounding, 2 u remain for the second-order terms; accumulate = 1 rounds the stored sum once
  more (+ u |out|).  ReLU is 1-Lipschitz and exact: the same bound.  GELU (Whisper's fc1): the pre-activation bound passes through
  |gelu'| <= 1.13 and the activation's own error is R.act_bound's (the project's 2e-5 of max|ref|, as in test_gemm_matrix_gpu.py).
  Bit identity: both loaders hand the same values to the same MFMA sequence, so the four transposition forms (fed transposed copies)
  and the aligned / offset-by-one / odd-ld placements of one logical (A, W, bias) are torch.equal.

fusion.hip element-wise and reduction kernels.  colsum: (M + 1) u sum|x| per column (M in-order additions).  relu_bwd / dropout: exact.
fuse_fwd: (E + 1) u sum_e |h att| around the fp64 sum (E fused steps in stream order); dh exact (one fp32 product); datt: (H + 7) u
sum_j |dout h| (ceil(H / 64) fused steps per lane, a 6-level shuffle tree).  ce_loss / mse_loss / adam: R.ce_bounds, R.MSE_ROW_REL,
R.adam_bounds state their derivations (counted roundings, the cancellation in 1 - b^t); nothing here is tuned to an observed error.

LSTM, small attention and the group engine go through expf / tanhf (or compose everything), so their tolerances are measured, not
derived: max-norm relative error against the fp64 reference, 4 x the worst value over the matrix, never above the project's present
bounds (2e-5 for h_T, 2e-4 for the LSTM gradients, 2e-6 for small attention, 5e-5 / 1e-4 for the group engine).  Measured on the
MI355X (worst over the matrix -> tolerance):
  lstm h_T                                7.93e-7 -> 3.2e-6
  lstm gradients (more than one element)  2.33e-6 -> 9.3e-6
  lstm dX at B = T = D = 1                5.08e-5 -> 2e-4 (the cap): ONE number, a 4H-term sum that cancels (H = 80)
  small_attention, score scale 1          7.01e-7 -> 2e-6 (the cap; 4 x would be 2.8e-6)
  small_attention, scale 30, grid inputs  2.16e-7 -> 2e-6
  group engine, the ten cases B <= 33     loss 7.23e-6 -> 2.9e-5, out 9.36e-6 -> 3.7e-5, grad 9.45e-7 -> 3.8e-6, param / moments 2.59e-5 -> 1e-4 (the cap)
  group engine, B = 2048                  loss 1.23e-6 -> 4.9e-6, out 5.38e-7 -> 2.2e-6, grad 1.09e-6 -> 4.4e-6, param / moments 2.21e-6 -> 8.8e-6
small_attention at score scale 30 with CONTINUOUS q and k measures 2.5e-6 .. 4.5e-6 (Tk = 256, 257, 2047, causal T = 5): the fp32
dot product's own rounding, which the exponential turns into that relative error of the weights whatever the kernel does.  The
scale-30 cases of the matrix therefore draw q and k on a grid of 1/8 (every partial sum of q . k is then exact in fp32: below
2^24 / 64), which keeps what they are for — a softmax over scores of +-100 stays finite and accurate because the maximum is
subtracted — inside the 2e-6 bound; test_small_attention_large_scores_continuous runs ordinary inputs at that scale against
R.small_attention_bound, derived from the fused chain's running sums on those inputs.
"""
import ctypes

import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu
U = R.U32
NAN = float("nan")
MER_EINVAL, MER_ESHAPE, MER_EUNSUPPORTED = -1, -2, -5

# the tolerances of the module docstring
LSTM_H_TOL, LSTM_G_TOL, LSTM_G1_TOL, SATT_TOL = 3.2e-6, 9.3e-6, 2e-4, 2e-6


def _ops():
    from mertools_amd import ops
    return ops


def _lib():
    from mertools_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == 0, f"{what}: rc {rc} {_lib().mer_last_error()}"


class _Win:
    """rows x cols fp32 window at row stride ld inside a larger flat device buffer: `off` floats in front (the allocation is 256-byte
    aligned, so off = 1 gives a base that is not 16-byte aligned), `extra` rows after the last; everything outside the window holds
    `fill` (NaN for operands, the fp32 canary for outputs)."""

    def __init__(self, dev, rows, cols, ld, off=0, extra=2, fill=NAN, data=None):
        assert ld >= cols
        self.buf = torch.full((off + (rows + extra) * ld + 8,), fill, dtype=torch.float32, device=dev)
        self.view = torch.as_strided(self.buf, (rows, cols), (ld, 1), off)
        self.mask = torch.zeros_like(self.buf, dtype=torch.bool)
        torch.as_strided(self.mask, (rows, cols), (ld, 1), off).fill_(True)
        self.fill = fill
        if data is not None:
            self.view.copy_(data)
        assert self.view.data_ptr() % 16 == (4 * off) % 16

    def untouched_outside(self):
        return R.is_canary32(self.buf[~self.mask])


def _ld(cols, kind):
    """aligned: ld % 4 == 0 and > cols; odd: ld = cols + 1 unless that is a multiple of 4 (then cols + 2)."""
    if kind == "odd":
        return cols + 1 if (cols + 1) % 4 else cols + 2
    return (cols + 3) // 4 * 4 + 4


def _gemm_case(dev, M, N, K, ta, tw, seed, pa="aligned", pw="aligned", bias=True, act=None, acc=False, keep=None):
    """One mer_gemm32 launch on logical A [M, K], W [N, K] (stored transposed where asked) in the given placements; returns
    (worst error / bound, output) after asserting the bound, finiteness and the canaries."""
    ops = _ops()
    A, W, b = R.rand((M, K), seed), R.rand((N, K), seed + 1, 0.3), R.rand((N,), seed + 2)
    if keep is not None:
        A, W, b = keep
    a_st, w_st = (A.T.contiguous() if ta else A), (W.T.contiguous() if tw else W)
    wa = _Win(dev, *a_st.shape, _ld(a_st.shape[1], "odd" if pa == "odd" else "aligned"), off=1 if pa == "off1" else 0, data=a_st)
    ww = _Win(dev, *w_st.shape, _ld(w_st.shape[1], "odd" if pw == "odd" else "aligned"), off=1 if pw == "off1" else 0, data=w_st)
    out = _Win(dev, M, N, N + 3, fill=R.CANARY32)
    base = None
    if acc:
        base = R.rand((M, N), seed + 3, 2.0)
        out.view.copy_(base)
    bd = b.to(dev) if bias else None
    ops.gemm32(wa.view, ww.view, bd, act, trans_a=ta, trans_w=tw, out=out.view, accumulate=acc)
    torch.cuda.synchronize()
    what = f"gemm32 M={M} N={N} K={K} ta={int(ta)} tw={int(tw)} A:{pa} W:{pw} bias={int(bias)} act={act} acc={int(acc)}"
    got = out.view.cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output (padding read?)"
    assert out.untouched_outside(), f"{what}: wrote outside the [M, N] window"
    z, S = R.gemm32_pre(a_st, w_st, b if bias else None, ta, tw)
    ref = R.gemm32_ref(a_st, w_st, b if bias else None, act, ta, tw, base)
    bound = R.gemm32_bound(S, K, got if acc else None)
    if act == "gelu":
        rel, _ = R.act_bound(z, act, base)
        bound = R.GELU_LIP * bound + rel * ref.abs().max()
    ratio = R.worst_ratio(got, ref, bound)
    assert ratio <= 1.0, f"{what}: |out - fp64| = {ratio:.3f} x the derived bound"
    return ratio, got


GEMM_MN = ((1, 1), (15, 17), (16, 16), (17, 15), (33, 1), (1, 33), (33, 33))
GEMM_K = (1, 3, 4, 5, 15, 16, 17, 32, 49)
FORMS = ((False, False), (False, True), (True, False), (True, True))


@pytest.mark.parametrize("ta,tw", FORMS, ids=["nn", "nt_dX", "tn", "tt_dW"])
def test_gemm32_shape_matrix(dev, ta, tw):
    """Every (M, N) of GEMM_MN (each of 1, 15, 16, 17, 33 on either side: one lane, a ragged tile, an exact tile, two tiles, three)
    at every K (below / at / past the 4-wide lane group and the 16-deep step), aligned placements, bias + ReLU."""
    worst = 0.0
    for i, (M, N) in enumerate(GEMM_MN):
        for K in GEMM_K:
            r, _ = _gemm_case(dev, M, N, K, ta, tw, 1000 + 37 * i + K, act="relu")
            worst = max(worst, r)
    print(f"gemm32 ta={int(ta)} tw={int(tw)}: {len(GEMM_MN) * len(GEMM_K)} shapes, worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("ta,tw", FORMS[:3], ids=["nn", "nt_dX", "tn"])
def test_gemm32_loader_conditions(dev, ta, tw):
    """The forms with a k-contiguous operand: every condition that turns the 16-byte loader off, separately for A and for W — K % 16
    != 0 (K = 17, 49), ld % 4 != 0 (ld = K + 1), a base one float past a 16-byte boundary — next to the all-aligned case (K = 16, 32),
    at a ragged (17, 33) and an exact (16, 16) tile grid."""
    pa_set = ("aligned", "odd", "off1") if not ta else ("aligned",)
    pw_set = ("aligned", "odd", "off1") if not tw else ("aligned",)
    for M, N in ((17, 33), (16, 16)):
        for K in (16, 32, 17, 49):
            for pa in pa_set:
                for pw in pw_set:
                    r, _ = _gemm_case(dev, M, N, K, ta, tw, 2000 + K, pa=pa, pw=pw)
                    print(f"gemm32 loaders ta={int(ta)} tw={int(tw)} ({M}, {N}, {K}) A:{pa} W:{pw}: |err| / bound {r:.3f}")


@pytest.mark.parametrize("ta,tw", [FORMS[0], FORMS[3]], ids=["nn", "tt_dW"])
def test_gemm32_epilogue(dev, ta, tw):
    """bias present / absent x the activations callers of ops.gemm32 pass (None, "relu": fusion_ops; "gelu": whisper fc1) x accumulate
    0 / 1 (onto a non-zero out), on a ragged shape with the scalar loaders and an exact one with the vector loaders."""
    for M, N, K in ((17, 33, 49), (16, 16, 16)):
        for bias in (True, False):
            for act in (None, "relu", "gelu"):
                for acc in (False, True):
                    r, _ = _gemm_case(dev, M, N, K, ta, tw, 3000 + K, bias=bias, act=act, acc=acc)
                    print(f"gemm32 epilogue ta={int(ta)} tw={int(tw)} ({M}, {N}, {K}) bias={int(bias)} act={act} acc={int(acc)}: |err| / bound {r:.3f}")


@pytest.mark.parametrize("M,N,K", [(33, 17, 32), (16, 16, 16), (17, 33, 49)])
def test_gemm32_bit_identity_across_forms_and_placements(dev, M, N, K):
    """One logical (A, W, bias): the four transposition forms and every placement of the operands give torch.equal outputs (at K = 49
    every launch is on the scalar loaders: the forms alone are compared)."""
    keep = (R.rand((M, K), 4000 + K), R.rand((N, K), 4001 + K, 0.3), R.rand((N,), 4002 + K))
    outs = {}
    for ta, tw in FORMS:
        for pa in (("aligned", "odd", "off1") if not ta else ("aligned",)):
            for pw in (("aligned", "odd", "off1") if not tw else ("aligned",)):
                outs[(ta, tw, pa, pw)] = _gemm_case(dev, M, N, K, ta, tw, 0, pa=pa, pw=pw, keep=keep)[1]
    first = outs[(False, False, "aligned", "aligned")]
    diff = [k for k, o in outs.items() if not torch.equal(o, first)]
    print(f"gemm32 bit identity ({M}, {N}, {K}): {len(outs)} launches, {len(diff)} differ")
    assert not diff, f"outputs differ from the aligned nn launch: {diff}"


# ---------------------------------------------------------------------------------------- fusion.hip: element-wise and reductions
@pytest.mark.parametrize("M", [1, 2, 33])
def test_colsum(dev, M):
    lib = _lib()
    for N in (1, 63, 64, 65, 130):
        x = R.rand((M, N), 5000 + N + M)
        w = _Win(dev, M, N, N + 3, data=x)
        for acc in (0, 1):
            out = _Win(dev, 1, N, N + 2, fill=R.CANARY32)
            base = R.rand((N,), 5100 + N, 3.0) if acc else None
            if acc:
                out.view.copy_(base[None])
            _ok(lib.mer_colsum(_p(w.view), M, N, w.view.stride(0), _p(out.view), acc, _st()), "mer_colsum")
            torch.cuda.synchronize()
            got = out.view.cpu()[0]
            assert torch.isfinite(got).all() and out.untouched_outside(), f"colsum M={M} N={N} acc={acc}"
            r = R.worst_ratio(got, R.colsum_ref(x, base), R.colsum_bound(x, base, got))
            print(f"colsum M={M} N={N} acc={acc}: |err| / bound {r:.3f}")
            assert r <= 1.0
    if M == 33:      # the wrapper (accumulate = 0, contiguous)
        from mertools_amd import fusion_ops
        x = R.rand((M, 130), 5200)
        got = fusion_ops.colsum(x.to(dev)).cpu()
        assert R.worst_ratio(got, R.colsum_ref(x), R.colsum_bound(x)) <= 1.0


SPECIALS = torch.tensor([0.0, -0.0, 1.401298464324817e-45, -1.401298464324817e-45, 1.0, -1.0])
ELEMWISE_N = (1, 255, 256, 257, 4096 * 256 + 5)


def _with_specials(x, shift=0):
    n = x.numel()
    for i in range(min(n, SPECIALS.numel())):
        x[(i + shift) % n] = SPECIALS[(i + shift) % SPECIALS.numel()]
    return x


@pytest.mark.parametrize("n", ELEMWISE_N)
def test_relu_bwd_exact(dev, n):
    """dz = y > 0 ? dy : 0, bit for bit; y holds +0, -0 and the smallest subnormals of either sign (a positive subnormal IS > 0);
    the last n takes the grid-stride loop (more than 4096 blocks of 256)."""
    from mertools_amd import fusion_ops
    dy, y = R.rand((n,), 6000), _with_specials(R.rand((n,), 6001), shift=n % 3)
    got = fusion_ops.relu_bwd(dy.to(dev), y.to(dev)).cpu()
    want = torch.where(y > 0, dy, torch.zeros_like(dy))
    print(f"relu_bwd n={n}: {int((got != want).sum())} elements differ")
    assert torch.equal(got, want)


@pytest.mark.parametrize("n", ELEMWISE_N)
def test_dropout_exact(dev, n):
    """out = keep ? x * scale : 0 with the fp32 scale the ABI receives, bit for bit (one fp32 product)."""
    lib = _lib()
    x = _with_specials(R.rand((n,), 6100), shift=n % 3)
    keep = (torch.rand(n, generator=torch.Generator().manual_seed(6101)) >= 0.3).to(torch.uint8)
    scale = ctypes.c_float(1.0 / (1.0 - 0.3)).value
    xd, kd = x.to(dev), keep.to(dev)
    out = torch.full((n + 4,), R.CANARY32, device=dev)
    _ok(lib.mer_dropout(_p(xd), _p(kd), scale, _p(out), n, _st()), "mer_dropout")
    torch.cuda.synchronize()
    want = torch.where(keep.bool(), x * torch.tensor(scale, dtype=torch.float32), torch.zeros_like(x))
    got = out[:n].cpu()
    print(f"dropout n={n}: {int((got != want).sum())} elements differ")
    assert torch.equal(got, want) and R.is_canary32(out[n:])


def _fuse_check(dev, B, H, E, seed, backward=True):
    from mertools_amd.fusion_ops import FuseFn
    h, att, dout = R.rand((B, E * H), seed), R.rand((B, E), seed + 1), R.rand((B, H), seed + 2)
    hd, ad = h.to(dev).requires_grad_(True), att.to(dev).requires_grad_(True)
    out = FuseFn.apply(hd, ad)
    if backward:
        out.backward(dout.to(dev))
    torch.cuda.synchronize()
    ref, mag = R.fuse_fwd_ref(h, att)
    got = out.detach().cpu()
    assert torch.isfinite(got).all(), f"fuse_fwd B={B} H={H} E={E}: non-finite (rows never written?)"
    rf = R.worst_ratio(got, ref, (E + 1) * U * mag)
    rows_bad = ((got.double() - ref).abs() > (E + 1) * U * mag).any(1).nonzero().flatten()
    assert rf <= 1.0, f"fuse_fwd B={B} H={H} E={E}: {rf:.3g} x bound; {rows_bad.numel()} bad rows, first {rows_bad[:3].tolist()}"
    if not backward:
        return rf, 0.0
    dh_ref, datt_ref, dmag = R.fuse_bwd_ref(dout, h, att)
    assert torch.equal(hd.grad.cpu(), dh_ref), f"fuse_bwd dh B={B} H={H} E={E}: not the fp32 product"
    rd = R.worst_ratio(ad.grad.cpu(), datt_ref, (H + 7) * U * dmag)
    assert rd <= 1.0, f"fuse_bwd datt B={B} H={H} E={E}: {rd:.3g} x bound"
    return rf, rd


@pytest.mark.parametrize("H", [1, 63, 64, 65, 130])
def test_fuse_fwd_bwd(dev, H):
    for E in (1, 3, 18):
        for B in (1, 5):
            rf, rd = _fuse_check(dev, B, H, E, 7000 + 31 * H + E)
            print(f"fuse B={B} H={H} E={E}: fwd |err| / bound {rf:.3f}, dh exact, datt |err| / bound {rd:.3f}")


def test_fuse_fwd_past_the_capped_grid(dev):
    """Regression: mer_fuse_fwd's grid is capped at 4096 blocks of 256 threads; B * H = 4097 * 256 = 1 048 832 outputs need the
    grid-stride loop (the kernel once computed one element per thread and left row 4096 unwritten while reporting success).  Every
    row is checked, the last one by name."""
    B, H, E = 4097, 256, 3
    lib = _lib()
    h, att = R.rand((B, E * H), 7900), R.rand((B, E), 7901)
    out = torch.full((B * H + 4,), R.CANARY32, device=dev)
    hd, ad = h.to(dev), att.to(dev)
    _ok(lib.mer_fuse_fwd(_p(hd), _p(ad), _p(out), B, H, E, _st()), "mer_fuse_fwd")
    torch.cuda.synchronize()
    got = out[:B * H].view(B, H).cpu()
    ref, mag = R.fuse_fwd_ref(h, att)
    bad = ((got.double() - ref).abs() > (E + 1) * U * mag).any(1).nonzero().flatten()
    print(f"fuse_fwd B={B} H={H} E={E}: {bad.numel()} rows outside the bound; |err| / bound over all rows {R.worst_ratio(got, ref, (E + 1) * U * mag):.3g}")
    assert not R.is_canary32(got[4096]), "row 4096 (elements past 1 048 576) was never written"
    assert bad.numel() == 0, f"rows outside the bound: {bad[:5].tolist()}"
    assert R.is_canary32(out[B * H:])
    _fuse_check(dev, B, H, E, 7900)      # and through FuseFn, backward included


def _logits(B, C, scale, seed):
    x = R.rand((B, C), seed)
    if scale == "equal":
        return torch.full((B, C), 3.25)
    if scale in ("pm80", "pm100"):      # rows offset alternately by + / - the constant, the third row mixes both signs by element
        off = float(scale[2:])
        sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)[:, None].expand(B, C).clone()
        if B > 2:
            sign[2] = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
        return x + off * sign
    return x


@pytest.mark.parametrize("C", [1, 2, 6, 63, 64, 65, 130])
def test_ce_loss_and_bwd(dev, C):
    """probs, per-row losses, the mean and dlogits (gout = 0.37) against fp64 within R.ce_bounds, at logits ~ N(0, 1), all equal, and
    offset by +-80 (and +-100: exp overflows fp32 there unless the row maximum is subtracted); targets at class 0 and C - 1."""
    from mertools_amd.fusion_ops import CELossFn
    lib = _lib()
    for B in (1, 7):
        for scale in ("n01", "equal", "pm80", "pm100"):
            x = _logits(B, C, scale, 8000 + C + B)
            tgt = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(8100 + C))
            tgt[0] = C - 1
            if B > 1:
                tgt[1] = 0
            xd, td = x.to(dev), tgt.to(dev)
            probs, rows, dl = (torch.full(s, R.CANARY32, device=dev) for s in ((B * C + 4,), (B + 4,), (B * C + 4,)))
            loss = torch.zeros((), device=dev)
            gout = torch.tensor(0.37, device=dev)
            _ok(lib.mer_ce_loss(_p(xd), _p(td), B, C, _p(probs), _p(rows), _p(loss), _st()), "mer_ce_loss")
            _ok(lib.mer_ce_loss_bwd(_p(probs), _p(td), _p(gout), _p(dl), B, C, _st()), "mer_ce_loss_bwd")
            torch.cuda.synchronize()
            assert all(R.is_canary32(t[n:]) for t, n in ((probs, B * C), (rows, B), (dl, B * C)))
            p_ref, r_ref, l_ref, d_ref = R.ce_ref(x, tgt, 0.37)
            bp, br, bd = R.ce_bounds(x, tgt, 0.37)
            pg, rg, dg = probs[:B * C].view(B, C).cpu(), rows[:B].cpu(), dl[:B * C].view(B, C).cpu()
            assert torch.isfinite(pg).all() and torch.isfinite(rg).all() and torch.isfinite(dg).all(), f"ce C={C} B={B} {scale}: non-finite"
            rp, rr, rd = R.worst_ratio(pg, p_ref, bp), R.worst_ratio(rg, r_ref, br), R.worst_ratio(dg, d_ref, bd)
            # the mean: in row order in fp32 — against the fp64 mean of the kernel's own rows, and against the reference's
            lg = loss.item()
            rm = abs(lg - rg.double().sum().item() / B) / max(R.mean_rows_bound(rg), 1e-300) if rg.abs().sum() > 0 else float(lg != 0)
            rl = abs(lg - l_ref.item()) / max(br.sum().item() / B + R.mean_rows_bound(r_ref), 1e-300)
            print(f"ce C={C} B={B} {scale}: |err| / bound probs {rp:.3f} rows {rr:.3f} mean(own rows) {rm:.3f} loss {rl:.3f} dlogits {rd:.3f}")
            assert max(rp, rr, rm, rl, rd) <= 1.0, f"ce C={C} B={B} {scale}"
            # the autograd front end runs the same two entry points
            xa = xd.clone().requires_grad_(True)
            la = CELossFn.apply(xa, td)
            (la * 0.37).backward()
            torch.cuda.synchronize()
            assert torch.equal(la.detach(), loss) and torch.equal(xa.grad.cpu(), dg)


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_mse_loss_and_bwd(dev, B):
    """rows = (pred - target)^2 within three roundings, the mean in row order, dpred = gout 2 (pred - target) / B within five."""
    lib = _lib()
    pred, tgt = R.rand((B,), 8500 + B, 3.0), R.rand((B,), 8501 + B, 3.0)
    if B > 2:
        tgt[2] = pred[2]                          # an exact zero row
    pd, td = pred.to(dev), tgt.to(dev)
    rows, dp = torch.full((B + 4,), R.CANARY32, device=dev), torch.full((B + 4,), R.CANARY32, device=dev)
    loss, gout = torch.zeros((), device=dev), torch.tensor(0.37, device=dev)
    _ok(lib.mer_mse_loss(_p(pd), _p(td), B, _p(rows), _p(loss), _st()), "mer_mse_loss")
    _ok(lib.mer_mse_loss_bwd(_p(pd), _p(td), _p(gout), _p(dp), B, _st()), "mer_mse_loss_bwd")
    torch.cuda.synchronize()
    assert R.is_canary32(rows[B:]) and R.is_canary32(dp[B:])
    r_ref, l_ref, d_ref = R.mse_ref(pred, tgt, 0.37)
    rg, dg, lg = rows[:B].cpu(), dp[:B].cpu(), loss.item()
    rr = R.worst_ratio(rg, r_ref, R.MSE_ROW_REL * r_ref)
    rl = abs(lg - l_ref.item()) / (R.MSE_ROW_REL * r_ref.sum().item() / B + R.mean_rows_bound(r_ref))
    rd = R.worst_ratio(dg, d_ref, R.MSE_BWD_REL * d_ref.abs())
    print(f"mse B={B}: |err| / bound rows {rr:.3f} loss {rl:.3f} dpred {rd:.3f}")
    assert max(rr, rl, rd) <= 1.0
    from mertools_amd.fusion_ops import MSELossFn
    pa = pd.clone().requires_grad_(True)
    la = MSELossFn.apply(pa, td)
    (la * 0.37).backward()
    torch.cuda.synchronize()
    assert torch.equal(la.detach(), loss) and torch.equal(pa.grad.cpu(), dg)


ADAM_HYP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_BIG = ((1, -1.0, 0.0), (2, 0.05, 1e-2), (10, -1.0, 1e-2), (1000, 0.05, 0.0))       # (step, clip, wd): every value once at the large n


def _adam_combos(n):
    if n > 100000:
        return ADAM_BIG
    return tuple((s, c, w) for s in (1, 2, 10, 1000) for c in (-1.0, 0.05) for w in (0.0, 1e-2))


@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 5])
def test_adam_step_and_adam_step_dev(dev, n):
    """Both Adam entry points against R.adam_ref (fp64 on the fp32-rounded hyper-parameters) within R.adam_bounds, per element, for p, m
    and v.  mer_adam_step_dev reads step - 1 from device memory and must leave it alone; mer_inc_i32 adds exactly one.  The two entry
    points are not required to agree bit for bit (one forms 1 - b^t on the host, the other on the device)."""
    lib = _lib()
    p, g, m, v = R.adam_inputs(n, 9000 + n)
    for step, clip, wd in _adam_combos(n):
        p1, m1, v1, aux = R.adam_ref(p, g, m, v, wd=wd, step=step, clip=clip, **ADAM_HYP)
        bp, bm, bv = R.adam_bounds(p1, aux)
        for entry in ("host", "dev"):
            t = [torch.cat([x, torch.full((4,), R.CANARY32)]).to(dev) for x in (p, m, v)]
            gd = g.to(dev)
            args = (_p(t[0]), _p(gd), _p(t[1]), _p(t[2]), n, ADAM_HYP["lr"], ADAM_HYP["b1"], ADAM_HYP["b2"], ADAM_HYP["eps"], wd)
            if entry == "host":
                _ok(lib.mer_adam_step(*args, step, clip, _st()), "mer_adam_step")
            else:
                ctr = torch.tensor([step - 1, 77], dtype=torch.int32, device=dev)
                _ok(lib.mer_adam_step_dev(*args, _p(ctr), clip, _st()), "mer_adam_step_dev")
                torch.cuda.synchronize()
                assert ctr.tolist() == [step - 1, 77], "mer_adam_step_dev moved the step counter"
                _ok(lib.mer_inc_i32(_p(ctr), _st()), "mer_inc_i32")
                torch.cuda.synchronize()
                assert ctr.tolist() == [step, 77], "mer_inc_i32 must add exactly one"
            torch.cuda.synchronize()
            assert all(R.is_canary32(x[n:]) for x in t)
            pg, mg, vg = (x[:n].cpu() for x in t)
            assert torch.isfinite(pg).all() and torch.isfinite(mg).all() and torch.isfinite(vg).all()
            rp, rm, rv = R.worst_ratio(pg, p1, bp), R.worst_ratio(mg, m1, bm), R.worst_ratio(vg, v1, bv)
            print(f"adam {entry} n={n} step={step} clip={clip} wd={wd}: |err| / bound p {rp:.3f} m {rm:.3f} v {rv:.3f}")
            assert max(rp, rm, rv) <= 1.0, f"adam {entry} n={n} step={step} clip={clip} wd={wd}"


# ------------------------------------------------------------------------------------------------------------------------ LSTM
@pytest.mark.parametrize("H", [16, 48, 80, 256])
def test_lstm_matrix(dev, H):
    """mer_lstm_fwd / mer_lstm_bwd through fusion_ops.lstm_last against torch.nn.LSTM(...).double() on the CPU: h_T and the gradients of
    x and of the four parameters.  Block sizes 4H = 64, 192, 320 (not powers of two), 1024; T = 1 has no recurrent term and takes the
    cprev = 0 branch alone; front-padded zero rows as func_mapping_feature produces."""
    import torch.nn as nn
    from mertools_amd.fusion_ops import lstm_last
    worst_h = worst_g = 0.0
    for T in (1, 2, 5):
        for B in (1, 3):
            for D in (1, 24):
                torch.manual_seed(100 * H + 10 * T + B + D)
                rnn = nn.LSTM(D, H, num_layers=1, batch_first=True)
                x = torch.randn(B, T, D)
                x[: (B + 1) // 2, : T // 2] = 0.0
                wgt = torch.randn(B, H)
                h_ref, g_ref = R.lstm_ref(x, rnn.state_dict(), wgt)
                rnn = rnn.to(dev)
                xd = x.clone().to(dev).requires_grad_(True)
                h = lstm_last(xd, rnn)
                (h * wgt.to(dev)).sum().backward()
                torch.cuda.synchronize()
                eh = R.max_rel(h, h_ref)
                got = {"x": xd.grad, **{k: getattr(rnn, k).grad for k in g_ref if k != "x"}}
                eg = {k: R.max_rel(got[k], g_ref[k]) for k in g_ref}
                print(f"lstm H={H} T={T} B={B} D={D}: h_T {eh:.2e} " + " ".join(f"d{k} {e:.2e}" for k, e in eg.items()))
                assert all(torch.isfinite(t).all() for t in got.values()) and torch.isfinite(h).all()
                worst_h, worst_g = max(worst_h, eh), max(worst_g, *eg.values())
                assert eh <= LSTM_H_TOL, f"lstm h_T H={H} T={T} B={B} D={D}: {eh:.3e} > {LSTM_H_TOL:.1e}"
                for k, e in eg.items():
                    tol = LSTM_G1_TOL if got[k].numel() == 1 else LSTM_G_TOL
                    assert e <= tol, f"lstm d{k} H={H} T={T} B={B} D={D}: {e:.3e} > {tol:.1e}"
    print(f"lstm H={H}: worst h_T {worst_h:.2e}, worst gradient {worst_g:.2e}")


@pytest.mark.parametrize("H", [8, 24, 272])
def test_lstm_refuses_unsupported_widths(dev, H):
    """4H must be a multiple of the 64-lane wave and H <= 256: MER_ESHAPE from the host check, before any launch, nothing written."""
    lib = _lib()
    B, T = 2, 3
    gx, wt = torch.zeros(B * T * 4 * H, device=dev), torch.zeros(4 * H * H, device=dev)
    outs = [torch.full((B * T * w,), R.CANARY32, device=dev) for w in (4 * H, H, H)]
    rc = lib.mer_lstm_fwd(_p(gx), _p(wt), B, T, H, _p(outs[0]), _p(outs[1]), _p(outs[2]), _st())
    rc2 = lib.mer_lstm_bwd(_p(gx), _p(outs[0]), _p(outs[1]), _p(wt), B, T, H, _p(outs[2]), _st())
    torch.cuda.synchronize()
    assert rc == MER_ESHAPE and rc2 == MER_ESHAPE, (rc, rc2)
    assert all(R.is_canary32(o) for o in outs)


# -------------------------------------------------------------------------------------------------------------- small attention
def _satt_case(dev, B, Tq, Tk, H, causal, scale_mult):
    """K and V are the two column halves of one [B*Tk, 2*H*64] matrix (as Whisper's cross-attention passes them), q sits at ldq >
    H*64 in a NaN-padded buffer, the output at ldo > H*64 in a canaried one; the ABI is called directly for the strides."""
    lib = _lib()
    D = H * 64
    seed = 11000 + 7 * Tk + Tq + H
    q, kv = R.rand((B * Tq, D), seed, scale_mult), R.rand((B * Tk, 2 * D), seed + 1)
    if scale_mult != 1.0:      # q and k on a grid of 1/8 (k within +-4): q . k is exact in fp32, see the module docstring
        q = (q * 8).round() / 8
        kv[:, :D] = ((kv[:, :D] * 8).round() / 8).clamp(-4, 4)
    qw = _Win(dev, B * Tq, D, D + 4, data=q)
    kvd = kv.to(dev)
    out = _Win(dev, B * Tq, D, D + 12, fill=R.CANARY32)
    rc = lib.mer_small_attention(_p(qw.view), qw.view.stride(0), _p(kvd[:, :D]), _p(kvd[:, D:]), kvd.stride(0), B, Tq, Tk, H, 0.125,
                                 int(causal), _p(out.view), out.view.stride(0), _st())
    _ok(rc, "mer_small_attention")
    torch.cuda.synchronize()
    got = out.view.cpu()
    what = f"small_attention B={B} Tq={Tq} Tk={Tk} H={H} causal={int(causal)} |q| x{scale_mult}"
    assert torch.isfinite(got).all() and out.untouched_outside(), what
    e = R.max_rel(got, R.small_attention_ref(q, kv[:, :D], kv[:, D:], B, Tq, Tk, H, 0.125, causal))
    print(f"{what}: {e:.2e}")
    assert e <= SATT_TOL, f"{what}: {e:.3e} > {SATT_TOL:.1e}"
    return e


@pytest.mark.parametrize("Tk", [1, 2, 255, 256, 257, 2047, 2048])
def test_small_attention_matrix(dev, Tk):
    """Tk at the 256-thread trip edges and the 2048 limit, Tq in {1, 3}, (H, B) in {(1, 2), (3, 1)}; scores at scale 1 and at scale 30
    (q 30 x larger: the softmax is near one-hot and stays finite because the maximum is subtracted)."""
    for Tq in (1, 3):
        for H, B in ((1, 2), (3, 1)):
            for mult in (1.0, 30.0):
                _satt_case(dev, B, Tq, Tk, H, False, mult)


@pytest.mark.parametrize("T", [1, 5])
def test_small_attention_causal(dev, T):
    for H, B in ((1, 2), (3, 1)):
        for mult in (1.0, 30.0):
            _satt_case(dev, B, T, T, H, True, mult)


@pytest.mark.parametrize("B,Tq,Tk,H", [(2, 3, 257, 1), (1, 1, 2047, 3)])
def test_small_attention_large_scores_continuous(dev, B, Tq, Tk, H):
    """Ordinary (continuous) q 30 x larger: scores of +-100 whose fp32 dot products round.  Elementwise inside R.small_attention_bound,
    which follows the kernel's fused chain on these inputs; the max-norm figure is printed beside it."""
    ops = _ops()
    D = H * 64
    q, k, v = R.rand((B * Tq, D), 12000 + Tk, 30.0), R.rand((B * Tk, D), 12001 + Tk), R.rand((B * Tk, D), 12002 + Tk)
    got = ops.small_attention(q.to(dev), k.to(dev), v.to(dev), B, Tq, Tk, H, 0.125).cpu()
    torch.cuda.synchronize()
    ref = R.small_attention_ref(q, k, v, B, Tq, Tk, H, 0.125)
    r = R.worst_ratio(got, ref, R.small_attention_bound(q, k, v, B, Tq, Tk, H, 0.125))
    print(f"small_attention continuous scale 30 B={B} Tq={Tq} Tk={Tk} H={H}: |err| / bound {r:.4f}, max-norm rel err {R.max_rel(got, ref):.2e}")
    assert torch.isfinite(got).all() and r <= 1.0


def test_small_attention_refuses_tk_2049(dev):
    lib = _lib()
    q, kv = torch.zeros(1, 64, device=dev), torch.zeros(2049, 128, device=dev)
    out = torch.full((1, 64), R.CANARY32, device=dev)
    rc = lib.mer_small_attention(_p(q), 64, _p(kv[:, :64]), _p(kv[:, 64:]), 128, 1, 1, 2049, 1, 0.125, 0, _p(out), 64, _st())
    torch.cuda.synchronize()
    assert rc == MER_EUNSUPPORTED and R.is_canary32(out), rc


# ------------------------------------------------------------------------------------------- the group engine at its dispatch edges
def _group_models(dev, case, data):
    import argparse
    from mertools_amd.toolkit.models import get_models
    ms = []
    for g in range(3):
        if case["kind"] == "att3":
            a = argparse.Namespace(model="attention", audio_dim=case["D"][0], text_dim=case["D"][1], video_dim=case["D"][2], output_dim1=case["C1"],
                                   output_dim2=case["C2"], dropout=0.0, hidden_dim=case["H"], grad_clip=R.GROUP_CLIP[g], feat_type="utt")
        else:
            a = argparse.Namespace(model="attention_topn", audio_dim=list(case["D"]), output_dim1=case["C1"], output_dim2=case["C2"], dropout=0.0,
                                   hidden_dim=case["H"], grad_clip=R.GROUP_CLIP[g], feat_type="utt")
        m = get_models(a)
        assert [k for k, _ in m.model.named_parameters()] == [k for k, _ in R.group_param_spec(case)]
        m.model.load_state_dict(data["inits"][g])
        ms.append(m.to(dev))
    return ms


@pytest.mark.parametrize("case", R.GROUP_CASES, ids=[c["id"] for c in R.GROUP_CASES])
def test_group_engine_edges(dev, case):
    """One group of G = 3 (different inits, learning rates, weight decays, one model with grad_clip) for two train steps and one eval
    step at the shapes of R.GROUP_CASES — H = 18 (H % 4 != 0: the column slices mh + e*H and every ldw are misaligned), H = 20 (K % 16
    != 0 in every hidden layer), a parameter count that moves the weight base par + g*P + off across alignments with g, C1 = 64, M = 1
    and 18, B = 2048 — against R.group_reference: an fp64 composition of oracle.fusion_ref's pieces, divisors n_g, autograd
    gradients, fp64 Adam on the fp32-rounded hyper-parameters.  Per model: every step's loss, out_emo / out_val below the count,
    flat_grad after step 0, parameters, moments and step counters after both steps, the eval step's outputs; the idle model is
    untouched.  The eval step's logits are also torch.equal to the module's own eval-mode forward through the single-model ops
    (the bitwise contract of test_topn_eval_step, carried to the fallback loaders).  The inits are ordinary order-one weights: in
    every gated layer the gates differ between the rows of a minibatch (asserted on the CPU), so the fused ReLU epilogue and the
    gate[row, col] > 0 store of dX see row-dependent gates at every shape.  Tolerances: R.group_tol (measured, 4 x the worst over the
    cases of the class — B <= 33, B = 2048 — capped at the project's 5e-5 / 1e-4)."""
    from mertools_amd.fusion_group import FusionGroupTrainer
    from mertools_amd.fusion_topn_group import FusionTopnGroupTrainer
    data = R.group_case_data(case)
    ref = R.group_reference(case, data)
    ms = _group_models(dev, case, data)
    B, C2, att3 = case["B"], case["C2"], case["kind"] == "att3"
    kw = dict(lr=R.group_lr(case), weight_decay=list(R.GROUP_WD), grad_clip=list(R.GROUP_CLIP), batch_size=B)
    if att3:
        tr = FusionGroupTrainer(ms, **kw)
        tr.set_tables(*data["feats"], data["emos"], data["vals"])
    else:
        tr = FusionTopnGroupTrainer(ms, **kw)
        tr.set_tables(data["feats"], data["emos"], data["vals"] if C2 else None)
    index, count = data["index"].numpy(), data["count"].numpy()
    got = [dict(losses=[], emo=[], val=[]) for _ in range(3)]
    state = ("flat", "flat_grad", "m", "v", "step")
    before = {x: getattr(tr, x).clone() for x in state}
    for s in range(3):
        loss, emo, val = (x.clone().cpu() for x in tr.run(index[s:s + 1], count[s:s + 1], s < 2))
        torch.cuda.synchronize()
        for g in range(3):
            n = int(count[s, g])
            got[g]["losses"].append(float(loss[0, g]) if n else None)
            got[g]["emo"].append(emo[0, g, :n] if n else None)
            got[g]["val"].append(val[0, g, :n].reshape(n, 1) if (n and C2) else None)
        if s == 0:
            for g in range(3):
                got[g]["grad0"] = tr.flat_grad[g].clone().cpu() if count[0, g] else None
            for x in state:      # model 2 sat idle: nothing of it moved while the others trained
                assert torch.equal(getattr(tr, x)[2], before[x][2]), f"idle model: {x} moved"
                assert x == "step" or not torch.equal(getattr(tr, x)[0], before[x][0]), f"model 0: {x} did not move"
        if s == 2:      # the eval step: state untouched, logits bitwise the single-model ops'
            for x in state:
                assert torch.equal(getattr(tr, x), after_train[x]), f"eval step moved {x}"
            for g in range(3):
                n = int(count[2, g])
                rows = data["index"][2, g, :n].long()
                names = ("audios", "texts", "videos") if att3 else [f"feat{i}" for i in range(len(case["D"]))]
                ms[g].eval()
                with torch.no_grad():
                    _, e, v, _ = ms[g]({k: f[rows].to(dev) for k, f in zip(names, data["feats"])})
                assert torch.equal(emo[0, g, :n], e.cpu()), f"model {g}: eval logits differ from the single-model ops by {(emo[0, g, :n] - e.cpu()).abs().max():.3e}"
                if C2:
                    assert torch.equal(val[0, g, :n].reshape(n, 1), v.cpu()), f"model {g}: eval valence differs from the single-model ops"
        after_train = {x: getattr(tr, x).clone() for x in state}
    for g in range(3):
        got[g].update(flat=tr.flat[g].cpu(), m=tr.m[g].cpu(), v=tr.v[g].cpu())
        assert int(tr.step[g]) == ref[g]["step"], f"model {g}: step counter {int(tr.step[g])}"
        for t in [got[g]["flat"], got[g]["m"], got[g]["v"]] + [x for x in got[g]["emo"] + got[g]["val"] if x is not None]:
            assert torch.isfinite(t).all()
    w, tol = R.group_diff(got, ref), R.group_tol(case)
    print(f"group {case['id']}: max-norm rel err " + " ".join(f"{k} {v:.2e}" for k, v in w.items()))
    for k, v in w.items():
        assert v <= tol[k], f"group {case['id']}: {k} {v:.3e} > {tol[k]:.1e}"
