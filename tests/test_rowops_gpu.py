"""The row-wise LayerNorm family and the small front-end kernels at their dispatch edges (GPU), against tests/op_refs.py.

RowLN<T, NV> (csrc/norm.hip: pick_nv) holds a row in NV 64-lane vector steps of 4 floats: NV = 2 (D <= 512), 3 (<= 768),
4 (<= 1024), 8 (<= 2048).  LN_D below visits every NV in both plane types with a partial last step (D / 4 no multiple of 64) and
at the full width; the multi-row kernel (NV <= 4) is compared bit for bit with the one-row kernel.

Entry point -> test
  mer_layernorm                 test_layernorm_widths, test_layernorm_multi_row_is_bit_identical, test_layernorm_without_affine,
                                test_layernorm_refuses_2052, test_layernorm_strided_rows
  mer_vit_assemble              test_vit_assemble_wide
  mer_bert_embed                test_bert_embed_wide
  mer_swiglu                    test_swiglu
  mer_token_reduce              test_token_reduce
  mer_add_pos                   test_add_pos_is_bit_exact
  mer_split16                   test_split16_bf16
  mer_sum_pool                  test_sum_pool_empty_and_long_segments
  mer_hubert_conv0_plain        test_hubert_conv0_plain
  mer_hubert_conv0_gn(_ragged)  test_hubert_conv0_gn_two_pass_fallback
  mer_posconv_pack_ragged       test_posconv_pack_ragged
  mer_hubert_valid_frames(_all) test_hubert_valid_frames
  mer_vit_patchify              test_vit_patchify_generic_path
  mer_video_patchify            test_video_patchify

Bounds (max-norm relative error, util.assert_close) are the project's own numbers for the same op in tests/test_ops_gpu.py —
2e-6 for the LayerNorm family in fp32 and as f16 hi + lo planes, 5e-6 for conv0 + GroupNorm + GELU, 1e-6 for the packing
kernels and the segment mean.  Wherever the result is read as bf16 hi + lo planes the bound is the fp32 one + 2^-16: the pair
carries 16 significand bits, so u^2 = 2^-16 is the format's own error, not the kernel's.
"""
import pytest
import torch

import op_refs as R
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu

LN_D = (8, 252, 384, 1028, 1280, 1536, 2044, 2048)     # NV = 2, 2, 2, 8, 8, 8, 8, 8; partial last step at 8, 252, 384, 1028, 1280, 2044
LN_ROWS_D = (8, 252, 384, 700, 1020)                   # multi-row kernel: NV = 2, 2, 2, 3, 4, every one with a partial step
LN_ROWS_M = 33003                                      # as test_layernorm_many_rows: more than 8 rows per resident wave slot


def _ops():
    from mertools_amd import ops
    return ops


def _plane_tol(tol, dtype):
    return tol if dtype == "f16" else tol + R.U2


def _ln_inputs(M, D, seed=12):
    x = R.rand((M, D), seed, 3.0) + 0.5
    return x, R.rand((D,), seed + 1) * 0.1 + 1.0, R.rand((D,), seed + 2) * 0.1


# --------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("act", [None, "gelu"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_widths(dev, D, dtype, act):
    ops = _ops()
    M = 77                                                # the one-row kernel; 77 = 19 workgroups of 4 rows + 1
    x, g, b = _ln_inputs(M, D)
    ref = R.layernorm_ref(x, g, b, 1e-5, act).float()
    o32, oh, ol = ops.layernorm(x.to(dev), g.to(dev), b.to(dev), 1e-5, act=act, out32=True, out16=True, out16_lo=True, dtype=dtype)
    p32, ph, pl = ops.layernorm(x.to(dev), g.to(dev), b.to(dev), 1e-5, act=act, out32=True, out16=True, out16_lo=True, dtype=dtype)
    torch.cuda.synchronize()
    assert torch.equal(o32, p32) and torch.equal(oh, ph) and torch.equal(ol, pl)
    assert_close(o32.cpu(), ref, 2e-6, f"layernorm D={D} act={act} fp32")
    assert_close((oh.float() + ol.float()).cpu(), ref, _plane_tol(2e-6, dtype), f"layernorm D={D} act={act} {dtype} planes")
    assert torch.equal(oh, o32.to(oh.dtype)), "the hi plane is the fp32 result rounded once"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", LN_ROWS_D)
def test_layernorm_multi_row_is_bit_identical(dev, D, dtype):
    """M large enough for layernorm_rows_kernel (gamma / beta through LDS, partial vector step) against fp64 and — the kernel's
    header promises the same arithmetic per row — bit for bit against the one-row kernel on the same rows."""
    ops = _ops()
    M = LN_ROWS_M
    x, g, b = _ln_inputs(M, D)
    xd, gd, bd = x.to(dev), g.to(dev), b.to(dev)
    ref = R.layernorm_ref(x, g, b, 1e-5).float()
    o32, oh, ol = ops.layernorm(xd, gd, bd, 1e-5, out32=True, out16=True, out16_lo=True, dtype=dtype)
    og, _, _ = ops.layernorm(xd, gd, bd, 1e-5, act="gelu")
    head = xd[:1000].contiguous()
    s32, sh, sl = ops.layernorm(head, gd, bd, 1e-5, out32=True, out16=True, out16_lo=True, dtype=dtype)     # small M: the one-row kernel
    sg, _, _ = ops.layernorm(head, gd, bd, 1e-5, act="gelu")
    tail = xd[M - 999:].contiguous()
    t32, _, _ = ops.layernorm(tail, gd, bd, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(o32[:1000], s32) and torch.equal(oh[:1000], sh) and torch.equal(ol[:1000], sl), "multi-row != one-row LayerNorm"
    assert torch.equal(og[:1000], sg), "multi-row != one-row LayerNorm + GELU"
    assert torch.equal(o32[M - 999:], t32), "multi-row != one-row LayerNorm on the last rows"
    assert_close(o32.cpu(), ref, 2e-6, f"layernorm D={D} fp32 (multi-row)")
    assert_close((oh.float() + ol.float()).cpu(), ref, _plane_tol(2e-6, dtype), f"layernorm D={D} {dtype} planes (multi-row)")
    assert_close(og.cpu(), R.act_ref(ref.double(), "gelu").float(), 2e-6, f"layernorm+gelu D={D} (multi-row)")


@pytest.mark.parametrize("M", [77, LN_ROWS_M])
@pytest.mark.parametrize("D", [384, 1280])
def test_layernorm_without_affine(dev, D, M):
    """gamma = beta = NULL: identity scale from registers (one-row kernel) / from the LDS copy's defaults (multi-row, D <= 1024)."""
    ops = _ops()
    x, _, _ = _ln_inputs(M, D)
    o32, _, _ = ops.layernorm(x.to(dev), None, None, 1e-5)
    torch.cuda.synchronize()
    assert_close(o32.cpu(), R.layernorm_ref(x, None, None, 1e-5).float(), 2e-6, f"layernorm D={D} M={M} without gamma / beta")


def test_layernorm_refuses_2052(dev):
    from mertools_amd._lib import MerError
    ops = _ops()
    x = torch.zeros((4, 2052), device=dev)
    with pytest.raises(MerError, match="unsupported"):
        ops.layernorm(x, None, None, 1e-5)
    torch.cuda.synchronize()


@pytest.mark.parametrize("D,M", [(1280, 77), (384, 77), (384, LN_ROWS_M)])
def test_layernorm_strided_rows(dev, D, M):
    """ldx = D + 4, ld32 = D + 8, ld16 = D + 12: the input's gap columns hold a canary that must not be read (it would wreck the
    statistics), the outputs' gap columns and two spare rows a canary that must survive."""
    ops = _ops()
    x, g, b = _ln_inputs(M, D)
    xw = torch.full((M, D + 4), R.CANARY32, device=dev)
    xw[:, :D] = x.to(dev)
    b32 = torch.full((M + 2, D + 8), R.CANARY32, device=dev)
    bh, bl = R.canary16((M + 2, D + 12), "bf16", dev), R.canary16((M + 2, D + 12), "bf16", dev)
    ops.layernorm(xw, g.to(dev), b.to(dev), 1e-5, act="gelu", dtype="bf16", M=M, D=D, ldx=D + 4, out=(b32[:M, :D], bh[:M, :D], bl[:M, :D]))
    d32, dh, dl = ops.layernorm(x.to(dev), g.to(dev), b.to(dev), 1e-5, act="gelu", dtype="bf16", out16=True, out16_lo=True)
    torch.cuda.synchronize()
    assert (b32[:, D:] == R.CANARY32).all() and (b32[M:] == R.CANARY32).all(), "layernorm wrote outside its fp32 rows"
    for buf in (bh, bl):
        assert R.is_canary16(buf[:, D:]) and R.is_canary16(buf[M:]), "layernorm wrote outside its 16-bit rows"
    assert torch.equal(b32[:M, :D], d32) and torch.equal(bh[:M, :D], dh) and torch.equal(bl[:M, :D], dl), "strided != dense"
    assert_close(d32.cpu(), R.layernorm_ref(x, g, b, 1e-5, "gelu").float(), 2e-6, f"layernorm strided D={D}")


@pytest.mark.parametrize("D", [384, 1280])
def test_vit_assemble_wide(dev, D):
    ops = _ops()
    N, P = 2, 10                                          # 22 rows: the last workgroup has two idle waves
    patch, cls, pos = R.rand((N * P, D), 22), R.rand((D,), 23), R.rand((P + 1, D), 24)
    g, b = R.rand((D,), 25) * 0.1 + 1, R.rand((D,), 26) * 0.1
    tok = torch.cat([cls.expand(N, 1, D), patch.view(N, P, D)], 1) + pos[None]
    ref = R.layernorm_ref(tok, g, b, 1e-5).float().view(-1, D)
    o32, oh, ol = ops.vit_assemble(patch.to(dev), cls.to(dev), pos.to(dev), g.to(dev), b.to(dev), 1e-5, N, P, D,
                                   dtype="bf16", out16=True, out16_lo=True)
    p32, ph, pl = ops.vit_assemble(patch.to(dev), cls.to(dev), pos.to(dev), None, None, 1e-5, N, P, D, dtype="bf16", out16=True, out16_lo=True)
    torch.cuda.synchronize()
    assert_close(o32.cpu(), ref, 2e-6, f"vit_assemble + LN D={D}")
    assert_close((oh.float() + ol.float()).cpu(), ref, _plane_tol(2e-6, "bf16"), f"vit_assemble + LN D={D} bf16 planes")
    assert torch.equal(oh, o32.bfloat16())
    assert torch.equal(p32.cpu(), tok.view(-1, D)), "assembly without LayerNorm is one fp32 add per element"
    assert torch.equal(ph, p32.bfloat16())
    assert_close((ph.float() + pl.float()).cpu(), tok.view(-1, D), R.U2, f"vit_assemble D={D} bf16 planes")


@pytest.mark.parametrize("pos_mode", [0, 1])
@pytest.mark.parametrize("D", [384, 1280])
def test_bert_embed_wide(dev, D, pos_mode):
    ops = _ops()
    B, T, V, pad = 3, 21, 100, 1
    gen = torch.Generator().manual_seed(27)
    ids = torch.randint(3, V, (B, T), generator=gen)
    ids[1, 12:] = pad
    ids[2, 5:] = pad
    tt = torch.randint(0, 2, (B, T), generator=gen)
    word, pos, typ = R.rand((V, D), 28), R.rand((T + 4, D), 29), R.rand((2, D), 30)
    g, b = R.rand((D,), 31) * 0.1 + 1, R.rand((D,), 32) * 0.1
    if pos_mode == 1:
        m = (ids != pad).long()
        pid = torch.cumsum(m, 1) * m + pad
    else:
        pid = torch.arange(T)[None].expand(B, T)
    ref = R.layernorm_ref(word[ids] + typ[tt] + pos[pid], g, b, 1e-12).float().view(-1, D)
    o32, oh, ol = ops.bert_embed(ids.to(dev), tt.to(dev), word.to(dev), pos.to(dev), typ.to(dev), pos_mode, pad, g.to(dev), b.to(dev), 1e-12,
                                 dtype="bf16", out16_lo=True)
    torch.cuda.synchronize()
    assert_close(o32.cpu(), ref, 2e-6, f"bert_embed D={D}")
    assert_close((oh.float() + ol.float()).cpu(), ref, _plane_tol(2e-6, "bf16"), f"bert_embed D={D} bf16 planes")
    assert torch.equal(oh, o32.bfloat16())


# ------------------------------------------------------------------------------------------------------ element-wise kernels
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("M", [1, 300])
@pytest.mark.parametrize("F", [4, 1364, 4096])
def test_swiglu(dev, F, M, pad, dtype):
    """silu(gate) * linear with saturating gates: +-30 and +-100 in the gate half (exp(100) overflows fp32: the kernel's
    a / (1 + exp(-a)) must go to -0, not NaN)."""
    ops = _ops()
    y = torch.full((M, 2 * F + pad), R.CANARY32)
    y[:, :2 * F] = R.rand((M, 2 * F), 70, 2.0)
    y[:, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    ref = R.swiglu_ref(y, F).float()
    oh, ol = ops.swiglu(y.to(dev), F, dtype=dtype, lo=True)
    torch.cuda.synchronize()
    assert_close((oh.float() + ol.float()).cpu(), ref, _plane_tol(2e-6, dtype), f"swiglu F={F} M={M} ldy={2 * F + pad} {dtype}")
    assert (oh[:, 3].float().abs() < 1e-30).all(), "silu(-100) is 0 to fp32"


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("N,T,D", [(3, 1, 64), (5, 257, 768), (2, 1568, 100), (4, 1370, 1536)])
def test_token_reduce(dev, N, T, D, mean):
    """scale * x.sum(1).  The project has no number for a 1568-term fp32 sum, so the yardstick is measured per case on the CPU:
    4 x the error of torch's own fp32 x.sum(1) against fp64, not below 1e-6 (torch sums pairwise, the kernel in four sequential
    chains of T / 4 terms: the factor covers the different order).

    Measured on an MI355X (kernel error / torch fp32 CPU error / bound): T = 257, D = 768: 2.1e-7 / 1.7e-7 / 1e-6; T = 1568,
    D = 100: 3.9e-7 / 1.2e-7 / 1e-6; T = 1370, D = 1536: 5.1e-7 / 1.8e-7 / 1e-6; T = 1: exact."""
    ops = _ops()
    x = R.rand((N, T, D), 80)
    scale = 1.0 / T if mean else 1.0
    ref = R.token_sum_ref(x, scale)
    cpu_err, _ = rel_err(x.sum(1) * scale, ref)
    bound = max(1e-6, 4.0 * cpu_err)
    out = ops.token_reduce(x.to(dev), scale)
    torch.cuda.synchronize()
    e = assert_close(out.cpu(), ref.float(), bound, f"token_reduce N={N} T={T} D={D} scale={scale:.3g}")
    print(f"token_reduce T={T} D={D}: err {e:.3e}, fp32 CPU sum {cpu_err:.3e}, bound {bound:.3e}")


def test_add_pos_is_bit_exact(dev):
    ops = _ops()
    rows, P, D = 200, 37, 100                             # rows no multiple of P, D no multiple of 64
    x, pos = R.rand((rows, D), 81), R.rand((P, D), 82)
    out = ops.add_pos(x.to(dev).clone(), pos.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), R.add_pos_ref(x, pos))


def test_split16_bf16(dev):
    ops = _ops()
    x = R.rand((100003,), 83, 5.0)                        # no multiple of the 256-thread block
    hi, lo = ops.split16(x.to(dev), "bf16")
    only, none = ops.split16(x.to(dev), "bf16", lo=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(hi, only)
    assert torch.equal(hi.cpu(), x.bfloat16()), "hi is the round-to-nearest-even bf16 of x"
    got = hi.float().cpu().double() + lo.float().cpu().double()
    assert ((got - x.double()).abs() <= R.U2 * x.double().abs()).all(), "hi + lo must carry 16 significand bits of every element"


def test_sum_pool_empty_and_long_segments(dev):
    ops = _ops()
    M, D = 1100, 100                                      # D % 64 != 0: the second column block is partial
    h = R.rand((M, D), 84)
    starts = torch.tensor([0, 50, 50, 1050], dtype=torch.int32)
    lens = torch.tensor([50, 0, 1000, 50], dtype=torch.int32)
    fr, pooled = ops.sum_pool([h.to(dev)], starts.to(dev), lens.to(dev), frames=True)
    torch.cuda.synchronize()
    assert torch.equal(fr.cpu(), h)
    assert (pooled[1] == 0).all(), "an empty segment pools to zeros (not NaN)"
    for i in (0, 2, 3):                                   # the empty segment's neighbours are what they would be without it
        s, n = int(starts[i]), int(lens[i])
        assert_close(pooled[i].cpu(), h[s:s + n].double().mean(0).float(), 1e-6, f"segment mean, segment {i} ({n} rows)")


# -------------------------------------------------------------------------------------------------------- HuBERT front end
CONV0_GEOM = [(48, 10, 5), (512, 12, 4), (100, 3, 2), (64, 16, 8)]       # (C, k, stride): C < 65, k > 10, C % 8 != 0, C < 65 and k = 16


def _conv0_L(k, stride, which):
    return 4000 if which == "L4000" else 256 * stride + k             # T0 = 257: one frame in the second 256-frame chunk


@pytest.mark.parametrize("which", ["L4000", "T0_257"])
@pytest.mark.parametrize("C,k,stride", CONV0_GEOM)
def test_hubert_conv0_plain(dev, C, k, stride, which):
    ops = _ops()
    B, L = 3, _conv0_L(k, stride, which)
    wav, w, bias = R.rand((B, L), 17), R.rand((C, k), 18) * 0.3, R.rand((C,), 19)
    ref = R.conv0_ref(wav, w, stride, bias).float()
    out = ops.hubert_conv0_plain(wav.to(dev), w.to(dev), bias.to(dev), stride=stride)
    nob = ops.hubert_conv0_plain(wav.to(dev), w.to(dev), None, stride=stride)
    torch.cuda.synchronize()
    assert out.shape == ref.shape and (which != "T0_257" or out.shape[1] == 257)
    assert_close(out.cpu(), ref, 2e-6, f"conv0 plain C={C} k={k} s={stride} L={L}")
    assert_close(nob.cpu(), R.conv0_ref(wav, w, stride).float(), 2e-6, f"conv0 plain without bias C={C} k={k} s={stride} L={L}")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("which", ["L4000", "T0_257"])
@pytest.mark.parametrize("C,k,stride", CONV0_GEOM)
def test_hubert_conv0_gn_two_pass_fallback(dev, C, k, stride, which, dtype):
    """The two-pass form of conv0 + GroupNorm + GELU (every shape outside k <= 10, C % 8 == 0, C >= 65) on white noise with ragged
    valid_frames, at test_hubert_conv0_groupnorm_gelu's 5e-6.  Its statistics are E[y^2] - E[y]^2 over fp32 partial sums, which is
    the right tool for "other shapes" and white noise; it is NOT held to test_hubert_conv0_statistics_on_a_correlated_signal
    (DC + slow sine under difference filters, where that subtraction cancels): see the figures at the end of this docstring.

    Measured on an MI355X on that correlated signal (B, L, k, stride, filters and valid_frames as in that test, but C = 48 so that
    the fallback runs; f16 hi + lo; bound there 1e-4): 3.8e-6 / 5.0e-6 / 6.1e-6 for the rows of 7999 / 4100 / 257 valid frames,
    against 3.8e-6 / 5.0e-6 / 5.7e-6 of the moment-based fast path at C = 512 — on this signal the fallback loses nothing."""
    ops = _ops()
    B, L = 3, _conv0_L(k, stride, which)
    T0 = (L - k) // stride + 1
    wav, w = R.rand((B, L), 17), R.rand((C, k), 18) * 0.3
    g, b = R.rand((C,), 19) * 0.1 + 1.0, R.rand((C,), 20) * 0.1
    valid = [T0, T0 // 3 + 1, 256 if which == "T0_257" else 300]
    ref = R.conv0_gn_gelu_ref(wav, w, stride, g, b, 1e-5, valid).float()
    oh, ol = ops.hubert_conv0_gn(wav.to(dev), w.to(dev), g.to(dev), b.to(dev), 1e-5, stride=stride, dtype=dtype, lo=True,
                                 valid_frames=torch.tensor(valid, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    out = (oh.float() + ol.float()).cpu()
    for i in range(B):                                    # frames past valid[i] are normalised with the same statistics: all T0 are defined
        assert_close(out[i], ref[i], _plane_tol(5e-6, dtype), f"conv0+GN+GELU fallback C={C} k={k} s={stride} L={L} {dtype} row {i} ({valid[i]} valid)")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("T,D,G,K", [(37, 96, 4, 128), (50, 64, 2, 5)])
def test_posconv_pack_ragged(dev, T, D, G, K, dtype):
    ops = _ops()
    lens = [1, T, T - 1, 20]
    x = R.rand((len(lens), T, D), 85)
    ref = R.posconv_pack_ref(x, G, K, lens).float()
    oh, ol = ops.posconv_pack(x.to(dev), G, K, dtype=dtype, lo=True, valid_frames=torch.tensor(lens, dtype=torch.int32, device=dev))
    fh, fl = ops.posconv_pack(x.to(dev), G, K, dtype=dtype, lo=True)
    torch.cuda.synchronize()
    assert_close((oh.float() + ol.float()).cpu(), ref, _plane_tol(1e-6, dtype), f"posconv_pack ragged T={T} K={K} {dtype}")
    assert_close((fh.float() + fl.float()).cpu(), R.posconv_pack_ref(x, G, K).float(), _plane_tol(1e-6, dtype), f"posconv_pack T={T} K={K} {dtype}")
    zero = ref == 0
    assert (oh[zero.to(dev)] == 0).all() and (ol[zero.to(dev)] == 0).all(), "padding and frames past the row's length are exact zeros"


@pytest.mark.parametrize("batch", [0, 1, 2])
def test_hubert_valid_frames(dev, batch):
    """Exact integer equality with the pure-Python recursion: B = 130 (three 64-thread blocks); over the three batches
    valid_samples = 1 + 321 i, i = 0 .. 389, hits every residue of the stack's total stride 320, starts below the 400-sample
    receptive field and ends beyond L (the kernel clamps to L)."""
    ops = _ops()
    kernels, strides = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
    B, L = 130, 100000
    vs = [1 + 321 * i for i in range(batch * B, (batch + 1) * B)]
    assert (batch != 0 or vs[1] < 400) and (batch != 2 or vs[-1] > L)
    want = R.valid_frames_ref(vs, L, kernels, strides)
    vd = torch.tensor(vs, dtype=torch.int32, device=dev)
    t0, tn = ops.hubert_valid_frames(vd, L, kernels, strides)
    lens = ops.hubert_valid_frames(vd, L, kernels, strides, all_layers=True)
    one = ops.hubert_valid_frames(vd, L, kernels[:1], strides[:1], all_layers=True)
    torch.cuda.synchronize()
    assert t0.tolist() == want[0] and tn.tolist() == want[-1]
    assert lens.tolist() == want
    assert one.tolist() == want[:1]


# ---------------------------------------------------------------------------------------------------------------- patchify
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("P,S", [(14, 56), (6, 24)])
def test_vit_patchify_generic_path(dev, P, S, dtype):
    """P % 4 != 0 (CLIP-L/14: 3 * 14 * 14 = 588 -> 592 columns; P = 6: 108 -> 112): the one-element-per-thread kernel, rows
    zero-padded to a multiple of 8 columns."""
    ops = _ops()
    px = R.rand((3, 3, S, S), 21)
    ref = R.vit_patchify_ref(px, P)
    cols = 3 * P * P
    ph, pl = ops.vit_patchify(px.to(dev), P, dtype=dtype, lo=True)
    torch.cuda.synchronize()
    assert ph.shape == ref.shape and ref.shape[1] == (cols + 7) // 8 * 8 and ref.shape[1] > cols
    assert (ph[:, cols:] == 0).all() and (pl[:, cols:] == 0).all(), "pad columns must be exactly zero in both planes"
    assert_close((ph.float() + pl.float()).cpu(), ref, _plane_tol(1e-6, dtype), f"patchify P={P} {dtype}")
    assert torch.equal(ph.cpu(), ref.to(ph.dtype))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("B,Fr,ts,P,S", [(2, 4, 2, 16, 32), (1, 6, 3, 4, 8)])
def test_video_patchify(dev, B, Fr, ts, P, S, dtype):
    ops = _ops()
    px = R.rand((B, Fr, 3, S, S), 86)
    ref = R.video_patchify_ref(px, P, ts)
    ph, pl = ops.video_patchify(px.to(dev), P, ts, dtype=dtype, lo=True)
    torch.cuda.synchronize()
    assert_close((ph.float() + pl.float()).cpu(), ref, _plane_tol(1e-6, dtype), f"video_patchify {(B, Fr, ts, P, S)} {dtype}")
    assert torch.equal(ph.cpu(), ref.to(ph.dtype))
