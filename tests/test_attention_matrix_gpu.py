"""Every attention instantiation at its dispatch edges (GPU), against the fp64 references of tests/op_refs.py.

The dispatch tables of csrc/attention.hip are restated below (SP_EDGES, CLS_EDGES) and the case tables are built from them, so
the coverage can be read off the tables: every attn_sp_kernel<T, NKT, BIAS> (NKT = edge / 16) and the streaming kernel run
unmasked and masked-and-poisoned, row-major and head-major, in f16 and bf16; every attn_cls bucket at both edges.

Entry point -> test
  mer_attention        test_attention_matrix[rm-*] (+ test_outputs_stay_inside_their_rows[sp / stream])
  mer_attention_hm     test_attention_matrix[hm-*] (fp64 reference AND bit equality with mer_attention) (+ canary [hm])
  mer_attention_bias   test_attention_bias_matrix, test_attention_bias_refuses_the_streaming_range (+ canary [bias])
  mer_attention_cls    test_attention_cls_matrix, test_attention_cls_strided_operands, test_attention_cls_refuses_585
  mer_attention_f32    test_attention_f32_planes (+ canary [f32])

How a masked case is made to fail loudly.  Every masked case runs on poisoned inputs (op_refs.poison_masked: K rows >= kv_len
hold 4 x the first query, V rows 50.0) and is asserted per sequence on rows < kv_len[b] only (rows beyond are unspecified by the
ABI).  The kernels never load rows >= kv_len (the single-pass kernels zero them in LDS, the streaming kernel re-fetches the last
valid row), so the poison guards that property: a kernel that reads them is off by order 1.  A wrong mask COMPARE leaks a
zero-score key instead; input family "neg" (+1.6 on Q, -1.6 on K before rounding: valid scores near -22, a zero K row scores 0)
makes that an error of order 1 in the single-pass kernels, where plain N(0, 1) inputs ("rand") would hide it at 1 / n.  In the
streaming kernel the leaked key is a copy of the last valid one (1 / n): its ragged sets hold 1 and 65 / 129.

Tolerances (max-norm relative error, per sequence where ragged) are the project's own, from tests/test_ops_gpu.py:
f16 hi + lo 8e-4 and bf16 hi + lo 6e-3 (test_attention), f16 hi alone 1.5e-3 (test_attention_kv_len_mask), f16 + bias 2e-3
(test_attention_with_score_bias), attention_f32 1e-5 (+ 2^-16 for bf16 planes: hi + lo of bf16 carries 16 significand bits).
bf16 + bias reads the hi plane alone, for which the project has no number: max(6e-3, 2 x op_refs.attention_rounding_model of
that very case, output rounding included) — computed on the CPU at run time, never from the kernel's output; the factor 2 covers
what the model leaves out (fp32 accumulation order, the hardware exp2).  Every failure message carries measured error, bound
and the model's error.  Each case is launched twice into separate outputs which must be bit-identical (a staging race shows as a
run-to-run difference).
"""
import functools

import pytest
import torch

import op_refs as R
from util import rel_err

pytestmark = pytest.mark.gpu

SP_EDGES = (64, 128, 224, 256, 288, 512)      # launch_attn: T <= edge -> attn_sp_kernel<NKT = edge / 16>; beyond: attn_stream_kernel
CLS_EDGES = (64, 208, 264, 584)               # launch_attn_cls: T <= edge -> attn_cls_kernel<NIT = edge / 8>; beyond: refused
SCALE = 0.125

# single-pass lengths per bucket: first length, [a length of the "rare branch" range T <= TP - 32,] a length in the last two key
# tiles that is no multiple of 4, the edge.  (The first bucket's first lengths are the tiny ones.)
SP_T = {64: (1, 15, 16, 17, 50, 64), 128: (65, 70, 111, 128), 224: (129, 150, 210, 224), 256: (225, 250, 256),
        288: (257, 275, 288), 512: (289, 300, 497, 512)}
STREAM_T = (513, 576, 641, 1568)              # first length, a whole number of 64-key blocks, one key into a block, VideoMAE


def _check_tables():
    lo = 0
    for edge in SP_EDGES:
        ts, tp = SP_T[edge], edge
        assert all(lo < t <= edge for t in ts) and lo + 1 in ts and edge in ts
        assert any(t % 4 and tp - 32 < t <= tp for t in ts), edge
        if lo + 1 <= tp - 32:                                   # the bucket has unmasked lengths that take the rare branch
            assert any(t <= tp - 32 and t not in (1, lo + 1) for t in ts), edge
        lo = edge
    assert all(t > SP_EDGES[-1] for t in STREAM_T)


_check_tables()


def sp_tp(T):
    return next(e for e in SP_EDGES if T <= e)


def ragged_lens(T):
    """Key lengths of a ragged batch at sequence length T: T itself, 1, and both sides of the kernel's mask paths."""
    if T > SP_EDGES[-1]:
        m = {513: 256, 576: 512, 641: 640, 1568: 832}[T]        # around one multiple of the 64-key block
        extra = 129 if T in (576, 1568) else 65                 # one key in the last block of a short row
        want = [T, 1, m - 1, m, m + 1, extra]
    else:
        tp = sp_tp(T)
        early = 16 * max(1, (tp - 32) // 32)                    # a multiple of 16 with early + 1 <= TP - 32: the rare branch
        assert early + 1 <= tp - 32
        want = [T, 1, early - 1, early, early + 1]
        late = tp - 16                                          # the multiple of 16 inside the last two tiles
        if late < T:
            want += [late - 1, late, late + 1]
    out = []
    for n in want:
        if 1 <= n <= T and n not in out:
            out.append(n)
    return out


def _ops():
    from mertools_amd import ops
    return ops


def _inputs(B, T, H, dtype, family, seed):
    x = R.rand((B * T, 3 * H * 64), seed)
    if family == "neg":
        D = H * 64
        x[:, :D] += 1.6
        x[:, D:2 * D] -= 1.6
    return x.to(R.T16[dtype])


def _ref(qkv, B, T, H, lens=None, bias=None, gate=None):
    """attention_ref, one sequence at a time above 512 keys (the fp64 score tensor of a whole ragged batch is large there)."""
    if T <= 512:
        return R.attention_ref(qkv, B, T, H, SCALE, lens, bias, gate)
    q3 = qkv.view(B, T, -1)
    return torch.cat([R.attention_ref(q3[b], 1, T, H, SCALE, None if lens is None else lens[b:b + 1],
                                      bias, None if gate is None else gate[b:b + 1]) for b in range(B)])


@functools.lru_cache(maxsize=2)
def _plain_case(T, dtype, masked, family):
    lens = ragged_lens(T) if masked else None
    B, H = (len(lens) if masked else (3 if T <= 512 else 2)), 2
    qkv = _inputs(B, T, H, dtype, family, 1000 + T)
    ref = _ref(qkv, B, T, H, lens)
    if masked:
        qkv = R.poison_masked(qkv, B, T, H, lens)
    return B, H, lens, qkv, ref


def _assert_seqs(out, ref, lens, bound, what, model):
    """Per sequence over rows < lens[b]; the failure message names measured error, bound and the CPU rounding model's error."""
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    worst = 0.0
    for b in range(ref.shape[0]):
        n = int(lens[b]) if lens is not None else ref.shape[1]
        assert torch.isfinite(out[b, :n]).all(), f"{what}: non-finite output in sequence {b} (kv_len {n})"
        e, _ = rel_err(out[b, :n], ref[b, :n])
        worst = max(worst, e)
        if e > bound:
            raise AssertionError(f"{what}: sequence {b} (kv_len {n}): max-norm rel err {e:.3e} > bound {bound:.2e} "
                                 f"(CPU rounding model of this case: {model():.3e})")
    print(f"{what}: err {worst:.3e} bound {bound:.2e}")
    return worst


def _plain_cases():
    cases = []
    for T in [t for e in SP_EDGES for t in SP_T[e]] + list(STREAM_T):
        for dtype in ("f16", "bf16"):
            variants = [(False, "rand"), (True, "rand")] + ([(True, "neg")] if T <= SP_EDGES[-1] and T > 1 else [])
            for masked, family in variants:
                for layout in ("rm", "hm"):
                    cases.append(pytest.param(layout, T, dtype, masked, family,
                                              id=f"{layout}-T{T}-{dtype}-{'ragged' if masked else 'full'}-{family}"))
    return cases


@pytest.mark.parametrize("layout,T,dtype,masked,family", _plain_cases())
def test_attention_matrix(dev, layout, T, dtype, masked, family):
    ops = _ops()
    B, H, lens, qkv, ref = _plain_case(T, dtype, masked, family)
    D = H * 64
    qd = qkv.to(dev)
    kv = torch.tensor(lens, dtype=torch.int32, device=dev) if masked else None
    oh, ol = ops.attention(qd, B, T, H, SCALE, kv_len=kv, out_lo=True)
    if layout == "rm":
        oh2, ol2 = ops.attention(qd, B, T, H, SCALE, kv_len=kv, out_lo=True)
    else:
        hm = R.to_headmajor(qd, B, T, H)
        rm_h, rm_l = oh, ol
        oh, ol = ops.attention_hm(hm, B, T, H, SCALE, kv_len=kv, out_lo=True)
        oh2, ol2 = ops.attention_hm(hm, B, T, H, SCALE, kv_len=kv, out_lo=True)
    torch.cuda.synchronize()
    assert torch.equal(oh, oh2) and torch.equal(ol, ol2), "two launches of the same case differ"
    what = f"attention {layout} T={T} (TP {sp_tp(T) if T <= 512 else 'stream'}) {dtype} lens={lens} {family}"

    def model(round_out=False):
        clean = _inputs(B, T, H, dtype, family, 1000 + T)
        return R.attention_rounding_model(clean, B, T, H, SCALE, lens, dtype=dtype, round_out=round_out)
    both = (oh.float() + ol.float()).cpu().view(B, T, D)
    _assert_seqs(both, ref, lens, 8e-4 if dtype == "f16" else 6e-3, what + " hi+lo", model)
    if dtype == "f16":
        _assert_seqs(oh.float().cpu().view(B, T, D), ref, lens, 1.5e-3, what + " hi", lambda: model(True))
    if layout == "hm":       # the existing invariant (test_qkv_headmajor_gemm_and_attention), for every bucket, dtype and mask
        for b in range(B):
            n = lens[b] if masked else T
            assert torch.equal(oh.view(B, T, D)[b, :n], rm_h.view(B, T, D)[b, :n]), f"{what}: head-major != row-major (hi), sequence {b}"
            assert torch.equal(ol.view(B, T, D)[b, :n], rm_l.view(B, T, D)[b, :n]), f"{what}: head-major != row-major (lo), sequence {b}"


# ------------------------------------------------------------------------------------------------------------- score bias
def _bias_T():
    out, lo = [], 0
    for e in SP_EDGES:
        out += [lo + 1, e]
        lo = e
    return out


def _bias_case(T, dtype, gated, masked, ldb_extra=0):
    lens = ragged_lens(T) if masked else None
    B, H = (len(lens) if masked else 3), 2
    qkv = (R.rand((B * T, 3 * H * 64), 2000 + T) * 0.5).to(R.T16[dtype])
    ldb = (T + 3) // 4 * 4 + ldb_extra
    bias = torch.full((H, T, ldb), 1e30)                  # the pad columns must never reach a score
    bias[:, :, :T] = R.rand((H, T, T), 2001 + T)
    gate = (1.0 + R.rand((B, H, T), 2002 + T).abs()) if gated else None
    return B, H, lens, qkv, bias, gate


def _run_bias(dev, T, dtype, gated, masked, ldb_extra=0):
    ops = _ops()
    B, H, lens, qkv, bias, gate = _bias_case(T, dtype, gated, masked, ldb_extra)
    D = H * 64
    ref = R.attention_ref(qkv, B, T, H, SCALE, lens, bias, gate)
    run = R.poison_masked(qkv, B, T, H, lens).to(dev) if masked else qkv.to(dev)
    kv = torch.tensor(lens, dtype=torch.int32, device=dev) if masked else None
    args = dict(gate=gate.to(dev) if gated else None, kv_len=kv)
    o1 = ops.attention_bias(run, B, T, H, SCALE, bias.to(dev), **args)
    o2 = ops.attention_bias(run, B, T, H, SCALE, bias.to(dev), **args)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2), "two launches of the same case differ"

    def model():
        return R.attention_rounding_model(qkv, B, T, H, SCALE, lens, bias, gate, dtype=dtype, round_out=True)
    bound = 2e-3 if dtype == "f16" else max(6e-3, 2.0 * model())
    _assert_seqs(o1.float().cpu().view(B, T, D), ref, lens, bound,
                 f"attention_bias T={T} (TP {sp_tp(T)}) {dtype} gated={gated} lens={lens} ldb={bias.shape[2]}", model)


@pytest.mark.parametrize("masked", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("T", _bias_T())
def test_attention_bias_matrix(dev, T, dtype, gated, masked):
    """Every attn_sp_kernel<T, NKT, true> at its first length (65, 129, 225, 257, 289: not multiples of 4 — the last bias-row
    vector load straddles T and reads the 1e30 pad columns) and at its edge, with and without a poisoned ragged kv_len."""
    _run_bias(dev, T, dtype, gated, masked)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_attention_bias_wider_table_rows(dev, dtype):
    _run_bias(dev, 210, dtype, True, True, ldb_extra=8)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_attention_bias_refuses_the_streaming_range(dev, dtype):
    from mertools_amd._lib import MerError
    ops = _ops()
    B, T, H = 1, SP_EDGES[-1] + 1, 1
    qkv = torch.zeros((B * T, 3 * 64), dtype=R.T16[dtype], device=dev)
    bias = torch.zeros((H, T, 516), device=dev)
    with pytest.raises(MerError, match="rc=4|not supported"):
        ops.attention_bias(qkv, B, T, H, SCALE, bias)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------- CLS query
def _cls_lens(T):
    m = 8 * max(1, T // 16)                                      # a multiple of the kernel's 8-key wave-load inside the row
    out = []
    for n in (T, 1, m - 1, m, m + 1, T - 1):
        if 1 <= n <= T and n not in out:
            out.append(n)
    return out


def _cls_ref(q, qkv, B, T, H, lens):
    D = H * 64
    k = qkv[:, D:2 * D].double().view(B, T, H, 64)
    v = qkv[:, 2 * D:].double().view(B, T, H, 64)
    sc = torch.einsum("bhd,bthd->bht", q.double().view(B, H, 64), k) * SCALE
    for b, n in enumerate(lens):
        sc[b, :, n:] = float("-inf")
    return torch.einsum("bht,bthd->bhd", torch.softmax(sc, -1), v).reshape(B, D)


def _cls_T():
    out = [1]
    for e in CLS_EDGES:
        out += [e, e + 1]
    return out[:-1]                                             # 585 is refused: its own test


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("T", _cls_T())
def test_attention_cls_matrix(dev, T, dtype):
    """Every attn_cls_kernel<NIT> bucket at its edge and first length, ragged + poisoned, hi and hi + lo.  All fp32 inside, so the
    plain kernel's bound of the dtype holds with room (test_attention_cls); B * H = 3 * len(lens) is no multiple of the 4 waves of
    a workgroup for most T (the bh >= nbh exit)."""
    ops = _ops()
    lens = _cls_lens(T)
    B, H = len(lens), 3
    D = H * 64
    t16 = R.T16[dtype]
    qkv = R.rand((B * T, 3 * D), 3000 + T).to(t16)
    q = R.rand((B, D), 3001 + T).to(t16)
    ref = _cls_ref(q, qkv, B, T, H, lens)
    bad = R.poison_masked(qkv, B, T, H, lens).to(dev)
    kv = torch.tensor(lens, dtype=torch.int32, device=dev)
    oh, ol = ops.attention_cls(q.to(dev), bad, B, T, H, SCALE, kv_len=kv, out_lo=True)
    oh2, ol2 = ops.attention_cls(q.to(dev), bad, B, T, H, SCALE, kv_len=kv, out_lo=True)
    only_hi = ops.attention_cls(q.to(dev), bad, B, T, H, SCALE, kv_len=kv)
    torch.cuda.synchronize()
    assert torch.equal(oh, oh2) and torch.equal(ol, ol2) and torch.equal(oh, only_hi)
    bound = 8e-4 if dtype == "f16" else 6e-3
    what = f"attention_cls T={T} {dtype} lens={lens}"
    for b in range(B):        # one output row per sequence
        for name, got in (("hi", oh.float()), ("hi+lo", oh.float() + ol.float())):
            e, _ = rel_err(got[b].cpu(), ref[b])
            assert torch.isfinite(got[b]).all() and e <= bound, f"{what} sequence {b} {name}: rel err {e:.3e} > bound {bound:.1e}"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_attention_cls_strided_operands(dev, dtype):
    """ldq, ld and ldo larger than dense; the output's gap columns and two spare rows keep their canary."""
    ops = _ops()
    T, H = 209, 2
    lens = _cls_lens(T)
    B, D = len(lens), H * 64
    t16 = R.T16[dtype]
    qkv = R.rand((B * T, 3 * D), 3100).to(t16)
    q = R.rand((B, D), 3101).to(t16)
    ref = _cls_ref(q, qkv, B, T, H, lens)
    wide_qkv = R.canary16((B * T, 3 * D + 8), dtype, dev)
    wide_qkv[:, :3 * D] = R.poison_masked(qkv, B, T, H, lens).to(dev)
    wide_q = R.canary16((B, D + 8), dtype, dev)
    wide_q[:, :D] = q.to(dev)
    bh, bl = R.canary16((B + 2, D + 16), dtype, dev), R.canary16((B + 2, D + 16), dtype, dev)
    kv = torch.tensor(lens, dtype=torch.int32, device=dev)
    ops.attention_cls(wide_q[:, :D], wide_qkv[:, :3 * D], B, T, H, SCALE, kv_len=kv, out=(bh[:B, :D], bl[:B, :D]))
    dense_h, dense_l = ops.attention_cls(q.to(dev), wide_qkv[:, :3 * D].contiguous(), B, T, H, SCALE, kv_len=kv, out_lo=True)
    torch.cuda.synchronize()
    for buf in (bh, bl):
        assert R.is_canary16(buf[:, D:]) and R.is_canary16(buf[B:]), "attention_cls wrote outside its [B, H*64] output"
    assert torch.equal(bh[:B, :D], dense_h) and torch.equal(bl[:B, :D], dense_l)
    e, _ = rel_err(bh[:B, :D].float().cpu(), ref)
    assert e <= (8e-4 if dtype == "f16" else 6e-3), f"attention_cls strided {dtype}: rel err {e:.3e}"


def test_attention_cls_refuses_585(dev):
    from mertools_amd._lib import MerError
    ops = _ops()
    T = CLS_EDGES[-1] + 1
    qkv = torch.zeros((T, 3 * 64), dtype=torch.float16, device=dev)
    q = torch.zeros((1, 64), dtype=torch.float16, device=dev)
    with pytest.raises(MerError, match="unsupported"):
        ops.attention_cls(q, qkv, 1, T, 1, SCALE)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ fp32 operands
F32_SHAPES = [(3, 50, 2, None), (2, 197, 12, None), (2, 249, 3, [249, 100]), (1, 600, 2, None), (4, 16, 1, [16, 1, 7, 15]),
              (1, 1568, 1, None)]                                           # test_attention_f32's


def _f32_cases():
    cases = [pytest.param(B, T, H, lens, "bf16", id=f"T{T}-bf16") for B, T, H, lens in F32_SHAPES]
    for T in (70, 300, 513):
        for dtype in ("f16", "bf16"):
            lens = ragged_lens(T)
            cases.append(pytest.param(len(lens), T, 2, lens, dtype, id=f"T{T}-{dtype}-ragged-poisoned"))
    return cases


@pytest.mark.parametrize("B,T,H,lens,dtype", _f32_cases())
def test_attention_f32_planes(dev, B, T, H, lens, dtype):
    """mer_attention_f32 with bf16 output planes (hi + lo of bf16 carries 16 significand bits: 1e-5 + 2^-16) and, in both plane
    types, ragged lengths around its 16-key tiles on poisoned inputs."""
    ops = _ops()
    D = H * 64
    qkv = R.rand((B * T, 3 * D), 4000 + T)
    qkv[:, :D] *= 3.0
    ref = _ref(qkv, B, T, H, lens)
    run = (R.poison_masked(qkv, B, T, H, lens) if lens is not None else qkv).to(dev)
    kv = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    oh, ol = ops.attention_f32(run, B, T, H, SCALE, kv_len=kv, dtype=dtype)
    oh2, ol2 = ops.attention_f32(run, B, T, H, SCALE, kv_len=kv, dtype=dtype)
    torch.cuda.synchronize()
    assert torch.equal(oh, oh2) and torch.equal(ol, ol2), "two launches of the same case differ"
    bound = 1e-5 if dtype == "f16" else 1e-5 + R.U2
    _assert_seqs((oh.float() + ol.float()).cpu().view(B, T, D), ref, lens, bound, f"attention_f32 T={T} {dtype} planes lens={lens}",
                 lambda: float("nan"))


# ------------------------------------------------------------------------------------------------------- strided outputs
@pytest.mark.parametrize("family,T,dtype", [("sp", 111, "bf16"), ("stream", 641, "f16"), ("hm", 210, "f16"), ("bias", 129, "bf16"),
                                            ("f32", 70, "f16")])
def test_outputs_stay_inside_their_rows(dev, family, T, dtype):
    """ldo = D + 16 and two spare rows, pre-filled with a canary bit pattern: the gap columns and the spare rows must still hold
    it after the launch, and the strided result equals the dense one bit for bit."""
    ops = _ops()
    B, H = 3, 2
    D = H * 64
    bh, bl = R.canary16((B * T + 2, D + 16), dtype, dev), R.canary16((B * T + 2, D + 16), dtype, dev)
    out = (bh[:B * T, :D], bl[:B * T, :D])
    if family == "f32":
        qkv = R.rand((B * T, 3 * D), 5000).to(dev)
        dense = ops.attention_f32(qkv, B, T, H, SCALE, dtype=dtype)
        ops.attention_f32(qkv, B, T, H, SCALE, dtype=dtype, out=out)
    else:
        qkv = R.rand((B * T, 3 * D), 5000).to(R.T16[dtype]).to(dev)
        if family == "hm":
            hm = R.to_headmajor(qkv, B, T, H)
            dense = ops.attention_hm(hm, B, T, H, SCALE, out_lo=True)
            ops.attention_hm(hm, B, T, H, SCALE, out=out)
        elif family == "bias":
            bias = R.rand((H, T, (T + 3) // 4 * 4), 5001).to(dev)
            dense = (ops.attention_bias(qkv, B, T, H, SCALE, bias), None)
            ops.attention_bias(qkv, B, T, H, SCALE, bias, out=out)
        else:
            dense = ops.attention(qkv, B, T, H, SCALE, out_lo=True)
            ops.attention(qkv, B, T, H, SCALE, out=out)
    torch.cuda.synchronize()
    for buf, want in ((bh, dense[0]), (bl, dense[1])):
        if want is None:
            assert R.is_canary16(buf), "the lo plane was not requested"
            continue
        assert R.is_canary16(buf[:, D:]), f"{family}: wrote into the gap columns"
        assert R.is_canary16(buf[B * T:]), f"{family}: wrote past the last row"
        assert torch.equal(buf[:B * T, :D], want), f"{family}: strided output differs from the dense one"
