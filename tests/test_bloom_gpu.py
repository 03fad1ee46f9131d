"""BLOOM text encoder on the GPU: mer_alibi_attention and mer_layernorm_row against float64 compositions (tests/bloom_refs.py, shown to
be HF's formulas in tests/test_bloom_cpu.py), HipBloomModel against HF's fp32 BloomModel on four tiny models, the by-name text driver
on a BLOOM checkpoint directory, and a BERT directory still taking its own path.

Bars.  mer_alibi_attention: mer_rope_attention's (tests/test_llama_gpu.py) — 2e-6 on hi + lo (+ 2^-16, what a bf16 pair carries, for
bf16 planes) on inputs where plain fp32 torch on the CPU sits within a quarter of it; under 30x larger q the elementwise bound
bloom_refs.alibi_attention_bound (+ what an f16 pair cannot carry: 2^-21 |ref| + 2^-24).  mer_layernorm_row: mer_rmsnorm's and
mer_layernorm's — 2e-6 max-norm in fp32 and as f16 hi + lo planes, + 2^-16 for bf16 planes; a row offset by 1e4 is held to
bloom_refs.layernorm_bound, which plain fp32 torch is inside and a one-pass variance far outside (tests/test_bloom_cpu.py).  Model: 1e-3
on every hidden state and 8e-4 (1e-3 less the 20 % margin of from_hf()'s ladder) on the UTT and FRAME features under the default
preset, which is the first rung of the ladder that holds both on every tiny model — mertools_amd/llama.py's rule."""
import glob
import os

import numpy as np
import pytest
import torch

import bloom_refs as R
from op_refs import worst_ratio
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu

EPS = float(torch.tensor(1e-5, dtype=torch.float32))     # the value the kernel receives


def _ops():
    from mertools_amd import ops
    return ops


def _t16(dtype):
    return torch.float16 if dtype == "f16" else torch.bfloat16


def _plane_tol(tol, dtype):
    return tol if dtype == "f16" else tol + R.U2


def _planes(hi, lo):
    return hi.double().cpu() + (lo.double().cpu() if lo is not None else 0.0)


# ---------------------------------------------------------------------------------------------------------- mer_alibi_attention
ATT_SHAPES = [(1, 1, 1, 64), (2, 5, 2, 128), (3, 17, 3, 64), (2, 65, 3, 64), (1, 64, 1, 128), (1, 257, 6, 128), (1, 2048, 1, 128)]
SLOPE_SETS = ("bloom", "steepest", "zero")


def _slopes(kind, H):
    if kind == "bloom":
        return R.hf_slopes(H)
    return torch.full((H,), R.STEEPEST if kind == "steepest" else 0.0, dtype=torch.float32)


def _run_attention(dev, x, slopes, B, T, H, hd, dtype="f16", out_lo=True):
    hi, lo = _ops().alibi_attention(x.to(dev), slopes.to(dev), B, T, H, hd, 1.0, out_lo=out_lo, dtype=dtype)
    torch.cuda.synchronize()
    return hi, lo


def _qkv(x, D):
    return x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D]


@pytest.fixture(scope="module", params=ATT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def att_case(request):
    """The inputs of one shape (plain and with q x 30), made once for the three slope sets."""
    B, T, H, hd = request.param
    ld_extra = 8 if T in (5, 65, 257) else 0            # ld > 3 H head_dim
    return request.param, R.attention_inputs(B, T, H, hd, seed=11 + T, ld_extra=ld_extra), \
        R.attention_inputs(B, T, H, hd, seed=11 + T, ld_extra=ld_extra, q_gain=30.0)


@pytest.mark.parametrize("kind", SLOPE_SETS)
def test_alibi_attention_matches_float64(dev, att_case, kind):
    shape, x, x30 = att_case
    B, T, H, hd = shape
    D = H * hd
    slopes = _slopes(kind, H)
    ref = R.alibi_attention_ref(*_qkv(x, D), slopes, B, T, H, hd, 1.0)
    cpu32 = rel_err(R.alibi_attention_ref(*_qkv(x, D), slopes, B, T, H, hd, 1.0, dtype=torch.float32), ref)[0]
    assert cpu32 <= 0.5e-6, f"plain fp32 torch (relative bias) is at {cpu32:.2e} on these inputs: change the inputs, not the bar"
    for dtype in ("f16", "bf16"):
        hi, lo = _run_attention(dev, x, slopes, B, T, H, hd, dtype)
        e = rel_err(_planes(hi, lo), ref)[0]
        print(f"alibi_attention {shape} {kind} {dtype}: {e:.2e} (torch fp32 on the CPU {cpu32:.2e})")
        assert_close(_planes(hi, lo), ref, _plane_tol(2e-6, dtype), f"alibi_attention {shape} {kind} {dtype}")
        hi1, lo1 = _run_attention(dev, x, slopes, B, T, H, hd, dtype)
        assert torch.equal(hi, hi1) and torch.equal(lo, lo1), "two runs on the same inputs differ"
        hi_only, none = _run_attention(dev, x, slopes, B, T, H, hd, dtype, out_lo=False)
        assert none is None and torch.equal(hi_only, hi)
    # 30x larger q: near-one-hot softmax, finite, inside the elementwise bound of the fp32 chain
    ref30 = R.alibi_attention_ref(*_qkv(x30, D), slopes, B, T, H, hd, 1.0)
    bound = R.alibi_attention_bound(*_qkv(x30, D), slopes, B, T, H, hd, 1.0) + ref30.abs() * 2.0 ** -21 + 2.0 ** -24
    hi, lo = _run_attention(dev, x30, slopes, B, T, H, hd)
    assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isfinite(lo.float()).all())
    w = worst_ratio(_planes(hi, lo), ref30, bound)
    w32 = worst_ratio(R.alibi_attention_ref(*_qkv(x30, D), slopes, B, T, H, hd, 1.0, dtype=torch.float32), ref30, bound)
    print(f"alibi_attention {shape} {kind} q x30: at {w:.3f} of the bound (torch fp32 on the CPU {w32:.3f}), max-norm {rel_err(_planes(hi, lo), ref30)[0]:.2e}")
    assert w32 <= 1.0 and w <= 1.0


def test_alibi_attention_rows_do_not_depend_on_the_batch_or_the_padding(dev):
    """Row (b, t) of a (3, 17) call equals, bit for bit, sentence b run alone at T = 9 and at T = 17."""
    B, T, H, hd = 3, 17, 3, 64
    x = R.attention_inputs(B, T, H, hd, seed=5)
    slopes = R.hf_slopes(H)
    hi, lo = _run_attention(dev, x, slopes, B, T, H, hd)
    hi, lo = hi.view(B, T, -1), lo.view(B, T, -1)
    for b in range(B):
        for n in (9, 17):
            xs = x.view(B, T, -1)[b, :n].contiguous()
            h1, l1 = _run_attention(dev, xs, slopes, 1, n, H, hd)
            assert torch.equal(h1, hi[b, :n]) and torch.equal(l1, lo[b, :n]), (b, n)


@pytest.mark.parametrize("hd", [64, 128])
def test_alibi_attention_is_causal(dev, hd):
    """Key t + 1 (its q, k and v) filled with 1e30 does not change row t's bits, nor any row before it."""
    B, T, H = 2, 40, 2
    x = R.attention_inputs(B, T, H, hd, seed=9)
    slopes = R.hf_slopes(H)
    hi, lo = _run_attention(dev, x, slopes, B, T, H, hd)
    for t in (0, 8, 15, 31, 38):
        y = x.clone()
        y.view(B, T, -1)[:, t + 1] = 1e30
        h1, l1 = _run_attention(dev, y, slopes, B, T, H, hd)
        assert torch.equal(h1.view(B, T, -1)[:, :t + 1], hi.view(B, T, -1)[:, :t + 1]) and torch.equal(l1.view(B, T, -1)[:, :t + 1], lo.view(B, T, -1)[:, :t + 1]), t


@pytest.mark.parametrize("hd", [64, 128])
def test_zero_slopes_are_the_rotary_kernel_at_position_zero_and_real_slopes_move_the_result(dev, hd):
    """The two operators share one kernel body: with slopes = 0 and with cos = 1, sin = 0 both are plain causal attention, bit for bit
    (x * 1 - y * 0 and s + 0 * (j - t) change no bit of a non-zero value).  BLOOM's slopes move the result by far more than any bar."""
    B, T, H = 2, 37, 3
    D = H * hd
    x = R.attention_inputs(B, T, H, hd, seed=13)
    zero = torch.zeros(H)
    ref = R.alibi_attention_ref(*_qkv(x, D), zero, B, T, H, hd, 1.0)
    hi, lo = _run_attention(dev, x, zero, B, T, H, hd)
    assert_close(_planes(hi, lo), ref, 2e-6, f"zero slopes hd={hd}")
    rh, rl = _ops().rope_attention(x.to(dev), torch.ones(T, hd // 2, device=dev), torch.zeros(T, hd // 2, device=dev), B, T, H, hd, 1.0)
    assert torch.equal(hi, rh) and torch.equal(lo, rl)
    moved = rel_err(_planes(*_run_attention(dev, x, R.hf_slopes(H), B, T, H, hd)), ref)[0]
    assert moved > 1e-2, f"BLOOM's slopes change nothing ({moved:.1e}): the bias is not applied"


# ------------------------------------------------------------------------------------------------------------ mer_layernorm_row
def _norm_inputs(M, D, seed=3):
    """tests/test_llama_gpu.py's rows and gains, and a bias."""
    g = torch.Generator().manual_seed(seed + D)
    return torch.randn((M, D), generator=g) * 2.0 + 0.25, 1.0 + 0.3 * torch.randn((D,), generator=g), 0.3 * torch.randn((D,), generator=g)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", [4, 132, 256, 2048, 2052, 2560, 4096, 8192])
def test_layernorm_row_widths(dev, D, dtype):
    """Every width class (one float4 in one thread ... eight float4s in every thread, both sides of mer_layernorm's 2048) at M = 1, 3, 77,
    every subset of the outputs; for D <= 2048 mer_layernorm agrees within the bar."""
    ops = _ops()
    for M in (1, 3, 77):
        x, g, b = _norm_inputs(M, D)
        ref = R.layernorm_ref(x, g, b, EPS)
        xd, gd, bd = x.to(dev), g.to(dev), b.to(dev)
        o32, hi, lo = ops.layernorm_row(xd, gd, bd, EPS, out32=True, out16=True, out16_lo=True, dtype=dtype)
        e32, e16 = rel_err(o32, ref)[0], rel_err(_planes(hi, lo), ref)[0]
        if M == 77:
            print(f"layernorm_row D={D} {dtype}: fp32 {e32:.2e} planes {e16:.2e}")
        assert_close(o32, ref, 2e-6, f"layernorm_row fp32 M={M} D={D}")
        assert_close(_planes(hi, lo), ref, _plane_tol(2e-6, dtype), f"layernorm_row {dtype} hi+lo M={M} D={D}")
        assert torch.equal(hi, o32.to(_t16(dtype))), "hi is the fp32 result rounded once"
        assert torch.equal(lo, (o32 - hi.float()).to(_t16(dtype))), "lo is the rounded remainder"
        for want32, want16, wantlo in ((True, False, False), (False, True, False), (False, True, True), (True, True, False)):
            a32, ah, al = ops.layernorm_row(xd, gd, bd, EPS, out32=want32, out16=want16, out16_lo=wantlo, dtype=dtype)
            assert (a32 is None) == (not want32) and (ah is None) == (not want16) and (al is None) == (not wantlo)
            assert (a32 is None or torch.equal(a32, o32)) and (ah is None or torch.equal(ah, hi)) and (al is None or torch.equal(al, lo))
        if D <= 2048:
            old = ops.layernorm(xd, gd, bd, EPS)[0]
            e_old = rel_err(o32, old)[0]
            assert e_old <= 2e-6, f"mer_layernorm and mer_layernorm_row differ by {e_old:.2e} at M={M} D={D}"
    o32, hi, lo = ops.layernorm_row(xd, None, None, EPS, out16=True, out16_lo=True, dtype=dtype)       # gamma = beta = NULL: ones, zeros
    assert_close(o32, R.layernorm_ref(x, None, None, EPS), 2e-6, f"layernorm_row without gamma / beta D={D}")


@pytest.mark.parametrize("D", [132, 2560, 8192])
def test_layernorm_row_bits_do_not_depend_on_M(dev, D):
    """Row r at M = 1 against the same row inside M = 300, bit for bit."""
    ops = _ops()
    x, g, b = _norm_inputs(300, D)
    xd, gd, bd = x.to(dev), g.to(dev), b.to(dev)
    o32, hi, lo = ops.layernorm_row(xd, gd, bd, EPS, out16=True, out16_lo=True)
    for r in (0, 151, 299):
        a32, ah, al = ops.layernorm_row(xd[r:r + 1].contiguous(), gd, bd, EPS, out16=True, out16_lo=True)
        assert torch.equal(a32[0], o32[r]) and torch.equal(ah[0], hi[r]) and torch.equal(al[0], lo[r]), (D, r)


def test_layernorm_row_strided_rows_and_canaries(dev):
    """ldx = D + 4, ld32 = D + 8, ld16 = D + 12: NaN in the input gaps and in two spare rows must never be read, the canaries in the
    output gaps and spare rows must survive."""
    ops = _ops()
    M, D = 5, 2564
    x, g, b = _norm_inputs(M, D)
    xb = torch.full((M + 2, D + 4), float("nan"))
    xb[:M, :D] = x
    xd = xb.to(dev)
    o32 = torch.full((M + 2, D + 8), 12345.0, device=dev)
    hi = torch.full((M + 2, D + 12), 77.0, dtype=torch.float16, device=dev)
    lo = torch.full((M + 2, D + 12), 77.0, dtype=torch.float16, device=dev)
    ops.layernorm_row(xd, g.to(dev), b.to(dev), EPS, M=M, D=D, ldx=D + 4, out=(o32[:M, :D], hi[:M, :D], lo[:M, :D]))
    ref = R.layernorm_ref(x, g, b, EPS)
    assert_close(o32[:M, :D], ref, 2e-6, "strided layernorm_row fp32")
    assert_close(_planes(hi[:M, :D], lo[:M, :D]), ref, 2e-6, "strided layernorm_row planes")
    dense = ops.layernorm_row(x.to(dev), g.to(dev), b.to(dev), EPS, out16=True, out16_lo=True)
    assert torch.equal(o32[:M, :D], dense[0]) and torch.equal(hi[:M, :D], dense[1]) and torch.equal(lo[:M, :D], dense[2])
    assert bool((o32[:M, D:] == 12345.0).all()) and bool((o32[M:] == 12345.0).all())
    for p in (hi, lo):
        assert bool((p[:M, D:] == 77.0).all()) and bool((p[M:] == 77.0).all())


@pytest.mark.parametrize("D", [132, 2560, 8192])
def test_layernorm_row_constant_and_offset_rows(dev, D):
    """A constant row has variance 0: the centred values are exact zeros and the output is beta, bit for bit.  Rows of unit spread
    around 1e4 are held to bloom_refs.layernorm_bound (the error of the fp32 mean, carried through the centred second pass), which a
    one-pass E[x^2] - E[x]^2 misses by five orders of magnitude (tests/test_bloom_cpu.py)."""
    ops = _ops()
    _, g, b = _norm_inputs(1, D)
    x = torch.full((3, D), 3.0)
    x[1] = -0.25
    x[2] = 1024.0
    o32, hi, lo = ops.layernorm_row(x.to(dev), g.to(dev), b.to(dev), EPS, out16=True, out16_lo=True)
    assert torch.equal(o32.cpu(), b[None].expand(3, D)), "constant rows: output = beta"
    assert torch.equal(hi, o32.half()) and bool(torch.isfinite(lo.float()).all())
    gen = torch.Generator().manual_seed(D)
    x = torch.randn((4, D), generator=gen) + 1e4
    ref, bound = R.layernorm_ref(x, g, b, EPS), R.layernorm_bound(x, g, b, EPS)
    o32 = ops.layernorm_row(x.to(dev), g.to(dev), b.to(dev), EPS)[0]
    assert bool(torch.isfinite(o32).all())
    w = worst_ratio(o32, ref, bound)
    w32 = worst_ratio(torch.nn.functional.layer_norm(x, (D,), g, b, EPS), ref, bound)
    wrong = worst_ratio(R.layernorm_one_pass32(x, g, b, EPS), ref, bound)
    print(f"layernorm_row offset rows D={D}: at {w:.3f} of the bound (torch fp32 on the CPU {w32:.3f}, one-pass variance {wrong:.1e}), "
          f"max-norm {rel_err(o32, ref)[0]:.2e}")
    assert w32 <= 1.0 and wrong >= 100.0 and w <= 1.0


# ------------------------------------------------------------------------------------------------------------------- the model
def _references(m, ids):
    refs = []
    for b, n in enumerate(R.LENGTHS):
        hs = [h[0] for h in R.hf_hidden_states(m, ids[b:b + 1, :n])]                 # the sentence alone, as the reference runs it
        fr = torch.stack(hs)[[-4, -3, -2, -1]].sum(0)
        refs.append(dict(hs=hs, frame=fr, utt=fr.mean(0)))
    return refs


@pytest.fixture(scope="module", params=sorted(R.TINY))
def tiny(request):
    """(name, HF module, ids [3, 17], per-sentence HF references): computed once per model."""
    m = R.tiny_bloom(request.param)
    ids = R.batch_ids()
    return request.param, m, ids, _references(m, ids)


def _model_errors(model, ids, refs):
    """-> (hidden states, FRAME, UTT) max-norm errors over the valid rows, each sentence run alone (lengths 17, 9, 1) through
    forward_raw / extract_utterance.  No special token is sliced off: BLOOM's tokenizer adds none."""
    hs_rows, fr_rows, utt_rows = [], [], []
    for b, n in enumerate(R.LENGTHS):
        one = ids[b:b + 1, :n].contiguous()
        hs, fr, _ = model.forward_raw(one, lengths=[n], hidden_states=True, frames=True)
        utt_rows.append(model.extract_utterance(one, [n], 0, None)[0])
        hs_rows.append(hs[:, 0])
        fr_rows.append(fr)
    torch.cuda.synchronize()
    e_hs = max(rel_err(torch.cat([h[i] for h in hs_rows]), torch.cat([r["hs"][i] for r in refs]))[0] for i in range(hs_rows[0].shape[0]))
    e_fr = rel_err(torch.cat(fr_rows), torch.cat([r["frame"] for r in refs]))[0]
    e_utt = rel_err(torch.stack(utt_rows), torch.stack([r["utt"] for r in refs]))[0]
    return e_hs, e_fr, e_utt


@pytest.fixture(scope="module")
def ladder(dev):
    """{model name: {preset: (hidden states, FRAME, UTT)}} for every tiny model under every preset: measured once, printed."""
    from mertools_amd.bloom import LADDER, HipBloomModel
    got = {}
    for name in sorted(R.TINY):
        m, ids = R.tiny_bloom(name), R.batch_ids()
        refs = _references(m, ids)
        got[name] = {p: _model_errors(HipBloomModel.from_hf(m, device=dev, precision=p), ids, refs) for p in LADDER}
        for p in LADDER:
            e = got[name][p]
            print(f"bloom [{name}] {p:9s}: hidden states {e[0]:.2e}  FRAME {e[1]:.2e}  UTT {e[2]:.2e}")
    return got


def test_model_matches_hf_under_the_default_preset(dev, ladder, tiny):
    from mertools_amd.bloom import DEFAULT_PRECISION, HipBloomModel
    name, m, ids, refs = tiny
    e_hs, e_fr, e_utt = ladder[name][DEFAULT_PRECISION]
    assert e_fr <= 8e-4 and e_utt <= 8e-4, f"default preset {DEFAULT_PRECISION}: FRAME {e_fr:.2e} UTT {e_utt:.2e} > 8e-4"
    assert e_hs <= 1e-3
    assert _model_errors(HipBloomModel.from_hf(m, device=dev), ids, refs) == (e_hs, e_fr, e_utt)      # the constructor's own default


def test_default_preset_is_the_cheapest_that_holds_the_bars(ladder):
    """The rule: the first preset of the ladder (cheapest first) that stays <= 8e-4 on the UTT and FRAME features and <= 1e-3 on every
    hidden state, on every test model."""
    from mertools_amd.bloom import DEFAULT_PRECISION, LADDER
    feat = {p: max(max(ladder[n][p][1:]) for n in ladder) for p in LADDER}
    hid = {p: max(ladder[n][p][0] for n in ladder) for p in LADDER}
    print("bloom ladder, worst over the tiny models (UTT / FRAME | hidden states): " + "  ".join(f"{p} {feat[p]:.2e} | {hid[p]:.2e}" for p in LADDER))
    holds = [p for p in LADDER if feat[p] <= 8e-4 and hid[p] <= 1e-3]
    assert holds and holds[0] == DEFAULT_PRECISION, (holds, DEFAULT_PRECISION)


def test_model_call_and_hidden_states(dev, tiny):
    """__call__ (the HF-style surface the driver's probe uses): hidden_states tuple, hidden_states[0] = the embedding LayerNorm's
    output, last_hidden_state = ln_f's output; .half() is refused."""
    from mertools_amd._lib import MerError
    from mertools_amd.bloom import HipBloomModel
    name, m, ids, refs = tiny
    model = HipBloomModel.from_hf(m, device=dev)
    assert model.to(dev) is model and model.cuda() is model and model.eval() is model
    with pytest.raises(MerError):
        model.half()
    mask = (torch.arange(ids.shape[1])[None] < torch.tensor(R.LENGTHS)[:, None]).long()
    out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    assert len(out.hidden_states) == m.config.n_layer + 1 and out.hidden_states[0].shape == (3, 17, m.config.hidden_size)
    assert torch.equal(out.last_hidden_state, out.hidden_states[-1])
    valid = lambda t: torch.cat([t[b, :n] for b, n in enumerate(R.LENGTHS)])
    assert_close(valid(out.last_hidden_state), torch.cat([r["hs"][-1] for r in refs]), 1e-3, f"last_hidden_state [{name}]")
    assert_close(valid(out.hidden_states[0]), torch.cat([r["hs"][0] for r in refs]), 2e-6, f"hidden_states[0] [{name}]")
    assert model(input_ids=ids).hidden_states is None
    with pytest.raises(MerError):
        model(input_ids=ids, attention_mask=mask.flip(1))


def test_a_sentence_is_a_function_of_the_sentence(dev, tiny):
    """Per clip, bit for bit: one batch of 3 == each sentence alone == the batch padded to T = 33; from_hf == the constructor."""
    from mertools_amd.bloom import HipBloomModel
    name, m, ids, _ = tiny
    model = HipBloomModel.from_hf(m, device=dev)
    twin = HipBloomModel(m.state_dict(), m.config, device=dev)
    lens = list(R.LENGTHS)

    def run(mod, x, ln):
        B, T = x.shape
        hs, fr, _ = mod.forward_raw(x, lengths=ln, hidden_states=True, frames=True)
        return hs, fr.view(B, T, -1), mod.extract_utterance(x, ln, 0, None)
    hs, fr, utt = run(model, ids, lens)
    hs2, fr2, utt2 = run(twin, ids, lens)
    assert torch.equal(hs, hs2) and torch.equal(fr, fr2) and torch.equal(utt, utt2)
    wide = torch.zeros((3, 33), dtype=torch.int64)
    wide[:, :17] = ids
    hs3, fr3, utt3 = run(model, wide, lens)
    for b, n in enumerate(lens):
        h1, f1, u1 = run(model, ids[b:b + 1, :n].contiguous(), [n])
        for other_hs, other_fr, other_utt, row in ((h1, f1, u1, 0), (hs3, fr3, utt3, b)):
            assert torch.equal(other_hs[:, row, :n], hs[:, b, :n]), (name, b)
            assert torch.equal(other_fr[row, :n], fr[b, :n]), (name, b)
            assert torch.equal(other_utt[row], utt[b]), (name, b)


# ------------------------------------------------------------------------------------------------------------------ the driver
CHARS = list(dict.fromkeys("今天气真好我很开心难过生惊讶害怕的了是不你他她们这那有没在和也都就要会可以说看想"))


def _bloom_checkpoint(d):
    """save_pretrained of a tiny model + a character-level PreTrainedTokenizerFast that adds no special token (BLOOM's adds none)."""
    from tokenizers import Regex, Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    vocab = {t: i for i, t in enumerate(["<pad>", "<s>", "</s>", "<unk>"] + CHARS)}
    assert len(vocab) <= R.VOCAB
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.Split(Regex("."), behavior="isolated")
    PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>").save_pretrained(d)
    R.tiny_bloom("h192x3").save_pretrained(d)


def _files(root):
    (d,) = glob.glob(os.path.join(root, "*"))
    return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_text_driver_on_a_bloom_checkpoint_directory(dev, tmp_path):
    import pandas as pd
    import transformers as tr
    from mertools_amd.extract import text
    d = str(tmp_path / "tools" / "bloom-tiny")
    os.makedirs(d)
    _bloom_checkpoint(d)
    rng = np.random.RandomState(4)
    names = [f"s{i}" for i in range(12)]
    sents = ["".join(rng.choice(CHARS, size=n)) for n in (5, 12, 30, 0, 8, 19, 1, 25, 3, 16, 17, 2)]
    csv = str(tmp_path / "trans.csv")
    pd.DataFrame({"name": names, "chinese": sents, "english": ["x"] * 12}).to_csv(csv, index=False)
    tok = tr.AutoTokenizer.from_pretrained(d, use_fast=False)
    assert text.find_start_end_pos(tok) == (0, None)
    ref_model = tr.AutoModel.from_pretrained(d, attn_implementation="eager").eval()
    assert type(ref_model).__name__ == "BloomModel"
    Dm = ref_model.config.hidden_size
    for level in ("UTTERANCE", "FRAME"):
        text.extract_embedding("bloom-tiny", csv, str(tmp_path / f"b4-{level}"), level, gpu=0, model_dir=d, batch_size=4)
        text.extract_embedding("bloom-tiny", csv, str(tmp_path / f"b1-{level}"), level, gpu=0, model_dir=d, batch_size=1)
        f4, f1 = _files(str(tmp_path / f"b4-{level}")), _files(str(tmp_path / f"b1-{level}"))
        assert sorted(f4) == sorted(f"{n}.npy" for n in names) and f4 == f1, "files differ between batch_size 4 and 1"
        (save_dir,) = glob.glob(str(tmp_path / f"b4-{level}" / "*"))
        worst = 0.0
        for n, s in zip(names, sents):
            out = np.load(os.path.join(save_dir, f"{n}.npy"))
            if not s:                                              # reference :235-249: an empty sentence is float64 zeros
                assert out.dtype == np.float64 and out.shape == ((Dm,) if level == "UTTERANCE" else (1, Dm)) and not out.any()
                continue
            enc = tok(s, return_tensors="pt")
            assert enc["input_ids"].shape[1] == len(s)
            with torch.no_grad():
                feat = torch.stack(ref_model(**enc, output_hidden_states=True).hidden_states)[[-4, -3, -2, -1]].sum(0)[0].numpy()   # :225-231
            ref = feat.mean(0) if level == "UTTERANCE" else feat
            assert out.shape == ref.shape, (n, out.shape, ref.shape)
            worst = max(worst, rel_err(torch.from_numpy(out).float(), torch.from_numpy(ref))[0])
        print(f"bloom text driver [{level}]: worst sentence {worst:.2e}")
        assert worst <= 1e-3


def test_bert_checkpoint_directory_still_takes_its_own_path(dev, tmp_path, monkeypatch):
    """The by-name driver on a BERT directory writes the bytes an injected HipBertModel writes: the dispatch on model_type leaves
    every other checkpoint on the path it had."""
    import pandas as pd
    import transformers as tr
    from mertools_amd import config
    from mertools_amd.encoders import HipBertModel
    from mertools_amd.extract import text
    torch.manual_seed(20261019)
    name = "bert-tiny-dir"
    root = tmp_path / "tools"
    d = root / "transformers" / name
    d.mkdir(parents=True)
    monkeypatch.setattr(config, "PATH_TO_PRETRAINED_MODELS", str(root))
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + CHARS
    (d / "vocab.txt").write_text("\n".join(vocab), encoding="utf-8")
    tr.BertTokenizer(str(d / "vocab.txt")).save_pretrained(str(d))
    tr.BertModel(tr.BertConfig(num_hidden_layers=4, hidden_size=128, num_attention_heads=2, intermediate_size=256, vocab_size=len(vocab),
                               attn_implementation="eager")).eval().save_pretrained(str(d))
    rng = np.random.RandomState(6)
    names = [f"s{i}" for i in range(5)]
    sents = ["".join(rng.choice(CHARS, size=n)) for n in (5, 12, 1, 8, 19)]
    csv = str(tmp_path / "trans.csv")
    pd.DataFrame({"name": names, "chinese": sents, "english": ["x"] * 5}).to_csv(csv, index=False)
    for level in ("UTTERANCE", "FRAME"):
        text.extract_embedding(name, csv, str(tmp_path / f"byname-{level}"), level, gpu=0, batch_size=3)
        model = HipBertModel.from_hf(tr.AutoModel.from_pretrained(str(d)), device="cuda:0")
        assert type(model) is HipBertModel
        tok = tr.AutoTokenizer.from_pretrained(str(d), use_fast=False)
        text.extract_embedding(name, csv, str(tmp_path / f"injected-{level}"), level, gpu=0, model=model, tokenizer=tok, batch_size=3)
        a, b = _files(str(tmp_path / f"byname-{level}")), _files(str(tmp_path / f"injected-{level}"))
        assert sorted(a) == sorted(f"{n}.npy" for n in names) and a == b
