"""LLaMA-family text encoder on the GPU: mer_rmsnorm and mer_rope_attention against float64 compositions (tests/llama_refs.py, shown to
be HF's formulas in tests/test_llama_cpu.py), HipLlamaModel against HF's fp32 LlamaModel on three tiny models, the by-name text driver
on a LLaMA checkpoint directory, and a BERT directory still taking its own path.

Bars.  mer_rmsnorm: mer_layernorm's (tests/test_rowops_gpu.py) — 2e-6 max-norm in fp32 and as f16 hi + lo planes, + 2^-16 (what a
bf16 pair carries) for bf16 planes.  mer_rope_attention: 2e-6 on hi + lo, the bar mer_small_attention is held to in
tests/test_whisper.py, on inputs where plain fp32 torch on the CPU sits within a quarter of it; under 30x larger q the elementwise
bound llama_refs.rope_attention_bound (+ what an f16 pair cannot carry: 2^-21 |ref| + 2^-24).  Model: 1e-3 on UTT and FRAME features
and on every hidden state under the default preset, 8e-4 (1e-3 less the 20 % margin of from_hf()'s ladder) on the features for the
preset that is the default, 3e-4 for `accurate` (tests/test_whisper.py's bar for its accurate encoder's output)."""
import glob
import os

import numpy as np
import pytest
import torch

import llama_refs as L
from op_refs import worst_ratio
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu

EPS = float(torch.tensor(1e-6, dtype=torch.float32))     # the value the kernel receives


def _ops():
    from mertools_amd import ops
    return ops


def _t16(dtype):
    return torch.float16 if dtype == "f16" else torch.bfloat16


def _plane_tol(tol, dtype):
    return tol if dtype == "f16" else tol + L.U2


def _planes(hi, lo):
    return hi.double().cpu() + (lo.double().cpu() if lo is not None else 0.0)


# ------------------------------------------------------------------------------------------------------------------ mer_rmsnorm
def _norm_inputs(M, D, seed=3):
    g = torch.Generator().manual_seed(seed + D)
    return torch.randn((M, D), generator=g) * 2.0 + 0.25, 1.0 + 0.3 * torch.randn((D,), generator=g)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", [4, 132, 256, 4096, 5120, 8192])
def test_rmsnorm_widths(dev, D, dtype):
    """Every width class (one float4 in one thread ... eight float4s in every thread) at M = 1, 3, 77, every subset of the outputs."""
    ops = _ops()
    for M in (1, 3, 77):
        x, g = _norm_inputs(M, D)
        ref = L.rmsnorm_ref(x, g, EPS)
        xd, gd = x.to(dev), g.to(dev)
        o32, hi, lo = ops.rmsnorm(xd, gd, EPS, out32=True, out16=True, out16_lo=True, dtype=dtype)
        e32 = assert_close(o32, ref, 2e-6, f"rmsnorm fp32 M={M} D={D}")
        e16 = assert_close(_planes(hi, lo), ref, _plane_tol(2e-6, dtype), f"rmsnorm {dtype} hi+lo M={M} D={D}")
        assert torch.equal(hi, o32.to(_t16(dtype))), "hi is the fp32 result rounded once"
        assert torch.equal(lo, (o32 - hi.float()).to(_t16(dtype))), "lo is the rounded remainder"
        for want32, want16, wantlo in ((True, False, False), (False, True, False), (False, True, True), (True, True, False)):
            a32, ah, al = ops.rmsnorm(xd, gd, EPS, out32=want32, out16=want16, out16_lo=wantlo, dtype=dtype)
            assert (a32 is None) == (not want32) and (ah is None) == (not want16) and (al is None) == (not wantlo)
            assert (a32 is None or torch.equal(a32, o32)) and (ah is None or torch.equal(ah, hi)) and (al is None or torch.equal(al, lo))
        if M == 77:
            print(f"rmsnorm D={D} {dtype}: fp32 {e32:.2e} planes {e16:.2e}")
            for r in (0, 40, 76):      # row r's bits at M = 1 and inside M = 77
                b32, bh, bl = ops.rmsnorm(xd[r:r + 1].contiguous(), gd, EPS, out32=True, out16=True, out16_lo=True, dtype=dtype)
                assert torch.equal(b32[0], o32[r]) and torch.equal(bh[0], hi[r]) and torch.equal(bl[0], lo[r]), (D, r)


def test_rmsnorm_strided_rows_and_canaries(dev):
    """ldx = D + 4, ld32 = D + 8, ld16 = D + 12: NaN in the input gaps and in two spare rows must never be read, the canaries in the
    output gaps and spare rows must survive."""
    ops = _ops()
    M, D = 5, 132
    x, g = _norm_inputs(M, D)
    xb = torch.full((M + 2, D + 4), float("nan"))
    xb[:M, :D] = x
    xd = xb.to(dev)
    o32 = torch.full((M + 2, D + 8), 12345.0, device=dev)
    hi = torch.full((M + 2, D + 12), 77.0, dtype=torch.float16, device=dev)
    lo = torch.full((M + 2, D + 12), 77.0, dtype=torch.float16, device=dev)
    ops.rmsnorm(xd, g.to(dev), EPS, M=M, D=D, ldx=D + 4, out=(o32[:M, :D], hi[:M, :D], lo[:M, :D]))
    ref = L.rmsnorm_ref(x, g, EPS)
    assert_close(o32[:M, :D], ref, 2e-6, "strided rmsnorm fp32")
    assert_close(_planes(hi[:M, :D], lo[:M, :D]), ref, 2e-6, "strided rmsnorm planes")
    dense = ops.rmsnorm(x.to(dev), g.to(dev), EPS, out16=True, out16_lo=True)
    assert torch.equal(o32[:M, :D], dense[0]) and torch.equal(hi[:M, :D], dense[1]) and torch.equal(lo[:M, :D], dense[2])
    assert bool((o32[:M, D:] == 12345.0).all()) and bool((o32[M:] == 12345.0).all())
    for p in (hi, lo):
        assert bool((p[:M, D:] == 77.0).all()) and bool((p[M:] == 77.0).all())


@pytest.mark.parametrize("D", [256, 8192])
def test_rmsnorm_without_gamma_zero_row_and_scales(dev, D):
    """gamma = NULL is ones; a row of zeros gives zeros (rsqrt(eps) is finite); rows 1e4 and 1e-4 times larger hold the bar — the sum of
    squares of |x| ~ 3e4 over 8192 columns (7e12) is far inside fp32, and squares of 1e-4 (1e-8) far above its subnormals."""
    ops = _ops()
    x, g = _norm_inputs(6, D)
    x[1] = 0.0
    x[2] *= 1e4
    x[3] *= 1e-4
    x[4] = 3e4 * torch.sign(x[4])
    for gamma in (None, g):
        ref = L.rmsnorm_ref(x, gamma, EPS)
        o32, hi, lo = ops.rmsnorm(x.to(dev), gamma.to(dev) if gamma is not None else None, EPS, out16=True, out16_lo=True)
        for r in range(6):          # row by row: each row is judged at its own magnitude
            if r != 1:
                assert_close(o32[r], ref[r], 2e-6, f"rmsnorm row {r} D={D}")
                assert_close(_planes(hi[r], lo[r]), ref[r], 2e-6, f"rmsnorm planes row {r} D={D}")
        assert bool((o32[1] == 0).all()) and bool((hi[1] == 0).all()) and bool((lo[1] == 0).all())
        assert bool(torch.isfinite(o32).all())


# ----------------------------------------------------------------------------------------------------------- mer_rope_attention
ATT_SHAPES = [(1, 1, 1, 64), (2, 5, 2, 128), (3, 17, 2, 128), (2, 65, 3, 64), (1, 64, 1, 128), (1, 257, 2, 128), (1, 2048, 1, 128)]


def _run_attention(dev, x, cos, sin, B, T, H, hd, dtype="f16", out_lo=True):
    hi, lo = _ops().rope_attention(x.to(dev), cos.to(dev), sin.to(dev), B, T, H, hd, 1.0, out_lo=out_lo, dtype=dtype)
    torch.cuda.synchronize()
    return hi, lo


def _qkv(x, D):
    return x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D]


@pytest.mark.parametrize("shape", ATT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope_attention_matches_float64(dev, shape):
    B, T, H, hd = shape
    D = H * hd
    ld_extra = 8 if T in (5, 65, 257) else 0            # ld > 3 H head_dim
    x = L.attention_inputs(B, T, H, hd, seed=11 + T, ld_extra=ld_extra)
    cos, sin = L.rope_tables(T, hd)
    ref = L.rope_attention_ref(*_qkv(x, D), cos, sin, B, T, H, hd, 1.0)
    cpu32 = rel_err(L.rope_attention_ref(*_qkv(x, D), cos, sin, B, T, H, hd, 1.0, dtype=torch.float32), ref)[0]
    assert cpu32 <= 0.5e-6, f"plain fp32 torch is at {cpu32:.2e} on these inputs: change the inputs, not the bar"
    for dtype in ("f16", "bf16"):
        hi, lo = _run_attention(dev, x, cos, sin, B, T, H, hd, dtype)
        e = assert_close(_planes(hi, lo), ref, _plane_tol(2e-6, dtype), f"rope_attention {shape} {dtype}")
        print(f"rope_attention {shape} {dtype}: {e:.2e} (torch fp32 on the CPU {cpu32:.2e})")
        hi1, lo1 = _run_attention(dev, x, cos, sin, B, T, H, hd, dtype)
        assert torch.equal(hi, hi1) and torch.equal(lo, lo1), "two runs on the same inputs differ"
        hi_only, none = _run_attention(dev, x, cos, sin, B, T, H, hd, dtype, out_lo=False)
        assert none is None and torch.equal(hi_only, hi)
    # 30x larger q: near-one-hot softmax, finite, inside the elementwise bound of the fp32 chain
    x30 = L.attention_inputs(B, T, H, hd, seed=11 + T, ld_extra=ld_extra, q_gain=30.0)
    ref30 = L.rope_attention_ref(*_qkv(x30, D), cos, sin, B, T, H, hd, 1.0)
    bound = L.rope_attention_bound(*_qkv(x30, D), cos, sin, B, T, H, hd, 1.0) + ref30.abs() * 2.0 ** -21 + 2.0 ** -24
    hi, lo = _run_attention(dev, x30, cos, sin, B, T, H, hd)
    assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isfinite(lo.float()).all())
    w = worst_ratio(_planes(hi, lo), ref30, bound)
    w32 = worst_ratio(L.rope_attention_ref(*_qkv(x30, D), cos, sin, B, T, H, hd, 1.0, dtype=torch.float32), ref30, bound)
    print(f"rope_attention {shape} q x30: at {w:.3f} of the bound (torch fp32 on the CPU {w32:.3f}), max-norm {rel_err(_planes(hi, lo), ref30)[0]:.2e}")
    assert w32 <= 1.0 and w <= 1.0


def test_rope_attention_rows_do_not_depend_on_the_batch_or_the_padding(dev):
    """Row (b, t) of a (3, 17) call equals, bit for bit, sentence b run alone at T = 9 and at T = 17."""
    B, T, H, hd = 3, 17, 2, 128
    x = L.attention_inputs(B, T, H, hd, seed=5)
    cos, sin = L.rope_tables(T, hd)
    hi, lo = _run_attention(dev, x, cos, sin, B, T, H, hd)
    hi, lo = hi.view(B, T, -1), lo.view(B, T, -1)
    for b in range(B):
        for n in (9, 17):
            xs = x.view(B, T, -1)[b, :n].contiguous()
            h1, l1 = _run_attention(dev, xs, cos, sin, 1, n, H, hd)
            assert float((h1.float() - hi[b, :n].float()).abs().max()) == 0.0 and float((l1.float() - lo[b, :n].float()).abs().max()) == 0.0, (b, n)


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_attention_is_causal(dev, hd):
    """Key t + 1 (its q, k and v) filled with 1e30 does not change row t's bits, nor any row before it."""
    B, T, H = 2, 40, 2
    x = L.attention_inputs(B, T, H, hd, seed=9)
    cos, sin = L.rope_tables(T, hd)
    hi, lo = _run_attention(dev, x, cos, sin, B, T, H, hd)
    for t in (0, 8, 15, 31, 38):
        y = x.clone()
        y.view(B, T, -1)[:, t + 1] = 1e30
        h1, l1 = _run_attention(dev, y, cos, sin, B, T, H, hd)
        assert torch.equal(h1.view(B, T, -1)[:, :t + 1], hi.view(B, T, -1)[:, :t + 1]) and torch.equal(l1.view(B, T, -1)[:, :t + 1], lo.view(B, T, -1)[:, :t + 1]), t


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_attention_position_zero_tables_give_plain_causal_attention(dev, hd):
    """cos = 1, sin = 0 (position 0 everywhere): mer_small_attention(causal=True) semantics, the float64 composition without rotation —
    the rotation, and only the rotation, depends on position."""
    B, T, H = 2, 37, 2
    D = H * hd
    x = L.attention_inputs(B, T, H, hd, seed=13)
    cos, sin = torch.ones(T, hd // 2), torch.zeros(T, hd // 2)
    ref = L.rope_attention_ref(*_qkv(x, D), cos, sin, B, T, H, hd, 1.0, rotary=False)
    hi, lo = _run_attention(dev, x, cos, sin, B, T, H, hd)
    assert_close(_planes(hi, lo), ref, 2e-6, f"position-0 tables hd={hd}")
    rc, rs = L.rope_tables(T, hd)
    moved = rel_err(_planes(*_run_attention(dev, x, rc, rs, B, T, H, hd)), ref)[0]
    assert moved > 1e-2, f"real tables change nothing ({moved:.1e}): the rotation is not applied"


# ------------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module", params=sorted(L.TINY))
def tiny(request):
    """(name, HF module, ids [3, 17], per-sentence HF references): computed once per model."""
    m = L.tiny_llama(request.param)
    ids = L.batch_ids()
    refs = []
    for b, n in enumerate(L.LENGTHS):
        hs = [h[0] for h in L.hf_hidden_states(m, ids[b:b + 1, :n])]                 # the sentence alone, as the reference runs it
        fr = torch.stack(hs)[[-4, -3, -2, -1]].sum(0)
        refs.append(dict(hs=hs, frame=fr, utt=fr[1:].mean(0) if n > 1 else None))
    return request.param, m, ids, refs


def _model_errors(model, ids, refs):
    """-> (hidden states, FRAME, UTT) max-norm errors over the valid rows of the batch, through forward_raw / extract_utterance."""
    B, T = ids.shape
    hs, fr, _ = model.forward_raw(ids, lengths=list(L.LENGTHS), hidden_states=True, frames=True)
    utt = model.extract_utterance(ids, list(L.LENGTHS), 1, None)
    torch.cuda.synchronize()
    fr = fr.view(B, T, -1)
    e_hs = max(rel_err(torch.cat([hs[i, b, :n] for b, n in enumerate(L.LENGTHS)]), torch.cat([r["hs"][i] for r in refs]))[0] for i in range(hs.shape[0]))
    e_fr = rel_err(torch.cat([fr[b, :n] for b, n in enumerate(L.LENGTHS)]), torch.cat([r["frame"] for r in refs]))[0]
    rows = [b for b, r in enumerate(refs) if r["utt"] is not None]
    e_utt = rel_err(utt[rows], torch.stack([refs[b]["utt"] for b in rows]))[0]
    return e_hs, e_fr, e_utt


def test_model_matches_hf_under_every_preset(dev, tiny):
    from mertools_amd.llama import DEFAULT_PRECISION, LADDER, HipLlamaModel
    name, m, ids, refs = tiny
    got = {}
    for precision in LADDER:
        got[precision] = _model_errors(HipLlamaModel.from_hf(m, device=dev, precision=precision), ids, refs)
        print(f"llama [{name}] {precision:9s}: hidden states {got[precision][0]:.2e}  FRAME {got[precision][1]:.2e}  UTT {got[precision][2]:.2e}")
    e_hs, e_fr, e_utt = got[DEFAULT_PRECISION]
    assert e_fr <= 8e-4 and e_utt <= 8e-4, f"default preset {DEFAULT_PRECISION}: FRAME {e_fr:.2e} UTT {e_utt:.2e} > 8e-4"
    assert e_hs <= 1e-3
    assert got["accurate"][1] <= 3e-4 and got["accurate"][2] <= 3e-4, got["accurate"]
    e_hs, e_fr, e_utt = _model_errors(HipLlamaModel.from_hf(m, device=dev), ids, refs)      # the constructor's own default
    assert (e_hs, e_fr, e_utt) == got[DEFAULT_PRECISION]


def test_default_preset_is_the_cheapest_that_holds_the_bars(dev):
    """The rule: the first preset of the ladder (cheapest first) that stays <= 8e-4 on the UTT and FRAME features and <= 1e-3 on every
    hidden state, on every test model — i.e. the cheapest one that passes test_model_matches_hf_under_every_preset as the default."""
    from mertools_amd.llama import DEFAULT_PRECISION, LADDER, HipLlamaModel
    feat, hid = {p: 0.0 for p in LADDER}, {p: 0.0 for p in LADDER}
    for name in sorted(L.TINY):
        m, ids = L.tiny_llama(name), L.batch_ids()
        refs = []
        for b, n in enumerate(L.LENGTHS):
            hs = [h[0] for h in L.hf_hidden_states(m, ids[b:b + 1, :n])]
            fr = torch.stack(hs)[[-4, -3, -2, -1]].sum(0)
            refs.append(dict(hs=hs, frame=fr, utt=fr[1:].mean(0) if n > 1 else None))
        for p in LADDER:
            e_hs, e_fr, e_utt = _model_errors(HipLlamaModel.from_hf(m, device=dev, precision=p), ids, refs)
            feat[p], hid[p] = max(feat[p], e_fr, e_utt), max(hid[p], e_hs)
    print("llama ladder, worst over the three models (UTT / FRAME | hidden states): " + "  ".join(f"{p} {feat[p]:.2e} | {hid[p]:.2e}" for p in LADDER))
    holds = [p for p in LADDER if feat[p] <= 8e-4 and hid[p] <= 1e-3]
    assert holds and holds[0] == DEFAULT_PRECISION, (holds, DEFAULT_PRECISION)


def test_model_call_and_hidden_states(dev, tiny):
    """__call__ (the HF-style surface the driver's probe uses): hidden_states tuple, last_hidden_state = the final norm's output."""
    from mertools_amd.llama import HipLlamaModel
    name, m, ids, refs = tiny
    model = HipLlamaModel.from_hf(m, device=dev)
    mask = (torch.arange(ids.shape[1])[None] < torch.tensor(L.LENGTHS)[:, None]).long()
    out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    assert len(out.hidden_states) == m.config.num_hidden_layers + 1 and out.hidden_states[0].shape == (3, 17, m.config.hidden_size)
    assert torch.equal(out.last_hidden_state, out.hidden_states[-1])
    for b, n in enumerate(L.LENGTHS):
        assert_close(out.last_hidden_state[b, :n], refs[b]["hs"][-1], 1e-3, f"last_hidden_state [{name}] sentence {b}")
        assert torch.equal(out.hidden_states[0][b, :n].cpu(), m.embed_tokens.weight[ids[b, :n]]), "hidden_states[0] is the embedding rows"
    assert model(input_ids=ids).hidden_states is None
    from mertools_amd._lib import MerError
    with pytest.raises(MerError):
        model(input_ids=ids, attention_mask=mask.flip(1))


def test_a_sentence_is_a_function_of_the_sentence(dev, tiny):
    """Per clip, bit for bit: one batch of 3 == each sentence alone == the batch padded to T = 33; from_hf == the constructor."""
    from mertools_amd.llama import HipLlamaModel
    name, m, ids, _ = tiny
    model = HipLlamaModel.from_hf(m, device=dev)
    twin = HipLlamaModel(m.state_dict(), m.config, device=dev)
    lens = list(L.LENGTHS)

    def run(mod, x, ln):
        B, T = x.shape
        hs, fr, _ = mod.forward_raw(x, lengths=ln, hidden_states=True, frames=True)
        return hs, fr.view(B, T, -1), mod.extract_utterance(x, ln, 1, None)
    hs, fr, utt = run(model, ids, lens)
    hs2, fr2, utt2 = run(twin, ids, lens)
    assert torch.equal(hs, hs2) and torch.equal(fr, fr2) and torch.equal(utt[:2], utt2[:2])
    wide = torch.zeros((3, 33), dtype=torch.int64)
    wide[:, :17] = ids
    hs3, fr3, utt3 = run(model, wide, lens)
    for b, n in enumerate(lens):
        h1, f1, u1 = run(model, ids[b:b + 1, :n].contiguous(), [n])
        for other_hs, other_fr, other_utt, row in ((h1, f1, u1, 0), (hs3, fr3, utt3, b)):
            assert float((other_hs[:, row, :n] - hs[:, b, :n]).abs().max()) == 0.0, (name, b)
            assert float((other_fr[row, :n] - fr[b, :n]).abs().max()) == 0.0, (name, b)
            if n > 1:
                assert float((other_utt[row] - utt[b]).abs().max()) == 0.0, (name, b)


# ------------------------------------------------------------------------------------------------------------------ the driver
CHARS = list(dict.fromkeys("今天气真好我很开心难过生惊讶害怕的了是不你他她们这那有没在和也都就要会可以说看想"))


def _llama_checkpoint(d):
    """save_pretrained of the tiny model + a character-level PreTrainedTokenizerFast ("<s> $A") in directory d."""
    from tokenizers import Regex, Tokenizer, models, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    vocab = {t: i for i, t in enumerate(["<pad>", "<s>", "</s>", "<unk>"] + CHARS)}
    assert len(vocab) <= L.VOCAB
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.Split(Regex("."), behavior="isolated")
    tk.post_processor = processors.TemplateProcessing(single="<s> $A", special_tokens=[("<s>", 1)])
    PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>").save_pretrained(d)
    L.tiny_llama("hd128").save_pretrained(d)


def _files(root):
    (d,) = glob.glob(os.path.join(root, "*"))
    return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_text_driver_on_a_llama_checkpoint_directory(dev, tmp_path):
    import pandas as pd
    import transformers as tr
    from mertools_amd.extract import text
    d = str(tmp_path / "tools" / "llama-tiny")
    os.makedirs(d)
    _llama_checkpoint(d)
    rng = np.random.RandomState(4)
    names = [f"s{i}" for i in range(12)]
    sents = ["".join(rng.choice(CHARS, size=n)) for n in (5, 12, 30, 0, 8, 19, 1, 25, 3, 16, 17, 2)]
    csv = str(tmp_path / "trans.csv")
    pd.DataFrame({"name": names, "chinese": sents, "english": ["x"] * 12}).to_csv(csv, index=False)
    tok = tr.AutoTokenizer.from_pretrained(d, use_fast=False)
    assert text.find_start_end_pos(tok) == (1, None)
    ref_model = tr.AutoModel.from_pretrained(d, attn_implementation="eager").eval()
    Dm = ref_model.config.hidden_size
    for level in ("UTTERANCE", "FRAME"):
        text.extract_embedding("llama-tiny", csv, str(tmp_path / f"b4-{level}"), level, gpu=0, model_dir=d, batch_size=4)
        text.extract_embedding("llama-tiny", csv, str(tmp_path / f"b1-{level}"), level, gpu=0, model_dir=d, batch_size=1)
        f4, f1 = _files(str(tmp_path / f"b4-{level}")), _files(str(tmp_path / f"b1-{level}"))
        assert sorted(f4) == sorted(f"{n}.npy" for n in names) and f4 == f1, "files differ between batch_size 4 and 1"
        (save_dir,) = glob.glob(str(tmp_path / f"b4-{level}" / "*"))
        worst = 0.0
        for n, s in zip(names, sents):
            out = np.load(os.path.join(save_dir, f"{n}.npy"))
            if not s:                                              # reference :235-249: an empty sentence is float64 zeros
                assert out.shape == ((Dm,) if level == "UTTERANCE" else (1, Dm)) and not out.any()
                continue
            enc = tok(s, return_tensors="pt")
            with torch.no_grad():
                feat = torch.stack(ref_model(**enc, output_hidden_states=True).hidden_states)[[-4, -3, -2, -1]].sum(0)[0, 1:].numpy()   # :225-231
            ref = feat.mean(0) if level == "UTTERANCE" else feat
            assert out.shape == ref.shape, (n, out.shape, ref.shape)
            worst = max(worst, rel_err(torch.from_numpy(out).float(), torch.from_numpy(ref))[0])
        print(f"llama text driver [{level}]: worst sentence {worst:.2e}")
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
