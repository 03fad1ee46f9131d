"""Reference formulas for the BLOOM text encoder (mertools_amd/bloom.py, csrc/decoder.hip): float64 torch compositions of HF's
BloomModel (modeling_bloom.py: LayerNorm, the head-interleaved query_key_value, build_alibi_tensor, eager attention, BloomGelu) and the
tiny test models.  tests/test_bloom_cpu.py shows that bloom_forward64 IS the HF module (<= 5e-6); the GPU tests lean on it.  The shared
helpers (ids, attention inputs, head views, HF calls) are tests/llama_refs.py's."""
import math

import torch

from llama_refs import LENGTHS, U2, U32, VOCAB, _heads, attention_inputs, batch_ids, hf_hidden_states, hf_sentence_features  # noqa: F401

# (hidden, heads, layers, apply_residual_connection_post_layernorm, outlier): head_dim 128, head_dim 64 with a head count that is no
# power of two, head_dim 64 with the post-LayerNorm residual, head_dim 128 with one dominating channel
TINY = {"h256x2": (256, 2, 5, False, False), "h192x3": (192, 3, 5, False, False), "h384x6post": (384, 6, 5, True, False),
        "outlier": (256, 2, 5, False, True)}
STEEPEST = 2.0 ** -0.25      # head 0 of a 32-head model (bloom-7b1): the steepest slope of the checkpoints this model is built for


def tiny_bloom(name, seed=20261019):
    """HF BloomModel (eager, fp32, CPU) with weights that bite, as llama_refs.tiny_llama makes them: LayerNorm gains 1 + 0.3 randn,
    every bias 0.3 randn, block matrices 3x HF's 0.02 init; `outlier`: embedding column 5 scaled by 300, so that one channel dominates
    the embedding LayerNorm's statistics."""
    import transformers as tr
    D, H, L, post, outlier = TINY[name]
    torch.manual_seed(seed)
    cfg = tr.BloomConfig(hidden_size=D, n_head=H, n_layer=L, vocab_size=VOCAB, apply_residual_connection_post_layernorm=post,
                         pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation="eager")
    m = tr.BloomModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                gain = n.endswith("weight")            # the only 1-D weights are LayerNorm gains
                p.copy_((1.0 if gain else 0.0) + 0.3 * torch.randn(p.shape, generator=g))
            elif n.startswith("h."):
                p.mul_(3.0)
        if outlier:
            m.word_embeddings.weight[:, 5] *= 300.0
    return m


def hf_slopes(H):
    """The slopes HF's build_alibi_tensor uses for H heads, read back from its output (position 1 of an unmasked sentence: slope * 1)."""
    from transformers.models.bloom.modeling_bloom import build_alibi_tensor
    return build_alibi_tensor(torch.ones((1, 2), dtype=torch.int64), H, torch.float32)[:, 0, 1].contiguous()


def layernorm_ref(x, gamma, beta, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    y = (x - mean) * torch.rsqrt((x - mean).pow(2).mean(-1, keepdim=True) + eps)
    if gamma is not None:
        y = y * gamma.double()
    return y + beta.double() if beta is not None else y


def layernorm_bound(x, gamma, beta, eps):
    """Elementwise bound on |layernorm_row_kernel - layernorm_ref(float64)| for rows whose mean dominates their spread (u = 2^-24).  The
    mean comes from n fp32 additions in sequence per lane slot (n = ceil(D / 1024) float4s per thread), 2 + 6 + 2 tree levels and the
    division: |d mean| <= (n + 11) u max|partial sum| / D <= (n + 11) u (|mean| + spread).  x - mean is then exact or one rounding of a
    small number, so the error of the mean shifts every centred value by d mean: |d out| <= |d mean| rstd |gamma|; the variance,
    rstd, the two products and the addition add the ordinary 2e-6 of the row's largest |out|."""
    x = x.double()
    D = x.shape[-1]
    n = math.ceil(D / 1024)
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    rstd = torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps)
    ref = layernorm_ref(x, gamma, beta, eps)
    g = gamma.double().abs() if gamma is not None else 1.0
    dmean = (n + 11) * U32 * (mean.abs() + c.abs().max(-1, keepdim=True).values)
    return dmean * rstd * g + 2e-6 * ref.abs().max(-1, keepdim=True).values


def layernorm_one_pass32(x, gamma, beta, eps):
    """The WRONG kernel in fp32: var = E[x^2] - E[x]^2 (clamped at 0).  The offset-row tests show it far outside the bound."""
    x = x.float()
    mean = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
    return (x - mean) * torch.rsqrt(var + eps) * gamma.float() + beta.float()


def _bias(slopes, T, dtype, relative):
    """[H, T, T]: slopes[h] * (j - t) (relative: what the kernel adds) or slopes[h] * j (absolute: what HF adds), in `dtype`."""
    j = torch.arange(T, dtype=dtype)
    pos = j[None, :] - j[:, None] if relative else j[None, :].expand(T, T)
    return slopes.to(dtype)[:, None, None] * pos[None]


def alibi_attention_ref(q, k, v, slopes, B, T, H, hd, scale, dtype=torch.float64, relative=True, v_shift=0):
    """q, k, v [B*T, H*hd], slopes fp32 [H] -> causal ALiBi attention [B*T, H*hd] computed in `dtype` (float64: the reference; float32:
    plain torch on the CPU, the yardstick of what fp32 arithmetic gives).  v_shift = 1: the WRONG kernel that pairs weight j with the
    next key's value row."""
    qh, kh, vh = (_heads(t.to(dtype), B, T, H, hd) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale + _bias(slopes, T, dtype, relative)[None]
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    if v_shift:
        vh = torch.roll(vh, -v_shift, dims=2)
    return (p @ vh).transpose(1, 2).reshape(B * T, H * hd)


def alibi_attention_bound(q, k, v, slopes, B, T, H, hd, scale):
    """llama_refs.rope_attention_bound with the rotation terms removed (q and k enter as they are: dq = dk = 0) and the bias added:
      score     s_j = rn(rn(dot) scale) + rn(slope (j - t)), rounded once more by the addition (j - t is exact):
                e_j = scale (hd / 4 + 2) u sum_d |q_d k_d| + u |dot_j scale| + u (|slope (j - t)| + |s_j|);   E = max_j e_j
    the weight, sum and output terms are that bound's, on the biased scores; times 1.01 for the second-order terms."""
    qh, kh, vh = (_heads(t.double(), B, T, H, hd) for t in (q, k, v))
    mask = torch.ones(T, T, dtype=torch.bool).triu(1)
    dot = (qh @ kh.transpose(-1, -2)) * scale
    bias = _bias(slopes, T, torch.float64, True)[None]
    s = dot + bias
    e = scale * (hd / 4 + 2) * U32 * (qh.abs() @ kh.abs().transpose(-1, -2)) + U32 * dot.abs() + U32 * (bias.abs() + s.abs())
    s = s.masked_fill(mask, float("-inf"))
    e = e.masked_fill(mask, 0.0)
    a = (s - s.max(-1, keepdim=True).values).masked_fill(mask, 0.0)
    tt = torch.arange(T, dtype=torch.float64)[:, None]
    n = torch.ceil((tt + 1) / 32)
    r = e + e.max(-1, keepdim=True).values + (2 * a.abs() + 4 + 6 * n) * U32
    p = torch.softmax(s, -1)
    out = p @ vh
    num = (p * (r + (tt + 1 + n + 2) * U32)) @ vh.abs()
    den = (p * r).sum(-1, keepdim=True) + (7 * n + 4) * U32
    return (1.01 * (num + out.abs() * den)).transpose(1, 2).reshape(B * T, H * hd)


def bloom_gelu64(x):
    return x * 0.5 * (1.0 + torch.tanh(0.79788456 * x * (1 + 0.044715 * x * x)))


def bloom_forward64(sd, cfg, ids):
    """HF BloomModel(...).hidden_states in float64 from the state dict: list of n_layer + 1 tensors [B, T, D]; causal mask only (right
    padding is never a visible key of a real token), position = token index, the bias in the kernel's relative form."""
    sd = {k: v.double() for k, v in sd.items()}
    B, T = ids.shape
    D, H = cfg.hidden_size, cfg.n_head
    hd = D // H
    eps, post = cfg.layer_norm_epsilon, cfg.apply_residual_connection_post_layernorm
    slopes = hf_slopes(H)
    ln = lambda x, p: layernorm_ref(x, sd[p + ".weight"], sd[p + ".bias"], eps)
    lin = lambda x, p: x @ sd[p + ".weight"].T + sd[p + ".bias"]
    x = ln(sd["word_embeddings.weight"][ids], "word_embeddings_layernorm")
    hs = [x]
    for l in range(cfg.n_layer):
        p = f"h.{l}."
        hN = ln(x, p + "input_layernorm")
        fused = lin(hN, p + "self_attention.query_key_value").reshape(B * T, H, 3, hd)       # HF: view(B, T, H, 3, hd)
        q, k, v = (fused[:, :, i].reshape(B * T, D) for i in range(3))
        ctx = alibi_attention_ref(q, k, v, slopes, B, T, H, hd, hd ** -0.5).reshape(B, T, D)
        x = (hN if post else x) + lin(ctx, p + "self_attention.dense")
        hN = ln(x, p + "post_attention_layernorm")
        x = (hN if post else x) + lin(bloom_gelu64(lin(hN, p + "mlp.dense_h_to_4h")), p + "mlp.dense_4h_to_h")
        hs.append(x)
    hs[-1] = ln(x, "ln_f")
    return hs
