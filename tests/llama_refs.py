"""Reference formulas for the LLaMA-family text encoder (mertools_amd/llama.py, csrc/decoder.hip): float64 torch compositions of
HF's LlamaModel (modeling_llama.py: LlamaRMSNorm, LlamaRotaryEmbedding, rotate_half / apply_rotary_pos_emb, eager attention, LlamaMLP)
and the tiny test models.  tests/test_llama_cpu.py shows that llama_forward64 IS the HF module (<= 5e-6); the GPU tests lean on it."""
import torch

U32 = 2.0 ** -24      # fp32 unit roundoff
U2 = 2.0 ** -16       # what a bf16 hi + lo pair carries

# (hidden, heads, intermediate, layers, outlier): head_dim 128, head_dim 64, head_dim 128 with one dominating channel
TINY = {"hd128": (256, 2, 688, 5, False), "hd64": (128, 2, 344, 5, False), "outlier": (256, 2, 688, 5, True)}
VOCAB = 96
LENGTHS = (17, 9, 1)


def tiny_llama(name, seed=20261019):
    """HF LlamaModel (eager, fp32, CPU) with weights that bite: norm gains 1 + 0.3 randn, block matrices 3x HF's 0.02 init (which
    would leave every block near the identity and hide a wrong one); `outlier`: embedding column 5 scaled by 300, so that one channel
    dominates every RMSNorm."""
    import transformers as tr
    D, H, F, L, outlier = TINY[name]
    torch.manual_seed(seed)
    cfg = tr.LlamaConfig(hidden_size=D, num_attention_heads=H, num_key_value_heads=H, intermediate_size=F, num_hidden_layers=L, vocab_size=VOCAB,
                         max_position_embeddings=2048, pad_token_id=0, bos_token_id=1, eos_token_id=2, attn_implementation="eager")
    m = tr.LlamaModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            elif "layers." in n:
                p.mul_(3.0)
        if outlier:
            m.embed_tokens.weight[:, 5] *= 300.0
    return m


def batch_ids(seed=7, lengths=LENGTHS, T=None, pad=0):
    """Right-padded [len(lengths), T] ids (T = the longest sentence unless given), real tokens in [3, VOCAB)."""
    g = torch.Generator().manual_seed(seed)
    T = T if T is not None else max(lengths)
    ids = torch.full((len(lengths), T), pad, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = torch.randint(3, VOCAB, (n,), generator=g)
    return ids


def rope_tables(T, head_dim, theta=10000.0):
    """fp32 (cos, sin) [T, head_dim / 2] exactly as LlamaRotaryEmbedding makes them (inv_freq and the angle in fp32)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float) / head_dim))
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def rotate(x, cos, sin):
    """x [..., T, hd] with tables [T, hd / 2] (any float dtype; computed in x's dtype): x cos + rotate_half(x) sin."""
    h = x.shape[-1] // 2
    c, s = torch.cat([cos, cos], -1).to(x.dtype), torch.cat([sin, sin], -1).to(x.dtype)
    return x * c + torch.cat([-x[..., h:], x[..., :h]], -1) * s


def rmsnorm_ref(x, gamma, eps):
    x = x.double()
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return y * gamma.double() if gamma is not None else y


def _heads(t, B, T, H, hd):
    return t.reshape(B, T, H, hd).transpose(1, 2)       # [B, H, T, hd]


def rope_attention_ref(q, k, v, cos, sin, B, T, H, hd, scale, dtype=torch.float64, rotary=True, v_shift=0):
    """q, k, v [B*T, H*hd] -> causal attention [B*T, H*hd] computed in `dtype` (float64: the reference; float32: plain torch on the CPU,
    the yardstick of what fp32 arithmetic gives).  The tables stay the fp32 ones.  v_shift = 1: the WRONG kernel that pairs weight j
    with the next key's value row (the bound tests show it far outside)."""
    qh, kh, vh = (_heads(t.to(dtype), B, T, H, hd) for t in (q, k, v))
    if rotary:
        qh, kh = rotate(qh, cos[:T], sin[:T]), rotate(kh, cos[:T], sin[:T])
    s = (qh @ kh.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    if v_shift:
        vh = torch.roll(vh, -v_shift, dims=2)
    return (p @ vh).transpose(1, 2).reshape(B * T, H * hd)


def rope_attention_bound(q, k, v, cos, sin, B, T, H, hd, scale):
    """Elementwise first-order bound on |rope_attention_kernel - rope_attention_ref(float64)| from the kernel's fp32 chain on THESE
    inputs (u = 2^-24; nothing here looks at a kernel's output):
      rotation  x' = rn(rn(x c) - rn(x2 s)):                      |dx'| <= u (|x c| + |x2 s| + |x'|)
      score     four chains of hd / 4 fused steps, two additions, the product with scale:
                e_j = scale ((hd / 4 + 2) u sum_d |q'_d k'_d| + sum_d (|dq'_d| |k'_d| + |q'_d| |dk'_d|)) + u |s_j|;   E = max_j e_j
      weight    expf(s_j - m_chunk) carried to the final maximum through one rescale factor expf(m_old - m_new) per 32-key chunk
                (n = ceil((t + 1) / 32) chunks; the maxima only grow, so the arguments add up to at most |s_j - max|):
                relative  r_j = e_j + E + (2 |s_j - max| + 4 + 6 n) u
      out_d     = (sum_j w_j v_jd) / (sum_j w_j): t + 1 fused steps and n rescales on the numerator; per chunk a 5-level tree, a
                product and an addition on the sum, the reciprocal and the final product:
                |d out_d| <= sum_j p_j |v_jd| (r_j + (t + 1 + n + 2) u)  +  |out_d| (sum_j p_j r_j + (7 n + 4) u),   p = softmax
    times 1.01 for the second-order terms."""
    qh, kh, vh = (_heads(t.double(), B, T, H, hd) for t in (q, k, v))
    c, s_ = torch.cat([cos[:T], cos[:T]], -1).double(), torch.cat([sin[:T], sin[:T]], -1).double()
    h = hd // 2

    def rot(x):
        a, b = x * c, torch.cat([-x[..., h:], x[..., :h]], -1) * s_
        return a + b, U32 * (a.abs() + b.abs() + (a + b).abs())
    qr, dq = rot(qh)
    kr, dk = rot(kh)
    mask = torch.ones(T, T, dtype=torch.bool).triu(1)
    s = (qr @ kr.transpose(-1, -2)) * scale
    e = scale * ((hd / 4 + 2) * U32 * (qr.abs() @ kr.abs().transpose(-1, -2)) + dq @ kr.abs().transpose(-1, -2) + qr.abs() @ dk.transpose(-1, -2)) + U32 * s.abs()
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


def attention_inputs(B, T, H, hd, seed, ld_extra=0, q_gain=1.0):
    """fp32 q | k | v rows [B*T, 3*H*hd + ld_extra] for scale = 1: q and k carry hd^-1/4 each, so the scores are O(1) as they are."""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    x = torch.randn((B * T, 3 * D + ld_extra), generator=g)
    x[:, :2 * D] *= hd ** -0.25
    x[:, :D] *= q_gain
    return x


def llama_forward64(sd, cfg, ids):
    """HF LlamaModel(...).hidden_states in float64 from the state dict: list of num_hidden_layers + 1 tensors [B, T, D]; causal mask
    only (right padding is never a visible key of a real token)."""
    sd = {k: v.double() for k, v in sd.items()}
    B, T = ids.shape
    D, H = cfg.hidden_size, cfg.num_attention_heads
    hd = D // H
    cos, sin = rope_tables(T, hd, cfg.rope_parameters["rope_theta"] if getattr(cfg, "rope_parameters", None) else cfg.rope_theta)
    eps = cfg.rms_norm_eps
    x = sd["embed_tokens.weight"][ids]
    hs = [x]
    for l in range(cfg.num_hidden_layers):
        p = f"layers.{l}."
        hN = rmsnorm_ref(x, sd[p + "input_layernorm.weight"], eps).reshape(B * T, D)
        q, k, v = (hN @ sd[p + f"self_attn.{n}_proj.weight"].T for n in "qkv")
        ctx = rope_attention_ref(q, k, v, cos, sin, B, T, H, hd, hd ** -0.5)
        x = x + (ctx @ sd[p + "self_attn.o_proj.weight"].T).reshape(B, T, D)
        hN = rmsnorm_ref(x, sd[p + "post_attention_layernorm.weight"], eps)
        gate, up = hN @ sd[p + "mlp.gate_proj.weight"].T, hN @ sd[p + "mlp.up_proj.weight"].T
        x = x + (torch.nn.functional.silu(gate) * up) @ sd[p + "mlp.down_proj.weight"].T
        hs.append(x)
    hs[-1] = rmsnorm_ref(x, sd["norm.weight"], eps)
    return hs


def hf_hidden_states(model, ids, attention_mask=None):
    with torch.no_grad():
        return model(input_ids=ids, attention_mask=attention_mask, output_hidden_states=True).hidden_states


def hf_sentence_features(model, ids_row, n, start=0, end=None):
    """The reference's per-sentence path (extract_text_huggingface.py:216-249) on the fp32 HF module: the sentence alone, last-4 sum,
    special tokens sliced off -> (FRAME [n', D], UTTERANCE [D])."""
    hs = hf_hidden_states(model, ids_row[None, :n])
    fr = torch.stack(hs)[[-4, -3, -2, -1]].sum(0)[0]
    fr = fr[start:(n + end if end is not None else n)]
    return fr, fr.mean(0)
