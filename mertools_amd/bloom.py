"""BLOOM decoder-only text models (HF:bloom/modeling_bloom.py BloomModel) for the reference's text extractor
(feature_extraction/text/extract_text_huggingface.py:170-196: bloom-7b1, and the smaller bloom-560m ... bloom-3b of the same family):
`model(**inputs, output_hidden_states=True).hidden_states` and the last-4 sum / special-token slice / mean of :226-249.

Like llama.py this model is orchestrated from Python over the C-ABI operators (no engine handle).  Per block:
    mer_layernorm_row -> planes (+ fp32) | fused [3D, D] QKV mer_gemm16 (+ bias, fp32 out) | mer_alibi_attention (causal, exact fp32)
    | dense mer_gemm16 (+ bias) + fp32 residual | mer_layernorm_row -> planes (+ fp32) | dense_h_to_4h mer_gemm16 (+ bias, tanh GELU,
    planes out) | dense_4h_to_h mer_gemm16 (+ bias) + fp32 residual
The residual stream stays fp32: it is the block's input, or the LayerNorm's fp32 output when the checkpoint sets
apply_residual_connection_post_layernorm.  Hidden states are HF's: word_embeddings_layernorm(embedding), the stream after every
block, the last one replaced by ln_f's output.  The embedding lookup is a torch gather (it moves rows, no arithmetic); every FLOP goes
through libmer_hip.so.

BLOOM stores query_key_value head-interleaved ([H, 3, head_dim] rows); the loader permutes weight and bias into q | k | v blocks.
ALiBi's slopes are HF's build_alibi_tensor values (ops.alibi_slopes, bit for bit); the kernel adds slope * (j - t), which softmax's
shift invariance makes equal to HF's slope * j and which is small where the probabilities are large.  pretraining_tp and
slow_but_exact only re-associate HF's own sums and are ignored.

Attention is causal and nothing else in a block mixes rows, so row (b, t) is a function of tokens 0..t of sentence b: right padding
needs no key mask, position j is the token index, and a sentence's features do not depend on its batch mates or on the padded length,
bit for bit.  The rows of the padding itself are computed on the pad token and mean nothing.

Not covered (refused at construction): head_dim other than 64 / 128, hidden_size above 8192 or not a multiple of 8; no KV cache, no
generation, no left padding."""
import torch

from . import ops
from .encoders import EncoderOutput, _sd_of
from .whisper import _PASSES, _W16

# llama.py's rule: the cheapest preset that holds 8e-4 (the project's 1e-3 less the 20 % margin of from_hf()'s ladder) on the UTT and
# FRAME features and 1e-3 on every hidden state of every test model, the outlier one included: measured on the MI355X, DESIGN.md
# "BLOOM text encoders" — here already the one-pass rung holds them (6.8e-4 on the features, 8.4e-4 on the hidden states)
DEFAULT_PRECISION = "fast"
LADDER = ("fast", "mx", "balanced", "accurate")   # cheapest first: 1 pass, 1 pass + the MX-fp4 weight residual, 2 passes, 3 passes


def check_config(config):
    """Raises ValueError naming the first field this implementation does not cover; returns (D, H, head_dim, layers, post_ln_residual)."""
    def refuse(field, value, why):
        raise ValueError(f"{field}={value!r}: {why}")
    mt = getattr(config, "model_type", None)
    if mt != "bloom":
        refuse("model_type", mt, "HipBloomModel runs BLOOM-architecture checkpoints only")
    D, H = int(config.hidden_size), int(config.n_head)
    if D > 8192:
        refuse("hidden_size", D, "mer_layernorm_row holds rows of up to 8192 columns")
    if D % 8 != 0:
        refuse("hidden_size", D, "must be a multiple of 8 (the GEMM planes are read 16 bytes at a time)")
    hd = D // H
    if hd not in (64, 128) or hd * H != D:
        refuse("head_dim", hd, f"head_dim = hidden_size / n_head must be 64 or 128 ({H} heads, hidden_size {D})")
    return D, H, hd, int(config.n_layer), bool(getattr(config, "apply_residual_connection_post_layernorm", False))


def _qkv_blocks(t, H, hd):
    """query_key_value weight [3D, D] or bias [3D] with rows ordered [H, 3, head_dim] -> rows ordered q | k | v ([3, H, head_dim])."""
    return t.reshape(H, 3, hd, *t.shape[1:]).transpose(0, 1).reshape(t.shape)


class HipBloomModel:
    def __init__(self, state_dict, config, device="cuda:0", precision=DEFAULT_PRECISION):
        self.D, self.H, self.head_dim, self.n_layers, self.post_ln_residual = check_config(config)
        if precision not in _PASSES:
            raise ValueError(f"precision={precision!r}: one of {sorted(_PASSES)}")
        ops._lib.lib()   # fail loudly if the HIP library is missing
        sd = _sd_of(state_dict)
        sd = {(k[len("transformer."):] if k.startswith("transformer.") else k): v for k, v in sd.items()}
        self.config, self.device = config, torch.device(device)
        self.precision, self.passes = precision, _PASSES[precision]
        self.eps = float(config.layer_norm_epsilon)
        dev, P, H, hd = self.device, self.passes, self.H, self.head_dim
        f32 = lambda t: t.detach().to(torch.float32).contiguous().to(dev)
        W = lambda t: _W16(t, P, dev)
        ln = lambda p: (f32(sd[p + ".weight"]), f32(sd[p + ".bias"]))
        self.embed = f32(sd["word_embeddings.weight"])
        self.embed_ln = ln("word_embeddings_layernorm")
        self.layers = []
        for l in range(self.n_layers):
            p = f"h.{l}."
            a, m = p + "self_attention.", p + "mlp."
            self.layers.append(dict(
                ln1=ln(p + "input_layernorm"),
                wqkv=W(_qkv_blocks(sd[a + "query_key_value.weight"], H, hd)), bqkv=f32(_qkv_blocks(sd[a + "query_key_value.bias"], H, hd)),
                wo=W(sd[a + "dense.weight"]), bo=f32(sd[a + "dense.bias"]),
                ln2=ln(p + "post_attention_layernorm"),
                w1=W(sd[m + "dense_h_to_4h.weight"]), b1=f32(sd[m + "dense_h_to_4h.bias"]),
                w2=W(sd[m + "dense_4h_to_h.weight"]), b2=f32(sd[m + "dense_4h_to_h.bias"])))
        self.ln_f = ln("ln_f")
        self.slopes = ops.alibi_slopes(H, device=dev)

    @classmethod
    def from_hf(cls, hf_model, **kw):
        return cls(hf_model.state_dict(), hf_model.config, **kw)

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def eval(self):
        return self

    def half(self):
        raise ops._lib.MerError("precision is chosen at construction (precision=...), .half() is not supported")

    # ------------------------------------------------------------------------------------------------------------
    def _gemm(self, a_hi, a_lo, w, **kw):
        P = self.passes
        return ops.gemm16(a_hi, w.hi, a_lo=a_lo if P == 3 else None, w_lo=w.lo, w_mx=w.mx, passes=P, dtype="f16", **kw)

    def _ints(self, values):
        return torch.tensor([int(v) for v in values], dtype=torch.int32).to(self.device)

    def _states(self, ids):
        """ids int64 [B, T] on the device -> HF's hidden_states as a list of n_layers + 1 fp32 [B*T, D] tensors."""
        B, T = ids.shape
        H, hd = self.H, self.head_dim
        lo, post = self.passes == 3, self.post_ln_residual
        emb = self.embed[ids.reshape(-1)].contiguous()      # embedding gather: index plumbing, no arithmetic
        x = ops.layernorm_row(emb, *self.embed_ln, self.eps)[0]
        hs = [x]
        for lay in self.layers:
            n32, hh, hl = ops.layernorm_row(x, *lay["ln1"], self.eps, out32=post, out16=True, out16_lo=lo)
            qkv = self._gemm(hh, hl, lay["wqkv"], bias=lay["bqkv"], out32=True)[0]
            ch, cl = ops.alibi_attention(qkv, self.slopes, B, T, H, hd, hd ** -0.5, out_lo=lo)
            x = self._gemm(ch, cl, lay["wo"], bias=lay["bo"], residual=n32 if post else x, out32=True)[0]
            n32, hh, hl = ops.layernorm_row(x, *lay["ln2"], self.eps, out32=post, out16=True, out16_lo=lo)
            _, fh, fl = self._gemm(hh, hl, lay["w1"], bias=lay["b1"], act="gelu_tanh", out16=True, out16_lo=lo)
            x = self._gemm(fh, fl, lay["w2"], bias=lay["b2"], residual=n32 if post else x, out32=True)[0]
            hs.append(x)
        hs[-1] = ops.layernorm_row(x, *self.ln_f, self.eps)[0]   # HF: the last hidden state is ln_f's output
        return hs

    def forward_raw(self, input_ids, *, lengths=None, hidden_states=False, frames=False, seg_start=None, seg_len=None):
        """-> (hidden_states fp32 [n_layers + 1, B, T, D] | None, frames fp32 [B*T, D] = last-4 sum | None, pooled fp32 [nseg, D] =
        mean of that sum over rows [seg_start[i], seg_start[i] + seg_len[i]) | None) — HipBertModel.forward_raw's contract.  `lengths`
        is accepted for that contract and not needed: attention is causal, so the padding behind a sentence is never a visible key."""
        if self.device.type != "cuda":
            raise ops._lib.MerError("mertools_amd encoders run on a GPU (there is no CPU path)")
        with torch.cuda.device(self.device):   # the op wrappers launch on the current device's current stream
            ids = input_ids.to(self.device, torch.int64).contiguous()
            B, T = ids.shape
            hs = self._states(ids)
            fr = pooled = None
            if frames or seg_start is not None:
                ss = self._ints(seg_start) if seg_start is not None else None
                sl = self._ints(seg_len) if seg_start is not None else None
                fr, pooled = ops.sum_pool(hs[-4:], ss, sl, frames=frames)
            out = torch.stack(hs).view(len(hs), B, T, self.D) if hidden_states else None
            return out, fr, pooled

    def __call__(self, input_ids=None, attention_mask=None, output_hidden_states=False, **_):
        lengths = None
        if attention_mask is not None:
            m = attention_mask.to("cpu")
            lengths = m.sum(dim=1).to(torch.int32)
            T = m.shape[1]
            if not bool((m == (torch.arange(T)[None] < lengths[:, None]).to(m.dtype)).all()):
                raise ops._lib.MerError("attention_mask must be a right-padded prefix mask")
        hs, _, _ = self.forward_raw(input_ids, lengths=lengths, hidden_states=True)
        return EncoderOutput(last_hidden_state=hs[-1], hidden_states=tuple(hs[i] for i in range(hs.shape[0])) if output_hidden_states else None)

    def extract_utterance(self, input_ids, lengths, start, end):
        """Last-4 sum, drop `start` leading / `-end` trailing special tokens (extract_text_huggingface.py:228-231), mean over the
        rest -> [B, D]."""
        B, T = input_ids.shape
        lengths = [int(x) for x in lengths]
        starts = [b * T + start for b in range(B)]
        lens = [max(0, (lengths[b] + (end if end is not None else 0)) - start) for b in range(B)]
        return self.forward_raw(input_ids, lengths=lengths, seg_start=starts, seg_len=lens)[2]
