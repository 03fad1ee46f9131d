"""LLaMA-family decoder-only text models (HF:llama/modeling_llama.py LlamaModel) for the reference's text extractor
(feature_extraction/text/extract_text_huggingface.py:65-85: llama-7b-hf / llama-13b-hf / llama-2-7b / Llama-2-13b-hf, vicuna,
chinese-alpaca-2): `model(**inputs, output_hidden_states=True).hidden_states` and the last-4 sum / special-token slice / mean of
:226-249.

Like whisper.py this model is orchestrated from Python over the C-ABI operators (no engine handle).  Per block:
    mer_rmsnorm -> planes | fused [3D, D] QKV mer_gemm16 (no bias, fp32 out) | mer_rope_attention (causal, rotary q / k, exact fp32)
    | o_proj mer_gemm16 + fp32 residual | mer_rmsnorm -> planes | fused [2F, D] gate|up mer_gemm16 (fp32 out) | mer_swiglu
    | down_proj mer_gemm16 + fp32 residual
The residual stream stays fp32; the GEMMs carry the FLOPs on the tuned kernels, attention over a sentence of tens of tokens is a
small exact kernel.  Hidden states are HF's: the embeddings, the stream after every block, the last one replaced by the final norm's
output.  The embedding lookup is a torch gather (it moves rows, no arithmetic); every FLOP goes through libmer_hip.so.

Attention is causal and nothing else in a block mixes rows, so row (b, t) is a function of tokens 0..t of sentence b: right padding
needs no key mask, and a sentence's features do not depend on its batch mates or on the padded length, bit for bit.  The rows of the
padding itself are computed on the pad token and mean nothing (HF's differ there too: it masks them as keys only).

Not covered (refused at construction): grouped-query attention, rotary scaling, attention / MLP biases, activations other than silu,
head_dim other than 64 / 128; no KV cache, no generation."""
import torch

from . import ops
from .encoders import EncoderOutput, _sd_of
from .whisper import _PASSES, _W16

# the cheapest preset that holds 8e-4 (the project's 1e-3 less the 20 % margin of from_hf()'s ladder) on the UTT and FRAME features of
# every test model, the outlier one included: measured on the MI355X, DESIGN.md "LLaMA-family text encoders"
DEFAULT_PRECISION = "accurate"
LADDER = ("fast", "mx", "balanced", "accurate")   # cheapest first: 1 pass, 1 pass + the MX-fp4 weight residual, 2 passes, 3 passes


def _rope_theta(config):
    """rope_theta of a default-type rotary embedding; any scaling type is refused."""
    rp = getattr(config, "rope_parameters", None)
    if rp is None:
        rp = getattr(config, "rope_scaling", None)
    theta = getattr(config, "rope_theta", None)
    if isinstance(rp, dict):
        kind = rp.get("rope_type", rp.get("type", "default"))
        if kind not in (None, "default"):
            raise ValueError(f"rope_type={kind!r}: only the default rotary embedding is supported (no scaling)")
        theta = rp.get("rope_theta", theta)
    return float(theta if theta is not None else 10000.0)


def check_config(config):
    """Raises ValueError naming the first field this implementation does not cover; returns (D, H, head_dim, F, layers, theta)."""
    def refuse(field, value, why):
        raise ValueError(f"{field}={value!r}: {why}")
    mt = getattr(config, "model_type", None)
    if mt != "llama":
        refuse("model_type", mt, "HipLlamaModel runs LLaMA-architecture checkpoints only")
    act = getattr(config, "hidden_act", None)
    if act != "silu":
        refuse("hidden_act", act, "only silu (SwiGLU) is supported")
    if getattr(config, "attention_bias", False):
        refuse("attention_bias", config.attention_bias, "attention projections with biases are not supported")
    if getattr(config, "mlp_bias", False):
        refuse("mlp_bias", config.mlp_bias, "MLP projections with biases are not supported")
    D, H, F = int(config.hidden_size), int(config.num_attention_heads), int(config.intermediate_size)
    if D % 8 != 0:
        refuse("hidden_size", D, "must be a multiple of 8 (the GEMM planes are read 16 bytes at a time)")
    if F % 8 != 0:
        refuse("intermediate_size", F, "must be a multiple of 8 (the GEMM planes are read 16 bytes at a time)")
    kv = getattr(config, "num_key_value_heads", None)
    if kv is not None and int(kv) != H:
        refuse("num_key_value_heads", kv, f"grouped-query attention is not supported (num_attention_heads={H})")
    hd = getattr(config, "head_dim", None)
    hd = int(hd) if hd is not None else D // H
    if hd not in (64, 128) or hd * H != D:
        refuse("head_dim", hd, f"head_dim must be 64 or 128 and num_attention_heads * head_dim == hidden_size ({H} heads, hidden_size {D})")
    theta = _rope_theta(config)
    return D, H, hd, F, int(config.num_hidden_layers), theta


class HipLlamaModel:
    def __init__(self, state_dict, config, device="cuda:0", precision=DEFAULT_PRECISION):
        self.D, self.H, self.head_dim, self.F, self.n_layers, self.theta = check_config(config)
        if precision not in _PASSES:
            raise ValueError(f"precision={precision!r}: one of {sorted(_PASSES)}")
        ops._lib.lib()   # fail loudly if the HIP library is missing
        sd = _sd_of(state_dict)
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
        self.config, self.device = config, torch.device(device)
        self.precision, self.passes = precision, _PASSES[precision]
        self.eps = float(config.rms_norm_eps)
        dev, P = self.device, self.passes
        f32 = lambda t: t.detach().to(torch.float32).contiguous().to(dev)
        W = lambda t: _W16(t, P, dev)
        self.embed = f32(sd["embed_tokens.weight"])
        self.layers = []
        for l in range(self.n_layers):
            p = f"layers.{l}."
            a, m = p + "self_attn.", p + "mlp."
            self.layers.append(dict(
                n1=f32(sd[p + "input_layernorm.weight"]),
                wqkv=W(torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0)),
                wo=W(sd[a + "o_proj.weight"]),
                n2=f32(sd[p + "post_attention_layernorm.weight"]),
                wgu=W(torch.cat([sd[m + "gate_proj.weight"], sd[m + "up_proj.weight"]], 0)),   # gate rows first: mer_swiglu's order
                wd=W(sd[m + "down_proj.weight"])))
        self.norm = f32(sd["norm.weight"])
        self._rope = None   # (T, cos, sin) of the longest batch so far; a shorter one reads its first rows

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
        return ops.gemm16(a_hi, w.hi, a_lo=a_lo if P == 3 else None, w_lo=w.lo, w_mx=w.mx, passes=P, dtype="f16", out32=True, **kw)[0]

    def _tables(self, T):
        if self._rope is None or self._rope[0] < T:
            cos, sin = ops.rope_tables(T, self.head_dim, self.theta, device=self.device)
            self._rope = (T, cos, sin)
        return self._rope[1], self._rope[2]

    def _ints(self, values):
        return torch.tensor([int(v) for v in values], dtype=torch.int32).to(self.device)

    def _states(self, ids):
        """ids int64 [B, T] on the device -> HF's hidden_states as a list of n_layers + 1 fp32 [B*T, D] tensors."""
        B, T = ids.shape
        D, H, hd, F = self.D, self.H, self.head_dim, self.F
        lo = self.passes == 3
        cos, sin = self._tables(T)
        x = self.embed[ids.reshape(-1)].contiguous()      # embedding gather: index plumbing, no arithmetic
        hs = [x]
        for lay in self.layers:
            _, hh, hl = ops.rmsnorm(x, lay["n1"], self.eps, out32=False, out16=True, out16_lo=lo)
            qkv = self._gemm(hh, hl, lay["wqkv"])
            ch, cl = ops.rope_attention(qkv, cos, sin, B, T, H, hd, hd ** -0.5, out_lo=lo)
            x = self._gemm(ch, cl, lay["wo"], residual=x)
            _, hh, hl = ops.rmsnorm(x, lay["n2"], self.eps, out32=False, out16=True, out16_lo=lo)
            gu = self._gemm(hh, hl, lay["wgu"])
            fh, fl = ops.swiglu(gu, F, lo=lo)
            x = self._gemm(fh, fl, lay["wd"], residual=x)
            hs.append(x)
        hs[-1] = ops.rmsnorm(x, self.norm, self.eps)[0]   # HF: the last hidden state is the final norm's output
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
