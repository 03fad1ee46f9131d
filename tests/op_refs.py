"""Plain torch fp64 references of the op-level kernels (include/mer_hip.h), one function per op.

Nothing here touches the GPU or imports the library: these are the yardsticks of tests/test_attention_matrix_gpu.py,
tests/test_gemm_matrix_gpu.py and tests/test_rowops_gpu.py, and tests/test_op_refs_cpu.py pins them against torch's own operators.  Layouts are the ABI's:
qkv is [B*T, 3*H*64] with the q | k | v column blocks, head h at columns 64 h .. 64 h + 63 of its block.
"""
import torch
import torch.nn.functional as F

T16 = {"f16": torch.float16, "bf16": torch.bfloat16, torch.float16: torch.float16, torch.bfloat16: torch.bfloat16}
U2 = 2.0 ** -16        # bf16 hi + lo carries 16 significand bits: the relative error of the pair


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------- attention
def _heads(qkv, B, T, H):
    D = H * 64
    assert qkv.shape == (B * T, 3 * D)
    return [t.double().view(B, T, H, 64).transpose(1, 2) for t in qkv.split(D, dim=1)]          # [B, H, T, 64] each


def attention_scores(qkv, B, T, H, scale, lens=None, bias=None, gate=None):
    """fp64 scores [B, H, T, T] (keys >= lens[b] at -inf) and the values [B, H, T, 64]."""
    q, k, v = _heads(qkv, B, T, H)
    s = q @ k.transpose(2, 3) * scale
    if bias is not None:
        bt = bias.double()[None, :, :, :T]                      # [1, H, T, T]: the table's pad columns are not scores
        s = s + (gate.double()[..., None] * bt if gate is not None else bt)
    if lens is not None:
        lens = torch.as_tensor(lens)
        dead = torch.arange(T)[None, :] >= lens[:, None]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    return s, v


def attention_ref(qkv, B, T, H, scale, lens=None, bias=None, gate=None):
    """softmax(q k^T scale + gate * bias) v in fp64 -> [B, T, H*64].  Rows t >= lens[b] are computed like the others (a query past
    the sequence's length still sees the valid keys): callers compare rows < lens[b] only."""
    s, v = attention_scores(qkv, B, T, H, scale, lens, bias, gate)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, H * 64)


def seq_rel_err(out, ref, lens=None):
    """max over the sequences of max|out - ref| / max|ref|, each over the sequence's rows < lens[b]."""
    worst = 0.0
    for b in range(ref.shape[0]):
        n = int(lens[b]) if lens is not None else ref.shape[1]
        d = (out[b, :n].double() - ref[b, :n].double()).abs().max().item()
        worst = max(worst, d / max(ref[b, :n].abs().max().item(), 1e-30))
    return worst


def attention_rounding_model(qkv, B, T, H, scale, lens=None, bias=None, gate=None, dtype="f16", round_out=False):
    """What the 16-bit kernels compute, in fp64 except for their one deliberate rounding: the un-normalised P = exp(s - max) goes
    through the 16-bit type before P.V (it is the MFMA's B operand) while the normaliser is the sum of the unrounded P; with
    round_out the result is rounded once more to the 16-bit type (a hi plane read alone).  Returns the model's max-norm relative
    error against attention_ref (per sequence over its valid rows, the worst sequence): the yardstick for a tolerance."""
    t16 = T16[dtype]
    s, v = attention_scores(qkv, B, T, H, scale, lens, bias, gate)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    out = (p.to(t16).double() @ v) / p.sum(-1, keepdim=True)
    out = out.transpose(1, 2).reshape(B, T, H * 64)
    if round_out:
        out = out.to(t16).double()
    return seq_rel_err(out, attention_ref(qkv, B, T, H, scale, lens, bias, gate), lens)


def poison_masked(qkv, B, T, H, lens):
    """A copy of qkv whose masked rows are loud: for every sequence b, rows t >= lens[b] of the K block hold 4 x the sequence's
    first query row (the leaked score is that query's row maximum and large for the others) and of the V block 50.0.  Large,
    finite, no NaN / inf — a kernel that lets one such key into the softmax is off by order 1, not 1 / n."""
    D = H * 64
    out = qkv.clone().view(B, T, 3 * D)
    for b in range(B):
        n = int(lens[b])
        if n < T:
            out[b, n:, D:2 * D] = (4.0 * out[b, 0, :D].float()).to(qkv.dtype)
            out[b, n:, 2 * D:] = 50.0
    assert torch.isfinite(out.float()).all()
    return out.view(B * T, 3 * D)


def to_headmajor(qkv, B, T, H):
    """[B*T, 3*H*64] -> [3, B, H, T, 64] holding exactly the same values (what gemm16(headmajor=) writes)."""
    return qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4).contiguous()


# ------------------------------------------------------------------------------------------------------------------ row ops
def act_ref(x, act):
    if act in (None, "none"):
        return x
    if act == "gelu":
        return F.gelu(x)
    if act == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if act in ("gelu_tanh", "gelu_new"):
        return F.gelu(x, approximate="tanh")
    if act == "relu":
        return F.relu(x)
    raise ValueError(act)


def layernorm_ref(x, gamma, beta, eps, act=None):
    D = x.shape[-1]
    y = F.layer_norm(x.double(), (D,), None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps)
    return act_ref(y, act)


def swiglu_ref(y, Fw):
    """silu(y[:, :F]) * y[:, F:2F] in fp64."""
    a, b = y[:, :Fw].double(), y[:, Fw:2 * Fw].double()
    return a * torch.sigmoid(a) * b


def token_sum_ref(x, scale=1.0):
    return x.double().sum(1) * scale


def add_pos_ref(x, pos):
    """x[r] + pos[r % P] in the input's own precision (one fp32 add per element: the kernel must match bit for bit)."""
    idx = torch.arange(x.shape[0]) % pos.shape[0]
    return x + pos[idx]


def conv0_ref(wav, w, stride, bias=None):
    """Conv1d(1 -> C, k, stride) in fp64, channels-last [B, T0, C]."""
    y = F.conv1d(wav[:, None].double(), w[:, None].double(), None if bias is None else bias.double(), stride=stride)
    return y.transpose(1, 2)


def conv0_gn_gelu_ref(wav, w, stride, gamma, beta, eps, valid=None):
    """conv0 + GroupNorm(C groups: per channel over time) + GELU, fp64 [B, T0, C]; valid[b] = the frames of row b the statistics run
    over (all frames are normalised with them)."""
    y = conv0_ref(wav, w, stride)                                            # [B, T0, C]
    out = torch.empty_like(y)
    for b in range(y.shape[0]):
        n = int(valid[b]) if valid is not None else y.shape[1]
        mu = y[b, :n].mean(0, keepdim=True)
        var = y[b, :n].var(0, unbiased=False, keepdim=True)
        out[b] = F.gelu((y[b] - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double())
    return out


def posconv_pack_ref(x, G, K, valid=None):
    """x [B, T, D] -> [B, G, T + K, D / G]: group-major, K // 2 zero frames in front, frames >= valid[b] zero."""
    B, T, D = x.shape
    Dg, half = D // G, K // 2
    out = torch.zeros(B, G, T + K, Dg, dtype=torch.float64)
    for b in range(B):
        n = int(valid[b]) if valid is not None else T
        out[b, :, half:half + n] = x[b, :n].double().view(n, G, Dg).transpose(0, 1)
    return out


def valid_frames_ref(valid_samples, L, kernels, strides):
    """Pure-integer frame counts: n = min(valid, L), then per valid conv n = (n - k) // s + 1 if n >= k else 0.  Returns one list per
    conv layer ([n_conv][B]); the conv-0 count is reported clamped to >= 1 (a clip shorter than the receptive field stays finite
    downstream), the recursion itself runs on the unclamped value."""
    rows = [[] for _ in kernels]
    for vs in valid_samples:
        n = min(int(vs), L)
        for i, (k, s) in enumerate(zip(kernels, strides)):
            n = (n - k) // s + 1 if n >= k else 0
            rows[i].append(max(n, 1) if i == 0 else n)
    return rows


def vit_patchify_ref(px, P):
    """[N, C, H, W] -> [N * gh * gw, ceil8(C P P)] rows in the (c, i, j) order of a flattened Conv2d weight, zero pad columns."""
    N, C, H, W = px.shape
    gh, gw = H // P, W // P
    rows = px.view(N, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, C * P * P)
    return F.pad(rows, (0, (-rows.shape[1]) % 8))


def video_patchify_ref(px, P, ts):
    """[B, F, C, H, W] -> [B * (F/ts) * gh * gw, C ts P P] rows in the (c, dt, i, j) order of a flattened Conv3d weight."""
    B, Fr, C, H, W = px.shape
    nt, gh, gw = Fr // ts, H // P, W // P
    return px.view(B, nt, ts, C, gh, P, gw, P).permute(0, 1, 4, 6, 3, 2, 5, 7).reshape(B * nt * gh * gw, C * ts * P * P)


def canary16(shape, dtype, device):
    """A 16-bit buffer filled with the bit pattern 0x7B7B (a large finite value in both formats)."""
    t = torch.empty(shape, dtype=torch.int16, device=device).fill_(0x7B7B)
    return t.view(T16[dtype])


def is_canary16(t):
    return bool((t.contiguous().view(torch.int16) == 0x7B7B).all())


CANARY32 = -1.2345678e30


def is_canary32(t):
    return bool((t == CANARY32).all())


# --------------------------------------------------------------------------------------------------------------------- gemm16
U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}          # unit roundoff of one 16-bit plane (round to nearest)
U_PAIR = {"f16": 2.0 ** -21, "bf16": U2}              # ... and of a hi + lo pair
GEMM_TOL = 2e-5                                       # the project's max-norm relative bound on an fp32 GEMM output (tests/test_ops_gpu.py)
GEMM_TERMS = {1: ("hh",), 2: ("hh", "hl"), 3: ("hh", "hl", "lh"), 6: ("hh", "lh")}    # passes -> plane products, (A plane)(W plane)


def gemm16_terms_ref(a_hi, a_lo, w_hi, w_lo, terms):
    """fp64 sum of the named plane products: "hl" = a_hi . w_lo^T and so on ("ll" exists only to model a mis-paired pass)."""
    pa, pw = {"h": a_hi, "l": a_lo}, {"h": w_hi, "l": w_lo}
    return sum(pa[t[0]].double() @ pw[t[1]].double().T for t in terms)


def gemm16_planes_ref(a_hi, a_lo, w_hi, w_lo, passes):
    """What mer_gemm16 accumulates for `passes`, in fp64 on the ROUNDED planes: 1 = hh, 2 = hh + a_hi.w_lo, 3 = hh + a_hi.w_lo +
    a_lo.w_hi, 6 = hh + a_lo.w_hi.  The planes are the inputs, so the reference carries no input rounding and one tolerance serves
    both 16-bit types."""
    return gemm16_terms_ref(a_hi, a_lo, w_hi, w_lo, GEMM_TERMS[passes])


def gemm_epilogue_ref(z, bias=None, act=None, residual=None, table=None, seg_rows=0):
    """fp64 epilogue of mer_gemm16 on pre-activations z [M, N]: + bias[n] (or + table[m // seg_rows, n]), act, + residual."""
    z = z.double()
    if table is not None:
        assert bias is None and seg_rows > 0
        z = z + table.double().repeat_interleave(seg_rows, 0)[:z.shape[0], :z.shape[1]]
    elif bias is not None:
        z = z + bias.double()
    z = act_ref(z, act)
    return z if residual is None else z + residual.double()


def act_model32(x, act):
    """The activation formulas of csrc/common.h restated in torch fp32 (exact exp / division where the kernel uses v_exp_f32 /
    v_rcp_f32): what fp32 arithmetic alone costs against act_ref.  Only the two formulas whose bound is derived from it."""
    x = x.float()
    if act == "quick_gelu":
        return x * (1.0 / (1.0 + torch.exp(-1.702 * x)))
    if act in ("gelu_tanh", "gelu_new"):
        u = 0.7978845608028654 * (x + 0.044715 * x * x * x)
        return 0.5 * x * (2.0 - 2.0 / (torch.exp(2.0 * u) + 1.0))
    raise ValueError(act)


def act_bound(pre, act, residual=None):
    """(bound, model) for an fp32 output after `act`: 2e-5 for none / gelu / relu; max(2e-5, 2 x model) for quick_gelu / gelu_tanh,
    model = max-norm relative error of act_model32 on these very pre-activations against fp64 (never the kernel's output)."""
    if act not in ("quick_gelu", "gelu_tanh", "gelu_new"):
        return GEMM_TOL, 0.0
    ref = act_ref(pre.double(), act)
    got = act_model32(pre, act).double()
    if residual is not None:
        ref, got = ref + residual.double(), got + residual.double()
    model = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    return max(GEMM_TOL, 2.0 * model), model


def indep_planes(M, N, K, dtype, seed):
    """Input family "indep": four INDEPENDENT random 16-bit planes, a_hi ~ N(0, 1), a_lo ~ 0.5 N(0, 1), w_hi ~ 0.05 N(0, 1), w_lo ~
    0.025 N(0, 1).  The lo planes are nobody's residual — the kernel cannot tell — and every product term is of order 1 next to hh,
    so a dropped or mis-paired pass moves the result by tens of percent instead of 2^-11."""
    t16 = T16[dtype]
    return (rand((M, K), seed).to(t16), rand((M, K), seed + 1, 0.5).to(t16),
            rand((N, K), seed + 2, 0.05).to(t16), rand((N, K), seed + 3, 0.025).to(t16))


def split_planes(x, dtype):
    """Input family "split": the true hi / lo split of fp32 data (hi = rn(x), lo = rn(x - hi))."""
    t16 = T16[dtype]
    hi = x.float().to(t16)
    return hi, (x.float() - hi.float()).to(t16)


def round16(x, dtype):
    return x.float().to(T16[dtype])


def auto_tile(M, N, passes):
    """The tile == 0 rule of mer_gemm16 (csrc/gemm16.hip) for a non-MX launch: 2 = 128x64, 1 = 128x128, 3 = 256x256."""
    t256 = -(-M // 256) * -(-N // 256)
    few_narrow = t256 <= 96 and N <= 1024 and passes != 4
    return 2 if N <= 64 else (3 if (M >= 1024 and N >= 192 and not few_narrow) else 1)
