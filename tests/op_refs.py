"""Plain torch fp64 references of the op-level kernels (include/mer_hip.h), one function per op.

Nothing here touches the GPU or imports the library: these are the yardsticks of tests/test_attention_matrix_gpu.py,
tests/test_gemm_matrix_gpu.py, tests/test_rowops_gpu.py and tests/test_seq_bias_gpu.py, and tests/test_op_refs_cpu.py pins them against torch's own operators.  Layouts are the ABI's:
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


# ----------------------------------------------------------------------------------------------- fp32 training kernels
# (csrc/gemm32.hip, csrc/fusion.hip: tests/test_train_kernels_gpu.py).  U32 is the unit roundoff of fp32 (round to nearest).
U32 = 2.0 ** -24
TINY32 = 2.0 ** -126  # smallest normal fp32
GELU_LIP = 1.13        # max |d gelu / dx| = 1.1289 (at x = sqrt 2): how a pre-activation error reaches a GELU output


def canary32(shape, device="cpu"):
    return torch.full(shape, CANARY32, dtype=torch.float32, device=device)


def gemm32_pre(a, w, bias=None, trans_a=False, trans_w=False):
    """fp64 pre-activations of mer_gemm32 on the operands AS STORED: a is [M, K] ([K, M] with trans_a), w is [N, K] ([K, N] with
    trans_w).  Returns (z, S) with S = |A| |W|^T + |bias|, the magnitude sum the rounding bound scales with."""
    A = a.double().T if trans_a else a.double()
    Wm = w.double().T if trans_w else w.double()
    z, S = A @ Wm.T, A.abs() @ Wm.abs().T
    if bias is not None:
        z, S = z + bias.double(), S + bias.double().abs()
    return z, S


def gemm32_ref(a, w, bias=None, act=None, trans_a=False, trans_w=False, base=None):
    """fp64 act(A W^T + bias) (+ base: what accumulate = 1 adds to)."""
    z, _ = gemm32_pre(a, w, bias, trans_a, trans_w)
    y = act_ref(z, act)
    return y if base is None else y + base.double()


def gemm32_bound(S, K, out=None):
    """Elementwise bound on |mer_gemm32 - fp64| before the activation: (2K + 3) u S.  Each of the K products is rounded at most once
    (not at all where the MFMA fuses) and enters at most K additions' worth of accumulation error whatever the order of the sum: K u
    + K u to first order; the bias add is one more rounding; the remaining 2 u cover the second-order terms of (1 + u)^(2K+1) for
    every K below 2^20.  accumulate = 1 rounds once more, on the stored sum: + u |out|."""
    b = (2 * K + 3) * U32 * S
    return b if out is None else b + U32 * out.double().abs()


def colsum_ref(x, base=None):
    s = x.double().sum(0)
    return s if base is None else s + base.double()


def colsum_bound(x, base=None, out=None):
    """(M + 1) u sum_m |x[m, n]|: M in-order additions (the first onto 0) + second order; accumulate adds u |out|."""
    b = (x.shape[0] + 1) * U32 * x.double().abs().sum(0)
    return b if base is None else b + U32 * out.double().abs()


def fuse_fwd_ref(h, att):
    """fused[b, j] = sum_e h[b, e H + j] att[b, e] in fp64, and the magnitude sum sum_e |h att|."""
    B, E = att.shape
    H = h.shape[1] // E
    t = h.double().view(B, E, H) * att.double()[:, :, None]
    return t.sum(1), t.abs().sum(1)


def fuse_fwd_chain32(h, att):
    """The kernel's own arithmetic in fp32: s = fmaf(h, att, s) over e in stream order (one rounding per step, emulated in fp64:
    the product of two fp32 values is exact in fp64, and rounding the fp64 sum of two fp32-representable addends of this range to
    fp32 equals the fused result except in double-rounding ties, which the bound absorbs)."""
    B, E = att.shape
    H = h.shape[1] // E
    s = torch.zeros(B, H, dtype=torch.float64)
    for e in range(E):
        s = (s + h[:, e * H:(e + 1) * H].double() * att[:, e:e + 1].double()).float().double()
    return s.float()


def fuse_bwd_ref(dout, h, att):
    """(dh as the one fp32 product it is, datt in fp64, sum_j |dout h| for datt's bound)."""
    B, E = att.shape
    H = h.shape[1] // E
    dh = (dout[:, None, :] * att[:, :, None]).reshape(B, E * H)                      # fp32 x fp32 -> fp32, one rounding
    t = dout.double()[:, None, :] * h.double().view(B, E, H)
    return dh, t.sum(2), t.abs().sum(2)


def ce_ref(logits, target, gout=1.0):
    """fp64 CELoss = sum_b -log_softmax(logits)[b, target[b]] / B: (probs, rows, loss, dlogits = gout (probs - onehot) / B)."""
    x = logits.double()
    B = x.shape[0]
    lsm = torch.log_softmax(x, 1)
    probs = lsm.exp()
    rows = -lsm.gather(1, target.view(-1, 1)).squeeze(1)
    onehot = torch.zeros_like(x).scatter_(1, target.view(-1, 1), 1.0)
    return probs, rows, rows.sum() / B, float(gout) * (probs - onehot) / B


def ce_bounds(logits, target, gout=1.0, ulp_fn=2):
    """Elementwise first-order bounds for ce_rows_kernel / ce_bwd_kernel against ce_ref, from counted roundings (u = 2^-24; expf and
    logf are taken as `ulp_fn` ulp = 2 ulp_fn u relative, twice the 1 ulp HIP documents).  Per row, with d = l - max, p = softmax:
      s   = sum exp(d):   each term carries (2 ulp_fn + |d|) u (function + rounded argument), the C - 1 additions u each in any order:
                          relative (C - 1 + 2 ulp_fn + sum_c p_c |d_c|) u
      lse = max + log s:  absolute  E = rel(s) + 2 ulp_fn u |log s| + u |lse|
      a   = l - lse:      absolute  u |a| + E;   probs = exp(a): relative (2 ulp_fn + 2 |a|) u + E
      row = lse - l_t:    absolute  E + u |row|
      dl  = g (p - 1h) / B: |g| / B dprobs + 4 u |dl|   (subtraction, product, division at <= 2 u)
    plus, on probs, the fp32 underflow threshold 2^-126: a probability below it (exp(-160) in the +-80 rows) is stored as a subnormal
    or as 0, an absolute error of up to the threshold that no relative bound covers.
    Returns (dprobs [B, C], drows [B], ddlogits [B, C])."""
    x = logits.double()
    B, C = x.shape
    mx = x.max(1, keepdim=True).values
    d = x - mx
    s = d.exp().sum(1, keepdim=True)
    lse = mx + s.log()
    p = (x - lse).exp()
    rel_s = (C - 1 + 2 * ulp_fn + (p * d.abs()).sum(1, keepdim=True)) * U32
    E = rel_s + 2 * ulp_fn * U32 * s.log().abs() + U32 * lse.abs()
    a = x - lse
    dprobs = p * ((2 * ulp_fn + 2 * a.abs()) * U32 + E) + TINY32
    rows = (lse - x.gather(1, target.view(-1, 1))).squeeze(1)
    drows = E.squeeze(1) + U32 * rows.abs()
    onehot = torch.zeros_like(x).scatter_(1, target.view(-1, 1), 1.0)
    dl = float(gout) * (p - onehot) / B
    return dprobs, drows, abs(float(gout)) / B * dprobs + 4 * U32 * dl.abs()


def mean_rows_bound(rows):
    """mean_rows_kernel: in-order fp32 sum of B rows, then one division: (B + 1) u sum|row| / B."""
    B = rows.numel()
    return (B + 1) * U32 * rows.double().abs().sum().item() / B


def mse_ref(pred, target, gout=1.0):
    """fp64 (rows = (pred - target)^2, loss = sum rows / B, dpred = gout 2 (pred - target) / B)."""
    d = pred.double() - target.double()
    return d * d, (d * d).sum() / d.numel(), float(gout) * 2.0 * d / d.numel()


MSE_ROW_REL = (1 + U32) ** 3 - 1        # d = fl(p - t) enters the square twice (2 u), the product rounds once: three roundings
MSE_BWD_REL = 5 * U32                   # fl(g * 2), d's own rounding, the product, the division (<= 2 u)


ADAM_R = 16       # see adam_bounds


def adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step, clip, mutate=None):
    """torch.optim.Adam (L2 weight decay) as csrc/fusion.hip documents it, in fp64 ON THE fp32-ROUNDED hyper-parameters the ABI receives
    (`1 - b` is formed from the rounded b, as the kernel forms it):  clip, then g += wd p, then m = b1 m + (1 - b1) g,
    v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);  step t counts from 1.
    mutate (the CPU sensitivity tests): "clip_after_wd", "eps_in_sqrt", "step_minus_1".  Returns (p, m, v, aux) in fp64."""
    f = lambda x: float(torch.tensor(x, dtype=torch.float32))
    lr, b1, b2, eps, wd, clip = f(lr), f(b1), f(b2), f(eps), f(wd), f(clip)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if mutate == "clip_after_wd":
        gc = g + wd * p
        gc = gc.clamp(-clip, clip) if clip > 0 else gc
        gi = gc
    else:
        gc = g.clamp(-clip, clip) if clip > 0 else g
        gi = gc + wd * p
    m1 = b1 * m + (1.0 - b1) * gi
    v1 = b2 * v + (1.0 - b2) * gi * gi
    t = step - 1 if mutate == "step_minus_1" else step
    bc1, bc2 = (torch.tensor(1.0 - b ** t, dtype=torch.float64) for b in (b1, b2))      # tensors: the step - 1 mutation divides by 0 at t = 1
    if mutate == "eps_in_sqrt":
        denom = (v1 / bc2 + eps).sqrt()
    else:
        denom = v1.sqrt() / bc2 ** 0.5 + eps
    upd = (lr / bc1) * (m1 / denom)
    G = gc.abs() + (wd * p).abs()
    aux = dict(G=G, upd=upd, denom=denom, lr_bc1=lr / bc1, r1=b1 ** t / bc1, r2=b2 ** t / bc2, b1=b1, b2=b2, m0=m, v0=v)
    return p - upd, m1, v1, aux


def adam_bounds(p1, aux):
    """Elementwise bounds on |kernel - adam_ref| for (p, m, v), counted from the kernel's roundings (u = 2^-24), first order with the
    second order absorbed as stated.  G = |clip(g)| + |wd p| bounds |g_i| and carries fmaf(wd, p, g)'s one rounding (u G).
      m = b1 m + (1 - b1) g_i : the first term is rounded by its product and the addition (2), the second by g_i's rounding, its product
          and the addition (3); 1 - b1 is exact in fp32 for b1 in [0.5, 1]:                     dm <= 4 u (|b1 m| + (1 - b1) G)
      v = b2 v + (1 - b2) g_i g_i : second term: g_i's rounding twice, two products, the addition (5):  dv <= 6 u (b2 v + (1 - b2) G^2)
          — all terms of v are positive, so dv / v <= 6 u: no cancellation.
      bias corrections bc = 1 - b^t in fp32: powf within 2 ulp (4 u b^t absolute; HIP documents 1 ulp, the host's libm less) and the
          subtraction's rounding: relative c = 4 u b^t / (1 - b^t) + u — the CANCELLATION term, 4e3 u for b2 = 0.999, t = 1.
      update U = (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)), divisions and square roots taken as <= 2 u each:
          lr / bc1: c1 + 2 u;  sqrt(v): 3 u + u;  / sqrt(bc2): + c2 / 2 + u + 2 u;  + eps: + u (both addends positive);
          m / denom: + 2 u;  the product: + u   =>  relative R = c1 + c2 / 2 + 13 u = (4 r1 + 2 r2 + 14.5) u, r = b^t / (1 - b^t);
          ADAM_R = 16 replaces 14.5 (1.5 u for the second-order terms).  m's own error enters absolutely (m may cancel to ~0):
                                                                                   dU <= |U| R + (lr / bc1) / denom dm
      p = fl(p - U):                                                                dp <= u |p| + dU."""
    G, b1, b2 = aux["G"], aux["b1"], aux["b2"]
    dm = 4 * U32 * ((b1 * aux["m0"]).abs() + (1.0 - b1) * G)
    dv = 6 * U32 * (b2 * aux["v0"] + (1.0 - b2) * G * G)
    R = (4 * aux["r1"] + 2 * aux["r2"] + ADAM_R) * U32
    dU = aux["upd"].abs() * R + aux["lr_bc1"] / aux["denom"] * dm
    return U32 * p1.abs() + dU, dm, dv


def adam_inputs(n, seed):
    """p ~ N(0, 1); |g| log-uniform over 1e-9 .. 1e2 with random signs, exact zeros and entries beyond +-0.05 on both sides pinned in;
    m ~ 0.1 N(0, 1), v = (0.1 N(0, 1))^2: a state some steps in.  Every fourth element is a fresh small parameter instead (m = v = 0,
    p ~ 1e-7 N(0, 1)): there sqrt(v) is of the order of |g| whatever the weight decay, so eps = 1e-8 decides the update for the small
    gradients and is invisible for the large ones."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    fresh = torch.arange(n) % 4 == 0
    p[fresh] *= 1e-7
    g = 10.0 ** (torch.rand(n, generator=gen) * 11.0 - 9.0) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
    fixed = torch.tensor([0.0, 100.0, -100.0, 0.06, -0.06, 0.05, -0.05, 1e-9, -1e-9, 0.0])
    k = min(n, fixed.numel())
    g[n - k:] = fixed[:k]
    m = 0.1 * torch.randn(n, generator=gen)
    v = (0.1 * torch.randn(n, generator=gen)) ** 2
    m[fresh], v[fresh] = 0.0, 0.0
    return p, g, m, v


def lstm_ref(x, state_dict, wgt):
    """torch.nn.LSTM(...).double() on the CPU: h_T [B, H] and the gradients of sum(h_T * wgt) w.r.t. x and the four parameters."""
    import torch.nn as nn
    D, H = x.shape[2], state_dict["weight_hh_l0"].shape[1]
    ref = nn.LSTM(D, H, num_layers=1, batch_first=True).double()
    ref.load_state_dict({k: v.double() for k, v in state_dict.items()})
    xr = x.double().clone().requires_grad_(True)
    _, (hn, _) = ref(xr)
    (hn[0] * wgt.double()).sum().backward()
    grads = {"x": xr.grad}
    grads.update({k: getattr(ref, k).grad for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
    return hn[0].detach(), grads


def small_attention_ref(q, k, v, B, Tq, Tk, H, scale, causal=False):
    """fp64 softmax(q k^T scale) v per (batch, head): q [B*Tq, H*64], k / v [B*Tk, H*64] -> [B*Tq, H*64]; causal masks key j > query t."""
    qh, kh, vh = (t.double().reshape(B, -1, H, 64).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(2, 3) * scale
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), diagonal=1), float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B * Tq, H * 64)


def small_attention_bound(q, k, v, B, Tq, Tk, H, scale):
    """Elementwise first-order bound on |small_attention_kernel - small_attention_ref| (non-causal), from the kernel's roundings on THESE
    inputs (u = 2^-24; nothing here looks at the kernel's output):
      score  s_j = scale * (64 fused steps over d in stream order): each step rounds its running sum once, so the chain's error is at most
             u sum_i |S_i| over the fp64 running sums S_1 .. S_64 — the data's own figure, not the worst case 64 u sum|q k| —, and the
             multiplication by scale rounds once more:  e_j = u (scale sum_i |S_i| + |s_j|);  E = max_j e_j bounds the maximum's error
      weight w_j = expf(s_j - max): relative  r_j = e_j + E + (|s_j - max| + 4) u   (argument errors, the subtraction, expf at 2 ulp)
      out_d  = (sum_j w_j v_jd) / (sum_j w_j): four chains of ceil(Tk / 4) fused steps, two additions, the product with 1 / sum;
             the sum itself ceil(Tk / 256) additions per thread, an 8-level tree and the reciprocal (<= 2 u):
             |d out_d| <= sum_j p_j |v_jd| (r_j + (Tk / 4 + 4) u)  +  |out_d| (sum_j p_j r_j + (Tk / 256 + 11) u),  p = softmax
    times 1.01 for the second-order terms (r_j stays below 1e-3)."""
    qh, kh, vh = (t.double().reshape(B, -1, H, 64).transpose(1, 2) for t in (q, k, v))
    run = (qh[:, :, :, None, :] * kh[:, :, None, :, :]).cumsum(-1)                      # [B, H, Tq, Tk, 64] running sums S_i
    s = run[..., -1] * scale
    e = U32 * (scale * run.abs().sum(-1) + s.abs())
    a = s - s.max(-1, keepdim=True).values
    r = e + e.max(-1, keepdim=True).values + (a.abs() + 4) * U32
    p = torch.softmax(s, -1)
    out = p @ vh
    num = (p * (r + (Tk / 4 + 4) * U32)) @ vh.abs()
    den = (p * r).sum(-1, keepdim=True) + (Tk / 256 + 11) * U32
    return (1.01 * (num + out.abs() * den)).transpose(1, 2).reshape(B * Tq, H * 64)


def max_rel(out, ref):
    """max|out - ref| / max|ref| in fp64 on the CPU."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    return (out - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def worst_ratio(out, ref, bound):
    """max over the elements of |out - ref| / bound (0 / 0 counts as 0: an exact value under a zero bound passes)."""
    err = (out.detach().double().cpu() - ref.double()).abs()
    bound = bound.double() if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return r.max().item() if r.numel() else 0.0


# ------------------------------------------------------------------------------------------- the group engine at its dispatch edges
# (csrc/fusion_topn_group.hip: tests/test_train_kernels_gpu.py::test_group_engine_edges).  A case is one group of G = 3 models run for
# two train steps and one eval step; model 1 has a partial batch at the last train step and at the eval step, model 2 is idle at
# step 0.  kind "topn": FusionTopnGroupTrainer on Attention_TOPN; "att3": FusionGroupTrainer on the 3-stream Attention model.
GROUP_CASES = (
    dict(id="H18-M2-C7-B5", kind="topn", D=(5, 18), H=18, C1=7, C2=0, B=5, seed=8),                  # H % 4 != 0: misaligned mh + e*H and ldw
    dict(id="H18-M18-C2v-B17", kind="topn", D=(3, 8, 5, 12, 7, 16, 9, 4, 11, 6, 13, 20, 1, 15, 10, 2, 14, 17), H=18, C1=2, C2=1, B=17),
    dict(id="H18-M1-C64-B33", kind="topn", D=(7,), H=18, C1=64, C2=0, B=33),
    dict(id="H20-M2-C7v-B33", kind="topn", D=(20, 33), H=20, C1=7, C2=1, B=33),              # K % 16 != 0 in every hidden layer
    dict(id="H20-M18-C64-B5", kind="topn", D=(4, 9, 6, 3, 8, 5, 12, 7, 2, 11, 16, 1, 10, 13, 14, 15, 17, 18), H=20, C1=64, C2=0, B=5),
    dict(id="H20-M1-C2v-B1", kind="topn", D=(16,), H=20, C1=2, C2=1, B=1, seed=1),
    dict(id="H48-M2-C2-B17", kind="topn", D=(48, 17), H=48, C1=2, C2=0, B=17),
    dict(id="H48-M18-C7v-B1", kind="topn", D=(3, 8, 5, 12, 7, 16, 9, 4, 11, 6, 13, 20, 1, 15, 10, 2, 14, 17), H=48, C1=7, C2=1, B=1),
    dict(id="H48-M1-C64v-B5", kind="topn", D=(32,), H=48, C1=64, C2=1, B=5, seed=111),
    dict(id="att3-H48-C7v-B17", kind="att3", D=(24, 16, 21), H=48, C1=7, C2=1, B=17),        # M = 3 through the mer_fusion_group_* ABI
    dict(id="limit-B2048", kind="topn", D=(4,), H=4, C1=2, C2=0, B=2048, counts=(2048, 2047, 2048)),
)
GROUP_LR, GROUP_WD, GROUP_CLIP = (1e-3, 2e-3, 5e-4), (1e-5, 0.0, 1e-4), (1.0, -1.0, -1.0)
# grad_clip = 1.0 on model 0 bites in every case (some first-step gradients exceed it: 5e-5 .. 27 % of them) without sitting far below
# the gradients' own scale: a clip of 0.05 under gradients of 10 .. 50 makes max|m|, max|v| the clip's while the fp32 error of an
# unclipped element stays that of its long sums — a plain fp32 composition on the CPU is then itself 2e-4 off in m and v.
GROUP_ROWS = 97            # rows of the split table (2100 for the B = 2048 case)
# measured on the MI355X (worst max-norm relative error against the fp64 reference over the cases of the class) -> 4 x, capped at the
# project's 5e-5 for losses and 1e-4 for outputs, gradients, parameters and moments.  Two classes, so that the ten cases with B <= 33
# are not asserted at the B = 2048 case's figures (in-order fp32 sums over 2048 rows).
GROUP_WORST = dict(small=dict(loss=7.23e-6, out=9.36e-6, grad=9.45e-7, param=2.59e-5), limit=dict(loss=1.23e-6, out=5.38e-7, grad=1.09e-6, param=2.21e-6))
GROUP_TOL = dict(small=dict(loss=2.9e-5, out=3.7e-5, grad=3.8e-6, param=1e-4), limit=dict(loss=4.9e-6, out=2.2e-6, grad=4.4e-6, param=8.8e-6))


def group_tol(case):
    return GROUP_TOL["limit" if case["B"] > 64 else "small"]


def group_lr(case):
    return list(GROUP_LR)


def group_encoder_names(case):
    M = len(case["D"])
    return ["audio_encoder", "text_encoder", "video_encoder"] if case["kind"] == "att3" else [f"encoder{i}" for i in range(M)]


def group_param_spec(case):
    """(name, shape) in model.parameters() order = the engine's flat layout."""
    H, M = case["H"], len(case["D"])
    spec = []
    for name, d in list(zip(group_encoder_names(case), case["D"])) + [("attention_mlp", M * H)]:
        for i, k in ((1, d), (2, H), (3, H)):
            spec += [(f"{name}.linear_{i}.weight", (H, k)), (f"{name}.linear_{i}.bias", (H,))]
    for name, n in (("fc_att", M), ("fc_out_1", case["C1"]), ("fc_out_2", case["C2"])):
        spec += [(f"{name}.weight", (n, H)), (f"{name}.bias", (n,))]
    return spec


GROUP_MARGIN = 1e-4        # no gated pre-activation of the fp64 reference within this fraction of its layer's max|z| of zero
GROUP_LEVELS = [(False, 1), (False, 2), (False, 3), (True, 1), (True, 2), (True, 3)]      # (attention_mlp?, linear_i) in forward order
_group_cache = {}


def _group_raw(case, seed):
    """An ordinary problem: per model, order-one weights U(-a, a) with a = sqrt(6 / fan_in) (He's uniform init: the pre-activations
    keep unit scale through the ReLUs, and the data term outweighs the bias, so a unit's gate differs between rows) and biases U(-0.1,
    0.1); N(0, 1) features, uniform labels, a random index table."""
    gen = torch.Generator().manual_seed(seed)
    G, B = 3, case["B"]
    n_rows = GROUP_ROWS if B <= 64 else B + 52
    inits = []
    for g in range(G):
        sd = {}
        for name, shape in group_param_spec(case):
            bound = (6.0 / shape[1]) ** 0.5 if name.endswith("weight") else 0.1
            sd[name] = (torch.rand(shape, generator=gen) * 2 - 1) * bound
        inits.append(sd)
    feats = [torch.randn(n_rows, d, generator=gen) for d in case["D"]]
    emos = torch.randint(0, case["C1"], (n_rows,), generator=gen)
    vals = torch.rand(n_rows, generator=gen) * 6 - 3
    index = torch.randint(0, n_rows, (3, G, B), generator=gen, dtype=torch.int32)
    full = case.get("counts", (B, max(1, B // 2), B))
    count = torch.tensor([[full[0], B, 0], list(full), list(full)], dtype=torch.int32)
    return dict(inits=inits, feats=feats, emos=emos, vals=vals, index=index, count=count, n_rows=n_rows, nudged=0)


def group_gate_margin(pres):
    """min over the gated layers, models and steps of min|z| / max|z|."""
    return min(float(z.abs().min() / z.abs().max()) for _, _, _, z in pres)


def _group_nudge(case, data):
    """Moves the few pre-activations that sit within 2 GROUP_MARGIN max|z| of zero out of that band by shifting their unit's INITIAL
    bias by the smallest amount that puts zero in the middle of a wide enough gap between that unit's pre-activations over all rows
    and steps (a shift of the order of 1e-4 .. 1e-3 of the layer's scale: the network stays the ordinary one).  Layers are visited in forward order, the reference re-run for each: a shift moves its own
    layer by itself and the later layers a little, and the earlier ones only through the gradients (second order)."""
    for _ in range(6):
        clean = True
        for att, i in GROUP_LEVELS:
            _, pres = group_reference(case, data, collect_pre=True)
            layers = {}
            for g, s, name, z in pres:
                if name.startswith("attention_mlp") == att and name.endswith(f"linear_{i}"):
                    layers.setdefault((g, name), []).append((2 * GROUP_MARGIN * float(z.abs().max()), z))
            todo = {}
            for (g, name), items in layers.items():
                need = max(t for t, _ in items)
                zs = torch.cat([z for _, z in items])                     # every step's rows of this layer: one bias serves them all
                for col in (zs.abs() < need).any(0).nonzero().flatten().tolist():
                    todo[(g, name, col)] = (need, zs[:, col])
            for (g, name, col), (need, zs) in todo.items():
                zs = zs.sort().values                                     # put zero in the middle of the nearest gap of width >= 2 need
                gaps = (zs[1:] - zs[:-1] >= 2 * need).nonzero().flatten()
                mids = (zs[1:] + zs[:-1])[gaps] / 2
                delta = -mids[mids.abs().argmin()]
                data["inits"][g][name + ".bias"][col] += float(delta)
                data["nudged"] += 1
                clean = False
        if clean:
            break
    return data


def group_case_data(case):
    """Everything a case runs on, made on the CPU from fixed seeds: per-model fp32 inits (_group_raw: order-one weights), the split
    table, the [3, G, B] index and [3, G] count tables.  ReLU gates are taken on fp32 values: a pre-activation within rounding of zero
    would flip a gate against the fp64 reference for no fault, so no gated pre-activation of the reference may lie within GROUP_MARGIN
    max|z| of zero (asserted per case in tests/test_op_refs_cpu.py, with the share of units whose gate differs between rows).
    Where a case is small enough for a seed to exist (about 3e-4 of the pre-activations of an ordinary network fall in the band: the
    cases with a "seed" entry were found by trying seeds 0, 1, ...), the seed alone achieves it.  The others hold 2e4 .. 4e5
    pre-activations, no seed can clear them, and the few that fall in the band are moved out of it by _group_nudge."""
    if case["id"] not in _group_cache:
        if "seed" in case:
            data = _group_raw(case, case["seed"])
        else:
            data = _group_nudge(case, _group_raw(case, 1 + sum(ord(c) for c in case["id"])))
        _group_cache[case["id"]] = data
    d = _group_cache[case["id"]]
    return dict(d, inits=[{k: v.clone() for k, v in sd.items()} for sd in d["inits"]])


def group_mixed_share(case, pres):
    """Per gated layer (attention_mlp?, linear_i): the share of (model, step, unit) columns whose gate is open for some rows of the
    minibatch and shut for others; the minimum over the layers.  Needs at least two rows."""
    worst = 1.0
    for att, i in GROUP_LEVELS:
        mixed = total = 0
        for g, s, name, z in pres:
            if name.startswith("attention_mlp") == att and name.endswith(f"linear_{i}") and z.shape[0] > 1:
                o = (z > 0).any(0) & (z <= 0).any(0)
                mixed, total = mixed + int(o.sum()), total + o.numel()
        if total:
            worst = min(worst, mixed / total)
    return worst


def _group_forward(sd, case, xs, drop_last_k=False, pre=None):
    """Attention / Attention_TOPN forward (attention.py:36-57) from oracle.fusion_ref's pieces, in the dtype of sd / xs."""
    from oracle import fusion_ref as O
    names = group_encoder_names(case)
    if drop_last_k:      # the mutation: the first hidden layer (encoder 0's linear_1, K = D[0]) loses its last k
        sd = dict(sd)
        key = f"{names[0]}.linear_1.weight"
        mask = torch.ones_like(sd[key])
        mask[:, -1] = 0
        sd[key] = sd[key] * mask
    if pre is not None:      # gated pre-activations, recomputed layer by layer
        def walk(prefix, x):
            for i in (1, 2, 3):
                z = F.linear(x, sd[f"{prefix}.linear_{i}.weight"], sd[f"{prefix}.linear_{i}.bias"])
                pre.append((f"{prefix}.linear_{i}", z.detach()))
                x = F.relu(z)
            return x
        enc_p = [walk(n, x) for n, x in zip(names, xs)]
        walk("attention_mlp", torch.cat(enc_p, dim=1))
    enc = [O.mlp_encoder(sd, n, x) for n, x in zip(names, xs)]
    mh = torch.cat(enc, dim=1)
    att = F.linear(O.mlp_encoder(sd, "attention_mlp", mh), sd["fc_att.weight"], sd["fc_att.bias"])
    fused = torch.matmul(torch.stack(enc, dim=2), att.unsqueeze(2)).squeeze(2)
    e = F.linear(fused, sd["fc_out_1.weight"], sd["fc_out_1.bias"])
    v = F.linear(fused, sd["fc_out_2.weight"], sd["fc_out_2.bias"]) if case["C2"] else None
    return e, v


def group_reference(case, data, mutate=None, collect_pre=False):
    """The fp64 reference of one case: per model g a dict of losses[s], emo[s] / val[s] (rows below the count; None when idle), grad0
    (flat gradient after step 0; None for the idle model), flat / m / v / step after both train steps.  Divisors are the model's row
    count n_g, autograd supplies the gradients, Adam is adam_ref (fp64 on the fp32-rounded hyper-parameters).
    mutate: "div_by_B" (the losses divided by B instead of n_g), "bias_over_B" (bias gradients summed over all B index rows instead
    of the first n_g), "drop_last_k" (the first hidden layer, encoder 0's linear_1, loses its last k)."""
    from oracle import fusion_ref as O
    G, B = 3, case["B"]
    spec = group_param_spec(case)
    out, pres = [], []
    for g in range(G):
        sd = {k: v.double() for k, v in data["inits"][g].items()}
        ms = {k: torch.zeros_like(v) for k, v in sd.items()}
        vs = {k: torch.zeros_like(v) for k, v in sd.items()}
        r = dict(losses=[], emo=[], val=[], grad0=None, step=0)
        for s in range(3):
            n = int(data["count"][s, g])
            if n == 0:
                r["losses"].append(None), r["emo"].append(None), r["val"].append(None)
                continue
            train = s < 2

            def loss_on(rows_n, prm, divisor, pre=None):
                rows = data["index"][s, g, :rows_n].long()
                e, v = _group_forward(prm, case, [f[rows].double() for f in data["feats"]], mutate == "drop_last_k", pre)
                loss = F.nll_loss(F.log_softmax(e, 1), data["emos"][rows], reduction="sum") / divisor
                if v is not None:
                    loss = loss + ((v.view(-1) - data["vals"][rows].double()) ** 2).sum() / divisor
                return loss, e, v

            prm = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.numel()}
            full = {**sd, **prm}
            pre = [] if collect_pre else None
            loss, e, v = loss_on(n, full, B if mutate == "div_by_B" else n, pre)
            if collect_pre:
                pres += [(g, s, name, z) for name, z in pre]
            r["losses"].append(loss.item()), r["emo"].append(e.detach()), r["val"].append(None if v is None else v.detach())
            if not train:
                continue
            grads = dict(zip(prm, torch.autograd.grad(loss, list(prm.values()))))
            if mutate == "bias_over_B" and n < B:
                prm2 = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.numel()}
                loss2, _, _ = loss_on(B, {**sd, **prm2}, n)
                g2 = dict(zip(prm2, torch.autograd.grad(loss2, list(prm2.values()))))
                grads.update({k: g2[k] for k in grads if k.endswith("bias")})
            grads = {k: grads.get(k, torch.zeros_like(sd[k])) for k in sd}
            if s == 0:
                r["grad0"] = torch.cat([grads[k].reshape(-1) for k, _ in spec])
            r["step"] += 1
            for k in sd:
                if sd[k].numel():
                    sd[k], ms[k], vs[k], _ = adam_ref(sd[k], grads[k], ms[k], vs[k], group_lr(case)[g], 0.9, 0.999, 1e-8, GROUP_WD[g], r["step"], GROUP_CLIP[g])
        r["flat"], r["m"], r["v"] = (torch.cat([d[k].reshape(-1) for k, _ in spec]) for d in (sd, ms, vs))
        out.append(r)
    return (out, pres) if collect_pre else out


def group_diff(a, b):
    """Worst max-norm relative difference between two group results per tolerance class: dict(loss, out, grad, param)."""
    w = dict(loss=0.0, out=0.0, grad=0.0, param=0.0)
    for ra, rb in zip(a, b):
        for s in range(3):
            if rb["losses"][s] is None:
                continue
            w["loss"] = max(w["loss"], abs(ra["losses"][s] - rb["losses"][s]) / max(abs(rb["losses"][s]), 1e-30))
            w["out"] = max(w["out"], max_rel(ra["emo"][s], rb["emo"][s]))
            if rb["val"][s] is not None:
                w["out"] = max(w["out"], max_rel(ra["val"][s], rb["val"][s]))
        if rb["grad0"] is not None:
            w["grad"] = max(w["grad"], max_rel(ra["grad0"], rb["grad0"]))
        w["param"] = max(w["param"], *(max_rel(ra[k], rb[k]) for k in ("flat", "m", "v")))
    return w


# --------------------------------------------------------------------------------------------------------------- mer_seq_bias
# (csrc/norm.hip: tests/test_seq_bias_gpu.py).  Restated from the words of include/mer_hip.h, not from the kernels.
SEQ_FIX = 16384.0          # the 2^-14 grid a sample is rounded to
SEQ_CLAMP = 131000.0       # ... after this clamp
SEQ_MAX_SAMPLES = 32


def seq_sample_stride(T):
    """The largest power of two s with 16 s <= T (1 for T < 16)."""
    return 1 << max((T // 16).bit_length() - 1, 0)


def seq_sample_rows(T, valid, rows_left, mutate=None):
    """The sampled rows of one sequence of T rows, relative to its first row: h, h + s, ... below min(valid, T, rows_left), s =
    seq_sample_stride(T), h = s / 2; rows_left = what the plane still holds from the sequence's first row on.
    mutate (the CPU sensitivity tests): "offset0", "stride2" (stride 2 s, offset kept), "drop_last", "no_valid"."""
    s = seq_sample_stride(T)
    h = 0 if mutate == "offset0" else s // 2
    lim = min(T, rows_left) if mutate == "no_valid" else min(valid, T, rows_left)
    rows = list(range(h, lim, 2 * s if mutate == "stride2" else s))
    return rows[:-1] if mutate == "drop_last" else rows


def round16_direct(x, dtype):
    """fp64 -> the 16-bit format in ONE round-to-nearest-even step, returned as fp64 (torch's own fp64 -> 16-bit cast goes through
    fp32).  No overflow handling: |x| stays below the format's largest value."""
    p, emin = (11, -13) if T16[dtype] == torch.float16 else (8, -125)        # x = m 2^e, m in [0.5, 1): one ulp is 2^(e - p)
    x = x.double()
    _, e = torch.frexp(x)
    q = torch.pow(torch.tensor(2.0, dtype=torch.float64), (e.clamp_min(emin) - p).double())
    return torch.round(x / q) * q


def seq_mean16_ref(a, seg_rows, valid=None, mutate=None):
    """The 16-bit mean plane [ceil(M / seg_rows), K] of a 16-bit plane a [M, K], as an integer model — bit for bit what the header
    promises: per sampled element rint(clamp(x, +-131000) 2^14) as int64 (ties to even; NaN counts as -131000), the samples summed,
    float64(sum) * (1.0 / (total * 16384.0)), rounded to fp32 and then to the plane's dtype, both to nearest even.  A sequence with
    no sample gives 0.  mutate: those of seq_sample_rows, and "no_f32" (fp64 -> 16 bits in one rounding)."""
    M, K = a.shape
    nseq = -(-M // seg_rows)
    out = torch.zeros((nseq, K), dtype=a.dtype)
    for s in range(nseq):
        v = seg_rows if valid is None else int(valid[s])
        rows = seq_sample_rows(seg_rows, v, M - s * seg_rows, mutate)
        if not rows:
            continue
        x = a[[s * seg_rows + r for r in rows]].double()
        x = torch.where(x.isnan(), torch.full_like(x, -SEQ_CLAMP), x.clamp(-SEQ_CLAMP, SEQ_CLAMP))
        total = torch.round(x * SEQ_FIX).to(torch.int64).sum(0)
        mean = total.double() * (1.0 / (len(rows) * SEQ_FIX))
        out[s] = round16_direct(mean, a.dtype).to(a.dtype) if mutate == "no_f32" else mean.float().to(a.dtype)
    return out


def seq_sample_mean64(a, seg_rows, valid=None):
    """The plain statement: the fp64 mean of the sampled rows themselves (finite inputs), 0 without a sample."""
    M, K = a.shape
    nseq = -(-M // seg_rows)
    out = torch.zeros((nseq, K), dtype=torch.float64)
    for s in range(nseq):
        rows = seq_sample_rows(seg_rows, seg_rows if valid is None else int(valid[s]), M - s * seg_rows)
        if rows:
            out[s] = a[[s * seg_rows + r for r in rows]].double().mean(0)
    return out


def seq_mean16_plain_bound(mean64, dtype):
    """|mean16 - fp64 mean of the samples| <= 2^-15 + one rounding to the dtype: every sample moves by at most half a grid step
    (2^-15) when it is put on the 2^-14 grid, so does their mean; the two final roundings (fp32, then the dtype) cost u |y| of the
    rounded value y, |y| <= |mean| + 2^-15, plus fp32's 2^-24 relative, and half the format's smallest subnormal step where y is
    subnormal (f16: 2^-25)."""
    m = mean64.abs() + 2.0 ** -15
    return 2.0 ** -15 + (U16[dtype] + 2.0 ** -24 + 2.0 ** -52) * m + 2.0 ** -25


def seq_ksplit(K):
    """How the table product splits K over its 16 waves: (per, [(k_lo, k_hi)] * 16) in k-steps of 32 — used by the k-slice
    mutation and the fp32 model only; the reference itself is a plain fp64 product."""
    ksteps = -(-K // 32)
    per = -(-ksteps // 16)
    return per, [(min(w * per * 32, K), min((w + 1) * per * 32, K)) for w in range(16)]


def seq_bias_table_ref(mean16, w_lo, bias=None, n_first=0, mutate=None):
    """fp64 table[s, n] = mean16[s] . w_lo[n] + bias[n]; columns below n_first are exactly bias (0 without one).
    mutate: "drop_kslice" (the second 32-wide k-step of wave 1 — or the last k-step, where K is too short — is left out),
    "n_first_block" (the plain range ends one 16-column block later), "n_clamp_low" (the last column reads the row before it),
    "no_n_clamp" (column n of a partial block reads row n of the w_lo BUFFER unclamped: w_lo must then hold ceil16(N) rows, and
    only the first N columns are written — see tests/test_op_refs_cpu.py for what that does and does not move)."""
    m, w = mean16.double(), w_lo.double()
    K = m.shape[1]
    N = w.shape[0]
    if mutate == "no_n_clamp":
        N = bias.shape[0] if bias is not None else N
        assert w.shape[0] >= -(-N // 16) * 16
        w = w[:-(-N // 16) * 16]
    if mutate == "drop_kslice":
        per, parts = seq_ksplit(K)
        k0 = parts[1][0] + 32 if parts[1][0] + 32 < parts[1][1] else (K - 1) // 32 * 32
        m = m.clone()
        m[:, k0:k0 + 32] = 0
    if mutate == "n_clamp_low":
        w = torch.cat([w[:-1], w[-2:-1]]) if N > 1 else w
    t = (m @ w.T)[:, :N]
    t[:, :min(n_first + (16 if mutate == "n_first_block" else 0), N)] = 0
    return t if bias is None else t + bias.double()


def seq_bias_bound(mean16, w_lo, bias=None, n_first=0):
    """Elementwise bound on |table - seq_bias_table_ref|: (K + 6) u S, u = 2^-24, S = |mean16| . |w_lo|^T + |bias|; 0 in the columns
    below n_first (they are the bias itself).  Counted as gemm32_bound counts: the product of two 16-bit values (11 or 8
    significand bits each) is exact in fp32, so only additions round; an output element is the root of a summation tree whose
    leaves are the K products: whatever order the MFMA and the k-loop take them in, no leaf lies under more than K additions
    inside its wave, 4 more in the fixed tree over the 16 k-split waves and 1 for the bias, each addition rounding its partial sum
    (<= the magnitude sum of what is below it) by at most u: (K + 5) u S to first order.  The sixth u covers the second-order terms
    of (1 + u)^(K + 5) for every K below 2^20.  Nothing here looks at the kernel's output."""
    m, w = mean16.double().abs(), w_lo.double().abs()
    S = m @ w.T
    if bias is not None:
        S = S + bias.double().abs()
    b = (m.shape[1] + 6) * U32 * S
    b[:, :min(n_first, b.shape[1])] = 0
    return b


def seq_bias_model32(mean16, w_lo, bias=None, n_first=0):
    """One admissible fp32 evaluation of the table: per wave of seq_ksplit a running fp32 sum over its k-steps (each k-step's 32
    products summed in fp32 by torch), the 16 partial sums through a pairwise tree, one bias add.  The CPU tests hold it to
    seq_bias_bound: the bound is not tighter than honest fp32 arithmetic."""
    m, w = mean16.float(), w_lo.float()
    K = m.shape[1]
    parts = []
    for lo, hi in seq_ksplit(K)[1]:
        acc = torch.zeros((m.shape[0], w.shape[0]), dtype=torch.float32)
        for k in range(lo, hi, 32):
            acc = acc + m[:, k:min(k + 32, hi)] @ w[:, k:min(k + 32, hi)].T
        parts.append(acc)
    d = 1
    while d < 16:
        for i in range(0, 16, 2 * d):
            parts[i] = parts[i] + parts[i + d]
        d *= 2
    t = parts[0]
    t[:, :min(n_first, t.shape[1])] = 0
    return t if bias is None else t + bias.float()


def seq_grid_values(shape, seed, dtype):
    """Inputs on which the 2^-14 grid matters: magnitudes log-uniform over 2^-20 .. 8 with random signs, rounded to the dtype, every
    third element an exact tie (n + 0.5) 2^-14 with n in 0 .. 63 (representable in both formats), every 29th an exact zero."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for d in shape:
        n *= d
    x = 2.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 23.0 - 20.0)
    x = x * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    tie = (torch.randint(0, 64, (n,), generator=g).double() + 0.5) / SEQ_FIX * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    idx = torch.arange(n)
    x = torch.where(idx % 3 == 1, tie, x)
    x = torch.where(idx % 29 == 5, torch.zeros_like(x), x)
    return x.float().to(T16[dtype]).view(shape)
